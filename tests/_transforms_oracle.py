"""Float64 restatements for the composable transforms (csrc/transforms.hip), numpy on the CPU.

  colored_noise   AddColoredNoise._gen_noise (reference augmentation/transformations/colored_noise.py:12-38) for GIVEN white
                  noise: rfft, 1 / linspace(1, sqrt(N/2), N/2+1)^f_decay, irfft(n=N), x / (rms + 1e-8), tiled to T.  Pinned by
                  golden g19 (the real _gen_noise in float32) to float32 rounding.
  bandpass_taps   julius 0.2.7 BandPassFilter restated (julius is in neither tree: PARITY UNPINNED, like oracle.augment's
                  low-pass): two windowed-sinc low-passes on the window of the LOWER cut-off, each of unit sum, subtracted.
  bandpass / bandstop   replicate-pad by half, correlate;  x - bandpass.
"""
from __future__ import annotations

import numpy as np

ZEROS = 8


def colored_noise(white, f_decay, T: int) -> np.ndarray:
    """white (..., N) -> (..., T) float64; f_decay a scalar or (...,)."""
    white = np.asarray(white, dtype=np.float64)
    N = white.shape[-1]
    fd = np.asarray(f_decay, dtype=np.float64)[..., None]
    mask = 1.0 / np.linspace(1.0, np.sqrt(N / 2.0), N // 2 + 1) ** fd
    x = np.fft.irfft(np.fft.rfft(white, axis=-1) * mask, n=N, axis=-1)
    x = x / (np.sqrt(np.mean(x * x, axis=-1, keepdims=True)) + 1e-8)
    return np.tile(x, -(-T // N))[..., :T]


def lowpass_taps_on(cutoff: float, half: int) -> np.ndarray:
    """One julius low-pass on a window of 2*half+1 points: 2c hann(k) sinc(2c pi (k - half)), normalised to unit sum."""
    n = 2 * half + 1
    k = np.arange(n, dtype=np.float64)
    window = 0.5 - 0.5 * np.cos(2.0 * np.pi * k / (n - 1))                # torch.hann_window(n, periodic=False)
    t = k - half
    taps = 2 * cutoff * window * np.sinc(2 * cutoff * t)                  # np.sinc(x) = sin(pi x) / (pi x)
    return taps / taps.sum()


def band_half(lo: float) -> int:
    return int(ZEROS / lo / 2)


def bandpass_taps(lo: float, hi: float) -> np.ndarray:
    if hi > 0.5 or lo > 0.5:
        raise ValueError("A cutoff above 0.5 does not make sense.")
    half = band_half(lo)
    return lowpass_taps_on(hi, half) - lowpass_taps_on(lo, half)


def bandpass(x, lo: float, hi: float) -> np.ndarray:
    """x (T,) -> (T,) float64."""
    x = np.asarray(x, dtype=np.float64)
    taps = bandpass_taps(lo, hi)
    half = (len(taps) - 1) // 2
    xp = np.concatenate([np.full(half, x[0]), x, np.full(half, x[-1])])
    if len(taps) * len(x) > 1 << 22:
        from scipy.signal import fftconvolve
        return fftconvolve(xp, taps[::-1], mode="valid")
    return np.correlate(xp, taps, mode="valid")


def bandstop(x, lo: float, hi: float) -> np.ndarray:
    return np.asarray(x, dtype=np.float64) - bandpass(x, lo, hi)


def g19_cases(g):
    """(rate, white (N,), f_decay, T, golden (T,)) of tests/golden/g19_colored_noise.npz."""
    for sr in g["rates"].tolist():
        for i, fd in enumerate(g["f_decay"].tolist()):
            for T in (sr + 7, sr // 2 + 3):
                yield sr, g[f"white_{sr}"], fd, T, g[f"noise_{sr}_{i}_{T}"]


def reference_error(g):
    """{rate: max over the g19 cases of that rate of max|golden - oracle|}: the reference's own float32 distance from the float64
    result (unit-RMS signals, so absolute = relative to the RMS)."""
    err = {}
    for sr, white, fd, T, y in g19_cases(g):
        err[sr] = max(err.get(sr, 0.0), float(np.abs(y.astype(np.float64) - colored_noise(white, fd, T)).max()))
    return err
