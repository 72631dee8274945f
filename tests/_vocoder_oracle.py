"""numpy restatement of mfpa_phase_vocoder (include/mfpa.h): torchaudio.functional.phase_vocoder at 257 bins / hop 256 with one rate
per clip, parametrised by the dtype of its arithmetic.  tests/test_vocoder_oracle.py checks it against the same formula written in
torch ops (torchaudio's source as text; torchaudio itself is not in the reference tree, parity with it is unpinned).

Error unit of every vocoder test: E(spec, rates) = max |oracle in float64 - oracle in np.longdouble|.  Both use the same float64 pi,
the same float64 time steps t = i r (so the same frames j and weights alpha) and the same order of additions: they differ by
rounding only, and E is the float64 rounding error of this formula on this input.  It is dominated by the running sum: phases grow
to 256 pi per frame at the top bin, so after n frames one rounding is about n * 1e-13 and E about |Z| n^1.5 * 1e-13 -- 1e-12 at
4 frames, 4e-8 at 502 frames for |Z| = 15.  Bounds are 8 E, the convention of tests/_istft_oracle.py.
Where np.longdouble is no wider than float64 (eps >= 2e-19) there is no unit: HAVE_LONGDOUBLE is False and the callers skip."""
import functools
import math

import numpy as np
import torch

from tests import _istft_oracle as io

N_BINS, N_HOP = 257, 256
MAX_FRAMES = 16384
HAVE_LONGDOUBLE = bool(np.finfo(np.longdouble).eps < 2e-19)
PI = np.float64(math.pi)


def frames(n_frames, rate):
    """ceil(n_frames / rate) in double = len(np.arange(0, n_frames, rate)); -1 for a rate that is not finite or not positive."""
    rate = float(rate)
    if not (rate > 0.0 and math.isfinite(rate)):
        return -1
    return int(math.ceil(n_frames / rate))


def phase_advance(dtype=np.float64):
    """torch.linspace(0, pi * 256, 257) in `dtype`: pi k, rounded once.  torch counts the upper half from the end, 256 pi - pi (256 - k):
    the same numbers where its kernel fuses the multiply-add (256 pi is exact), one float64 ulp away at 8 bins where it does not."""
    return dtype(PI) * np.arange(N_BINS).astype(dtype)


def clip(spec, rate, dtype=np.float64):
    """One clip: spec (257, n_frames) complex -> (real, imag) of the (257, n_out) output, each of `dtype`; None for a refused rate."""
    spec = np.asarray(spec, dtype=np.complex128)
    bins, nF = spec.shape
    assert bins == N_BINS and nF >= 1
    n_out = frames(nF, rate)
    if n_out < 0:
        return None
    re, im = spec.real.astype(dtype), spec.imag.astype(dtype)
    if float(rate) == 1.0:
        return re, im
    t = np.arange(n_out, dtype=np.float64) * np.float64(rate)                # float64 in every dtype: the same j and alpha
    j = np.floor(t).astype(np.int64)
    alpha = (t - np.floor(t)).astype(dtype)[None, :]
    assert j.max() <= nF + 1
    re = np.concatenate([re, np.zeros((bins, 2), dtype=dtype)], axis=1)      # torchaudio pads two zero frames
    im = np.concatenate([im, np.zeros((bins, 2), dtype=dtype)], axis=1)
    a0, a1 = np.arctan2(im[:, j], re[:, j]), np.arctan2(im[:, j + 1], re[:, j + 1])
    n0, n1 = np.hypot(re[:, j], im[:, j]), np.hypot(re[:, j + 1], im[:, j + 1])
    adv = phase_advance(dtype)[:, None]
    two_pi = dtype(2.0) * dtype(PI)
    d = a1 - a0 - adv
    d = d - two_pi * np.round(d / two_pi)
    inc = d + adv
    phase0 = np.arctan2(im[:, :1], re[:, :1])
    phi = np.cumsum(np.concatenate([phase0, inc[:, :-1]], axis=1), axis=1, dtype=dtype)
    mag = alpha * n1 + (dtype(1.0) - alpha) * n0
    return (mag * np.cos(phi)).astype(dtype), (mag * np.sin(phi)).astype(dtype)


def phase_vocoder(spec, rates, ld_out=None):
    """The kernel's output in float64: spec (B, 257, n_frames), rates a number or (B,) -> (out (B, 257, ld_out) complex128, n_out
    (B,) int32).  ld_out defaults to the largest n_out; a clip whose rate is refused or whose n_out exceeds ld_out is zeros, -1."""
    spec = np.asarray(spec, dtype=np.complex128)
    B, _, nF = spec.shape
    rates = np.broadcast_to(np.asarray(rates, dtype=np.float64), (B,))
    n = np.array([frames(nF, r) for r in rates], dtype=np.int64)
    if ld_out is None:
        ld_out = int(max(n.max(), 1))
    n = np.where(n > ld_out, -1, n).astype(np.int32)
    out = np.zeros((B, N_BINS, ld_out), dtype=np.complex128)
    for b in range(B):
        if n[b] >= 0:
            re, im = clip(spec[b], rates[b])
            out[b, :, :n[b]] = re + 1j * im
    return out, n


def error_unit(spec, rates):
    """E of the module docstring."""
    assert HAVE_LONGDOUBLE
    spec = np.asarray(spec, dtype=np.complex128)
    rates = np.broadcast_to(np.asarray(rates, dtype=np.float64), (spec.shape[0],))
    E = 0.0
    for b in range(spec.shape[0]):
        lo, hi = clip(spec[b], rates[b]), clip(spec[b], rates[b], np.longdouble)
        if lo is not None and lo[0].size:
            E = max(E, float(np.abs(lo[0] - hi[0]).max()), float(np.abs(lo[1] - hi[1]).max()))
    return E


def stretched_length(T, rate):
    return int(round(T / float(rate)))


# ----------------------------------------------------------------------------- shared inputs and the frequency estimator
SR = 8000
TONES = (250.0, 440.0, 1000.0, 1234.5, 3300.0)
TONE_RATES = (0.8, 0.9, 0.95, 1.05, 1.1, 1.25, 2.0 ** (1 / 12), 2.0 ** (-1 / 12))


@functools.lru_cache(maxsize=None)
def noise_spectrum(T, B=3):
    x = torch.rand(B, T, generator=torch.Generator().manual_seed(77 * B + T)) * 2 - 1
    return io.torch_stft(x).numpy()


def dominant_frequency(y, sr=SR):
    """Peak of the Hann-windowed rFFT, refined by a parabola through the log magnitudes of the peak bin and its neighbours."""
    y = np.asarray(y, dtype=np.float64)
    m = np.abs(np.fft.rfft(y * np.hanning(len(y))))
    k = int(np.argmax(m[1:-1])) + 1
    a, b, c = np.log(m[k - 1]), np.log(m[k]), np.log(m[k + 1])
    return (k + 0.5 * (a - c) / (a - 2 * b + c)) * sr / len(y)


def middle_half(y):
    n = len(y)
    return y[n // 4: n // 4 + n // 2]


@functools.lru_cache(maxsize=None)
def tones(T=64000):
    t = np.arange(T) / SR
    return torch.from_numpy(np.stack([0.5 * np.sin(2 * np.pi * f * t) for f in TONES]).astype(np.float32))
