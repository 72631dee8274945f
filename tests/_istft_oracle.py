"""numpy float64 restatement of mfpa_istft (include/mfpa.h): torch.istft(Z, 512, 256, window=w, center=True, length=length) at the
library's fixed geometry, with the magnitude rule Z = m * spec / |spec| applied first.  tests/test_istft_oracle.py checks it against
torch.istft on the CPU; the GPU tests use it where torch has no equivalent (the magnitude rule, the clamp).

Also the error unit of every inverse-STFT test: E(x) = max |torch.istft(torch.stft(x.double())) - x|, torch's own float64 round-trip
error on that input (torch_stft, torch_istft, error_unit below).  Bounds are 8 E: two independent float64 implementations may each
be off by about E, their FFTs round differently (numpy's and torch's pocketfft, the device's 16 x 16 network), the rest is margin.
E is a few float64 ulps of the largest sample -- 4e-16 to 1e-15 for samples in [-1, 1] -- and grows where the kept range ends
under one thin window tail: 2e-13 ... 2e-12 at T = 511, 5e-15 at T = 1000."""
import numpy as np
import torch

N_FFT, N_HOP, N_BINS = 512, 256, 257
ENVELOPE_MIN = 1e-11                   # torch.istft refuses a smaller overlap-added squared window


def window():
    return np.hanning(N_FFT + 2)[1:-1]


def length_ok(n_frames, length):
    return n_frames >= 2 and N_HOP * (n_frames - 1) <= length < N_HOP * n_frames


def apply_magnitude(spec, mag, denom=None, clamp=False):
    """Z[b,k,t] = m * spec / |spec|, m = mag * denom[b]; phase 0 where |spec| == 0; clamp: a negative m becomes 0."""
    spec = np.asarray(spec, dtype=np.complex128)
    m = np.asarray(mag).astype(np.float64)
    if denom is not None:
        m = m * np.asarray(denom, dtype=np.float64)[:, None, None]
    if clamp:
        m = np.where(m < 0, 0.0, m)
    r = np.hypot(spec.real, spec.imag)
    safe = np.where(r == 0, 1.0, r)
    return np.where(r == 0, m + 0j, m * (spec.real / safe) + 1j * (m * (spec.imag / safe)))


def envelope(win, n_frames):
    """The overlap-added squared window over the padded signal's 256 * (n_frames + 1) samples, frames added in order."""
    env = np.zeros(N_HOP * (n_frames + 1))
    w2 = np.asarray(win, dtype=np.float64) ** 2
    for t in range(n_frames):
        env[N_HOP * t:N_HOP * t + N_FFT] += w2
    return env


def envelope_min(win, n_frames, length):
    assert length_ok(n_frames, length)
    return float(envelope(win, n_frames)[N_HOP:N_HOP + length].min())


def istft(spec, length=None, mag=None, denom=None, clamp=False, win=None):
    """(B, 257, n_frames) complex -> (B, length) float64.  Raises RuntimeError where torch.istft does (the envelope minimum)."""
    win = window() if win is None else np.asarray(win, dtype=np.float64)
    Z = np.asarray(spec, dtype=np.complex128) if mag is None else apply_magnitude(spec, mag, denom, clamp)
    B, bins, nF = Z.shape
    assert bins == N_BINS
    length = N_HOP * (nF - 1) if length is None else length
    assert length_ok(nF, length)
    env = envelope(win, nF)
    if not env[N_HOP:N_HOP + length].min() >= ENVELOPE_MIN:
        raise RuntimeError("window overlap add min")
    Z = Z.copy()
    Z[:, 0] = Z[:, 0].real                                 # the c2r transform ignores the imaginary parts of bins 0 and 256
    Z[:, N_BINS - 1] = Z[:, N_BINS - 1].real
    frames = np.fft.irfft(Z, n=N_FFT, axis=1) * win[None, :, None]           # (B, 512, nF)
    y = np.zeros((B, N_HOP * (nF + 1)))
    for t in range(nF):
        y[:, N_HOP * t:N_HOP * t + N_FFT] += frames[:, :, t]
    return y[:, N_HOP:N_HOP + length] / env[N_HOP:N_HOP + length]


def torch_stft(x):
    return torch.stft(x.double(), N_FFT, N_HOP, window=torch.from_numpy(window()), return_complex=True)


def torch_istft(Z, length):
    return torch.istft(Z, N_FFT, N_HOP, window=torch.from_numpy(window()), center=True, length=length)


def error_unit(x):
    """E(x) of the module docstring for a (B, T) float32 tensor."""
    return float((torch_istft(torch_stft(x), x.shape[1]) - x.double()).abs().max())
