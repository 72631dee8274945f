"""The spectral noise suppressor's definition (include/mfpa.h, mfpa_spectral_suppress) restated in numpy float64: vectorised over
(B, F), a loop over the frames, every product, sum and quotient rounded on its own in the order written.  min and max are np.fmin
and np.fmax, which select and never round, so the device's block scheme for the sliding minimum gives the same bits; everything else
is a serial chain of correctly rounded operations.  The device is compared with this bit for bit (tests/test_gpu_denoise.py)."""
import numpy as np

DBL_MIN = np.finfo(np.float64).tiny
MAX_WINDOW = 128                                          # MFPA_DENOISE_MAX_WINDOW
BINS, CHUNK, GROUP = 16, 64, 16                           # csrc/denoise.hip: bins per workgroup, frames per tile, frames per lane in the minimum
DEFAULTS = dict(alpha=0.7, back=48, ahead=48, bias=3.0, a=0.9, xi_min=10.0 ** (-25.0 / 10.0), g_floor=10.0 ** (-20.0 / 20.0))

WINDOWS = [(0, 0), (0, 5), (5, 0), (48, 48), (63, 64)]   # the last is the maximum window, W = 128
F_LIST = [1, 63, 64, 65, 257]


def frames_list(back=48, ahead=48):
    W = back + ahead + 1
    raw = [1, 2, ahead, ahead + 1, W - 1, W, W + 1, 63, 64, 65, 251, 2 * W + 3, 1500,
           GROUP - 1, GROUP, GROUP + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1]
    return sorted({n for n in raw if n >= 1})


def sliding_min(s, back, ahead):
    """min{ s[..., u] : max(0, t - back) <= u <= min(nF - 1, t + ahead) } by brute force."""
    nF = s.shape[-1]
    out = np.empty_like(s)
    for t in range(nF):
        out[..., t] = s[..., max(0, t - back):min(nF - 1, t + ahead) + 1].min(axis=-1)
    return out


def smooth(p, alpha):
    s = np.empty_like(p)
    one_minus = 1.0 - alpha
    s[..., 0] = p[..., 0]
    for t in range(1, p.shape[-1]):
        s[..., t] = alpha * s[..., t - 1] + one_minus * p[..., t]
    return s


def suppress(m, *, alpha=DEFAULTS["alpha"], back=48, ahead=48, bias=3.0, a=0.9, xi_min=DEFAULTS["xi_min"], g_floor=DEFAULTS["g_floor"],
             noise=None, denom=None, apply=None):
    """(y, g, n), float64 (B, F, nF).  m (B, F, nF) float32 or float64; noise (B, F); denom (B,); apply (B,) of booleans."""
    m = np.asarray(m).astype(np.float64)
    B, F, nF = m.shape
    p = m * m
    if noise is None:
        n = bias * sliding_min(smooth(p, alpha), back, ahead)
    else:
        n = np.broadcast_to(np.asarray(noise, dtype=np.float64)[:, :, None], m.shape).copy()
    g = np.empty_like(m)
    one_minus_a = 1.0 - a
    carry = None
    with np.errstate(all="ignore"):
        for t in range(nF):
            d = np.fmax(n[..., t], DBL_MIN)
            q = p[..., t] / d
            inst = np.fmax(q - 1.0, 0.0)
            dd = np.full_like(q, a) if t == 0 else a * carry
            xi = np.fmax(dd + one_minus_a * inst, xi_min)
            g[..., t] = np.fmax(1.0 - 1.0 / (1.0 + xi), g_floor)
            carry = (g[..., t] * g[..., t]) * q
    if apply is not None:
        off = ~np.asarray(apply, dtype=bool)
        g[off] = 1.0
        n[off] = 0.0
    y = g * m
    if denom is not None:
        y = y / np.asarray(denom, dtype=np.float64)[:, None, None]
    return y, g, n


def magnitudes(F, nF, seed=0):
    """(5, F, nF) float64: |N(0,1)| * 10^U(-3, 2); row 1 exact zeros for its first 60 frames, row 2 all zeros, row 3 constant."""
    rng = np.random.default_rng([seed, F, nF])
    m = np.abs(rng.standard_normal((5, F, nF))) * 10.0 ** rng.uniform(-3.0, 2.0, (5, F, nF))
    m[1, :, :60] = 0.0
    m[2] = 0.0
    m[3] = 0.37
    return m


# ----------------------------------------------------------------------------- the chain's inputs: noise-free tonal clips plus noise
def tonal(n=32000, rate=8000, seed=0):
    """Decaying harmonic notes, no noise of their own (synth.clip carries broadband noise at -20 dB: the suppressor rightly removes it)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    x = np.zeros(n)
    for start in np.arange(0.0, n / rate, 0.25):
        f0 = 110.0 * 2.0 ** (rng.integers(0, 36) / 12.0)
        env = np.where(t >= start, np.exp(-(t - start) / 0.4), 0.0)
        for h in range(1, 6):
            if f0 * h < 0.45 * rate:
                x += env * np.sin(2.0 * np.pi * f0 * h * t + rng.uniform(0, 2 * np.pi)) / h
    return x / np.abs(x).max()


def coloured(n, kind, seed=1):
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(n)
    if kind == "pink":
        X = np.fft.rfft(w)
        f = np.arange(X.size, dtype=np.float64)
        f[0] = 1.0
        w = np.fft.irfft(X / np.sqrt(f), n)
    return w


def noisy(clean, kind, snr_db, seed=1):
    w = coloured(clean.size, kind, seed)
    w *= np.sqrt(np.mean(clean ** 2) / np.mean(w ** 2)) * 10.0 ** (-snr_db / 20.0)
    return clean + w


def snr_db(clean, estimate):
    return 10.0 * np.log10(np.sum(clean ** 2) / np.sum((clean - estimate) ** 2))


CHAIN_CASES = [("white", 0.0), ("white", 10.0), ("pink", 0.0), ("pink", 10.0)]


def chain(wav, **kw):
    """torch.stft in float64 on the CPU (the pipeline's transform: 512 points, hop 256, the window np.hanning(514)[1:-1]), the
    oracle, torch.istft."""
    import torch
    x = torch.from_numpy(np.asarray(wav, dtype=np.float64))[None]
    win = torch.from_numpy(np.hanning(514)[1:-1].copy())
    spec = torch.stft(x, 512, 256, 512, win, center=True, pad_mode="reflect", return_complex=True)
    mag = spec.abs().numpy()
    _, g, _ = suppress(mag, **kw)
    out = torch.istft(spec * torch.from_numpy(g), 512, 256, 512, win, center=True, length=x.shape[1])
    return out[0].numpy()
