"""float64 numpy restatement of the sparse-tap resampler as include/mfpa.h states it for mfpa_resample_sparse*: per phase i only the
S = support taps from k = first[i] on, and every output one ascending chain over them,
    y[j * n + i] = chain over u = 0 .. S-1 of acc = taps[i, u] * xpad[j * o + first[i] + u] + acc,   xpad[m] = x[m - width] or 0.
Geometry, filter width and rolloff are those of tests/_resample_oracle.py (imported).  Its tap formula is one function over the
whole (n, K) bank, which is exactly what must never be formed here (288 MB for 8979 : 8000), so the same expression is evaluated
on index arrays (`taps64_at`); tests/test_resample_sparse_oracle.py pins it to _resample_oracle.taps64 value for value."""
import math

import numpy as np

from tests import _resample_oracle as ro

LPW = ro.LOWPASS_FILTER_WIDTH


def geometry(orig_freq, new_freq):
    """(o, n, width, K, S): S = 2 * width + 1 rounded up to a multiple of 4."""
    o, n, width, K = ro.geometry(orig_freq, new_freq)
    return o, n, width, K, (2 * width + 1 + 3) // 4 * 4


def window_argument(orig_freq, new_freq, i, k):
    """t of tap k of phase i BEFORE its clamp to +-LPW, float64, in _resample_oracle.taps64's order of operations (i, k: integer
    arrays that broadcast)."""
    o, n, width, _ = ro.geometry(orig_freq, new_freq)
    base = min(o, n) * ro.ROLLOFF
    phase = ((-np.asarray(i)).astype(np.float32) / np.float32(n)).astype(np.float64)
    return (phase + (np.asarray(k) - width).astype(np.float64) / o) * base


def taps64_at(orig_freq, new_freq, i, k):
    """_resample_oracle.taps64(orig, new)[i, k] without the bank."""
    o, n, _, _ = ro.geometry(orig_freq, new_freq)
    base = min(o, n) * ro.ROLLOFF
    t = np.clip(window_argument(orig_freq, new_freq, i, k), -LPW, LPW)
    win = np.cos(t * math.pi / LPW / 2) ** 2
    t = t * math.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(t == 0, 1.0, np.sin(t) / t)
    return sinc * win * (base / o)


def first(orig_freq, new_freq):
    """(n,) int64: the first k >= 0 of each phase with t > -LPW, found with the float64 t itself around the real-number estimate
    width + o * (i / n - LPW / base)."""
    o, n, width, _ = ro.geometry(orig_freq, new_freq)
    base = min(o, n) * ro.ROLLOFF
    i = np.arange(n)
    est = np.floor(width + o * (i / n - LPW / base)).astype(np.int64)
    cand = est[:, None] + np.arange(-2, 4)[None, :]
    inside = window_argument(orig_freq, new_freq, i[:, None], cand) > -LPW
    assert not inside[:, 0].any() and inside[:, -1].all()                 # the estimate brackets the edge
    return np.maximum(cand[i, inside.argmax(axis=1)], 0)


def taps32(orig_freq, new_freq):
    """(taps (n, S) float32, first (n,)): row i holds taps first[i] .. first[i] + S - 1 of the dense row i, 0 where k >= K."""
    o, n, width, K, S = geometry(orig_freq, new_freq)
    f = first(orig_freq, new_freq)
    k = f[:, None] + np.arange(S)[None, :]
    taps = taps64_at(orig_freq, new_freq, np.arange(n)[:, None], k).astype(np.float32)
    taps[k >= K] = 0.0
    return taps, f


def resample(x, orig_freq, new_freq):
    """(B, L) -> (y (B, Tout) float64, bound = conv(|taps|, |x|)) with the float32 taps: the contract above, ascending in u."""
    x = np.asarray(x, dtype=np.float64)
    o, n, width, K, S = geometry(orig_freq, new_freq)
    B, L = x.shape
    Tout = ro.out_len(orig_freq, new_freq, L)
    taps, f = taps32(orig_freq, new_freq)
    taps = taps.astype(np.float64)
    q = np.arange(Tout)
    j, i = q // n, q % n
    start = j * o + f[i]                                                  # in xpad coordinates
    xpad = np.zeros((B, int(start.max(initial=0)) + S + 1))
    m = min(L, xpad.shape[1] - width)
    if m > 0:
        xpad[:, width:width + m] = x[:, :m]
    y = np.zeros((B, Tout))
    bound = np.zeros((B, Tout))
    for u in range(S):
        y = taps[i, u][None, :] * xpad[:, start + u] + y
        bound = np.abs(taps[i, u])[None, :] * np.abs(xpad[:, start + u]) + bound
    return y, bound
