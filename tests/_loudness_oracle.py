"""Oracles of the loudness meter (csrc/loudness.hip), shared by tests/test_loudness_oracle.py (CPU) and tests/test_gpu_loudness.py:

  restate_*    the kernels' own order of operations in numpy float64 (include/mfpa.h states it): the filter is tests/_iir_oracle.py's
               restate() (the scan scheme of sosfilt_kernel), the segment sums go by the pairwise tree over a lane group's 16 squares, by each
               lane's running sum from super-chunk to super-chunk and by the binary tree over the 64 lanes; the gate sums go by the 256 strided partial
               sums and their tree; the ranks by a sort; the gain by one division, one square root and one product.  numpy rounds every
               operation on its own like the kernels (built without fused multiply-adds): the device result is this one bit for bit;
  plain_*      the plain float64 definition: scipy.signal.sosfilt and sequential sums;
  truth_*      the definition in numpy's long double (80-bit here): a serial cascade, long-double sums.

The error convention is the project's (tests/_iir_oracle.py): E = max |plain - truth| over a case, D = max |restated - truth|, and the
bound is D <= 8 E."""
import math

import numpy as np
import scipy.signal

from tests import _iir_oracle as io

L, LANES, SUPER, BOUND = io.L, io.LANES, io.SUPER, io.BOUND
GATE_BLOCK = 256
OFFSET = -0.691
INF = float("inf")


def hop_of(sample_rate) -> int:
    return int(math.floor(0.1 * sample_rate + 0.5))


def power_of(lufs) -> float:
    return 10.0 ** ((float(lufs) - OFFSET) / 10.0)


def lufs_of(power):
    with np.errstate(divide="ignore"):
        return OFFSET + 10.0 * np.log10(np.asarray(power, dtype=np.float64))


# ----------------------------------------------------------------------------- segments
def restate_filtered(x, sos) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    return io.restate(x, sos)[0] if sos is not None and len(sos) else x.copy()


def restate_segments(x, sos, hop: int, y=None):
    """One row (T,) -> (seg (T // hop,), peak) as loudness_segments_kernel computes them.  `y`: restate_filtered(x, sos) computed before."""
    x = np.asarray(x, dtype=np.float64)
    T = len(x)
    y = restate_filtered(x, sos) if y is None else y
    sq = np.zeros(-(-T // SUPER) * SUPER)
    sq[:T] = y * y
    sq = sq.reshape(-1, LANES, L)
    nseg = T // hop
    lanes = np.zeros((nseg, LANES))                                            # every lane's running sum of every segment starts at 0
    offs = np.arange(LANES)[:, None] * L + np.arange(L)[None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(len(sq)):                                               # super-chunk by super-chunk, all its segments at once
            k = np.arange(c * SUPER // hop, min(nseg - 1, ((c + 1) * SUPER - 1) // hop) + 1)
            if not len(k):
                continue
            n = (c * SUPER + offs)[None]
            inside = (n >= (k * hop)[:, None, None]) & (n < ((k + 1) * hop)[:, None, None])
            t = np.where(inside, sq[c][None], 0.0)                             # (segments, 64, 16)
            while t.shape[2] > 1:                                              # a lane group's squares: neighbours first, four levels
                t = t[:, :, 0::2] + t[:, :, 1::2]
            lanes[k] = lanes[k] + t[:, :, 0]
        while lanes.shape[1] > 1:                                              # the butterfly with offsets 1, 2, ..., 32: neighbours first
            lanes = lanes[:, 0::2] + lanes[:, 1::2]
    return lanes[:, 0], float(np.fmax.reduce(np.abs(x), initial=0.0))


def plain_segments(x, sos, hop: int) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    y = scipy.signal.sosfilt(sos, x) if sos is not None and len(sos) else x
    sq = y * y
    return np.array([np.add.accumulate(sq[k * hop:(k + 1) * hop])[-1] for k in range(len(x) // hop)])


def truth_segments(x, sos, hop: int) -> np.ndarray:
    x = np.asarray(x, dtype=np.longdouble)
    y = io.truth(x, sos)[0] if sos is not None and len(sos) else x
    sq = y * y
    return np.array([np.sum(sq[k * hop:(k + 1) * hop]) for k in range(len(x) // hop)], dtype=np.longdouble)


# ----------------------------------------------------------------------------- gate
def _weights(weights, C, dtype):
    return np.ones(C, dtype=dtype) if weights is None else np.asarray(weights, dtype=dtype)


def block_powers(seg, hop: int, win: int, weights=None) -> np.ndarray:
    """seg (C, nseg) -> (nb,): k increasing inside the block, then c increasing; the kernel's operations in seg's dtype."""
    seg = np.asarray(seg)
    C, nseg = seg.shape
    nb = max(0, nseg - win + 1)
    G = _weights(weights, C, seg.dtype)
    d = seg.dtype.type(win) * seg.dtype.type(hop)
    p = np.zeros(nb, dtype=seg.dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(C):
            a = seg[c, 0:nb].copy()
            for i in range(1, win):
                a = a + seg[c, i:i + nb]
            t = G[c] * (a / d)
            p = t if c == 0 else p + t
    return p


def _strided_sum(p, member):
    """(sum, count) of p over `member` in the kernel's order: 256 strided partial sums, then the tree with offsets 128, ..., 1."""
    a = np.zeros(GATE_BLOCK)
    for j0 in range(0, len(p), GATE_BLOCK):
        m = min(GATE_BLOCK, len(p) - j0)
        with np.errstate(invalid="ignore", over="ignore"):
            a[:m] = np.where(member[j0:j0 + m], a[:m] + p[j0:j0 + m], a[:m])
    off = GATE_BLOCK // 2
    while off:
        with np.errstate(invalid="ignore", over="ignore"):
            a[:off] = a[:off] + a[off:2 * off]
        off //= 2
    return a[0], int(np.count_nonzero(member))


def rank_indices(n: int):
    return (n + 4) // 10, (19 * n - 9) // 20


def restate_gate(seg, hop: int, win: int = 4, rel: float = 0.1, weights=None, p_abs: float = None) -> dict:
    """One example: seg (C, nseg) float64 -> what loudness_gate_kernel returns."""
    p_abs = power_of(-70.0) if p_abs is None else p_abs
    p = block_powers(np.asarray(seg, dtype=np.float64), hop, win, weights)
    with np.errstate(invalid="ignore"):
        above = p > p_abs
        s_abs, n_abs = _strided_sum(p, above)
        m_abs = s_abs / np.float64(n_abs) if n_abs else 0.0
        thr = np.float64(rel) * m_abs
        both = above & (p > thr)
    s_rel, n_rel = _strided_sum(p, both)
    kept = np.sort(p[both])
    lo, hi = rank_indices(n_rel)
    return dict(power=s_rel / np.float64(n_rel) if n_rel else 0.0, abs_power=m_abs, n_abs=n_abs, n_rel=n_rel, blocks=p,
                lo=kept[lo] if n_rel else 0.0, hi=kept[hi] if n_rel else 0.0)


def definition_gate(seg, hop: int, win: int = 4, rel: float = 0.1, weights=None, p_abs: float = None, dtype=np.float64) -> dict:
    """The gate by sequential (float64) or long-double sums; `margin`: the smallest relative distance of a block power from a gate
    threshold it is compared with."""
    p_abs = power_of(-70.0) if p_abs is None else p_abs
    p = block_powers(np.asarray(seg, dtype=dtype), hop, win, weights)
    total = (lambda v: np.add.accumulate(v)[-1]) if dtype is np.float64 else np.sum
    above = p > p_abs
    margin = float(np.min(np.abs(p / dtype(p_abs) - 1))) if len(p) else INF
    m_abs = total(p[above]) / dtype(np.count_nonzero(above)) if above.any() else dtype(0)
    both = above & (p > dtype(rel) * m_abs)
    if above.any() and m_abs > 0:
        margin = min(margin, float(np.min(np.abs(p[above] / (dtype(rel) * m_abs) - 1))))
    n = int(np.count_nonzero(both))
    kept = np.sort(p[both])
    lo, hi = rank_indices(n)
    return dict(power=total(p[both]) / dtype(n) if n else dtype(0), abs_power=m_abs, n_abs=int(np.count_nonzero(above)), n_rel=n, blocks=p,
                lo=kept[lo] if n else dtype(0), hi=kept[hi] if n else dtype(0), margin=margin)


# ----------------------------------------------------------------------------- gain
def restate_gain(x, p_gated, p_target, peak=None, peak_limit=None, apply=None):
    """x (B, C, T) float32 or float64 -> (y in x's dtype, g (B,)) as loudness_apply_kernel computes them."""
    x = np.asarray(x)
    B = x.shape[0]
    y, g_out = x.copy(), np.ones(B)
    for b in range(B):
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            g = np.sqrt(np.float64(p_target[b]) / np.float64(p_gated[b]))
            if peak_limit is not None:
                lim = np.float64(peak_limit) / np.max(peak[b])
                g = lim if lim < g else g
        if p_gated[b] == 0.0 or not np.isfinite(g) or (apply is not None and not apply[b]):
            continue
        y[b] = (x[b].astype(np.float64) * g).astype(x.dtype)
        g_out[b] = g
    return y, g_out


# ----------------------------------------------------------------------------- whole meters (plain float64: the conformance figures)
def plain_loudness(x, sample_rate, sos, win: int = 4, rel: float = 0.1, weights=None) -> dict:
    """x (C, T) -> the plain gate of the plain segments."""
    hop = hop_of(sample_rate)
    seg = np.stack([plain_segments(row, sos, hop) for row in np.asarray(x, dtype=np.float64)])
    return definition_gate(seg, hop, win, rel, weights)


def lra_of(lo, hi) -> float:
    return float(10.0 * np.log10(hi / lo)) if lo > 0 else 0.0


def sine(freq, sample_rate, seconds, dbfs, channels: int = 1, phase: float = 0.0) -> np.ndarray:
    """(channels, T) float64: the same sine in every channel."""
    n = np.arange(int(round(seconds * sample_rate)))
    return np.tile(10.0 ** (dbfs / 20.0) * np.sin(2.0 * np.pi * freq * n / sample_rate + phase), (channels, 1))


def steps(sample_rate, parts, freq: float = 1000.0, channels: int = 2) -> np.ndarray:
    """A stereo sine whose level steps: parts = [(dbfs, seconds), ...], one continuous phase."""
    T = [int(round(s * sample_rate)) for _, s in parts]
    n = np.arange(sum(T))
    amp = np.concatenate([np.full(t, 10.0 ** (d / 20.0)) for (d, _), t in zip(parts, T)])
    return np.tile(amp * np.sin(2.0 * np.pi * freq * n / sample_rate), (channels, 1))


TECH_3341 = {                                                                  # case -> (parts, expected LUFS); the tolerance is 0.1 LU
    1: ([(-23.0, 20.0)], -23.0),
    3: ([(-36.0, 10.0), (-23.0, 60.0), (-36.0, 10.0)], -23.0),
    4: ([(-72.0, 10.0), (-36.0, 10.0), (-23.0, 60.0), (-36.0, 10.0), (-72.0, 10.0)], -23.0),
    5: ([(-26.0, 20.0), (-20.0, 20.1), (-26.0, 20.0)], -23.0),
}
TECH_3342 = {                                                                  # case -> (parts, expected LRA); the tolerance is 1 LU
    1: ([(-20.0, 20.0), (-30.0, 20.0)], 10.0),
    2: ([(-20.0, 20.0), (-15.0, 20.0)], 5.0),
    3: ([(-40.0, 20.0), (-20.0, 20.0)], 20.0),
    4: ([(-50.0, 20.0), (-35.0, 20.0), (-20.0, 20.0), (-35.0, 20.0), (-50.0, 20.0)], 15.0),
}
