"""CPU: the float64 restatement of the sparse-tap resampler (tests/_resample_sparse_oracle.py) that the device kernel is checked
against -- its tap formula against _resample_oracle's, its results against the dense oracle's, its geometry for the pairs of rates
only the sparse kernel takes, and the zero-tap argument itself on sampled phases of 8979 : 8000.

On "equal exactly": the sparse sum is the dense sum without its zero terms, so in ONE summation order both are the same float64
number.  _resample_oracle.resample sums with np.einsum, whose order is numpy's business (blocked, SIMD lanes): against it the
ascending chain differs in the last bits (up to 1.8e-15 absolute, 8 ulp, on the standard-normal inputs below -- measured when this
file was written).  So the comparison is made three ways: exactly against the dense taps and frames of _resample_oracle summed in
ascending order; exactly against _resample_oracle.resample itself on inputs for which every order gives the same float64 (at most
one nonzero sample, a power of two, under any window); and against _resample_oracle.resample on standard-normal inputs within the
float64 any-order summation bound (K + 2) * 2^-53 * conv(|taps|, |x|) -- derived like the float32 bound of the device tests."""
import numpy as np
import pytest

from tests import _resample_oracle as ro
from tests import _resample_sparse_oracle as so

EPS64 = 2.0 ** -53
LARGE = {   # (orig, new) -> (o, n, width, K, S), first[0], first[1], first[2], first[n - 1]: worked out from the formula on the CPU
    (8979, 8000): ((8979, 8000, 7, 8993, 16), 1, 2, 3, 8979),
    (7127, 8000): ((7127, 8000, 7, 7141, 16), 1, 2, 3, 7128),
    (11313, 8000): ((11313, 8000, 9, 11331, 20), 1, 2, 4, 11313),
    (8979, 1000): ((8979, 1000, 55, 9089, 112), 1, 10, 19, 8971),
    (1025, 2048): ((1025, 2048, 7, 1039, 16), 1, 2, 2, 1026),
}


def _cases():
    out = sorted(ro.LENGTHS)
    return out + [(a, b, 1000) for a, b in sorted(ro.TABLE) if not any(c[:2] == (a, b) for c in out)]


def _clips(orig, new, L, b=3):
    return np.random.default_rng([orig, new, L]).standard_normal((b, L)).astype(np.float32)


def _dense_chain(x, orig, new, absolute=False):
    """_resample_oracle's float32 taps on _resample_oracle's frames, every output one chain over k = 0 .. K-1 in ascending order;
    absolute: |taps| on |x|."""
    o, n, width, K = ro.geometry(orig, new)
    tp = ro.taps32(orig, new).astype(np.float64)                         # (n, K)
    fr = ro._frames(np.asarray(x, dtype=np.float64), o, n, width, K)     # (B, J, K)
    if absolute:
        tp, fr = np.abs(tp), np.abs(fr)
    y = np.zeros(fr.shape[:2] + (n,))
    for k in range(K):
        y = fr[:, :, k, None] * tp[None, None, :, k] + y
    return y.reshape(x.shape[0], -1)[:, :ro.out_len(orig, new, x.shape[1])]


@pytest.mark.parametrize("pair", sorted(ro.TABLE), ids=str)
def test_the_tap_formula_is_the_dense_oracles(pair):
    o, n, width, K, S = so.geometry(*pair)
    assert (o, n, width, K) == ro.TABLE[pair] and S % 4 == 0 and 2 * width + 1 <= S < 2 * width + 5
    dense = ro.taps64(*pair)
    assert np.array_equal(so.taps64_at(*pair, np.arange(n)[:, None], np.arange(K)[None, :]), dense)
    taps, first = so.taps32(*pair)
    d32 = dense.astype(np.float32)
    scattered = np.zeros((n, K + S), dtype=np.float32)
    for i in range(n):
        scattered[i, first[i]:first[i] + S] = taps[i]
    assert np.array_equal(scattered[:, :K], d32) and not scattered[:, K:].any()      # what the rows leave out is 0.0f


@pytest.mark.parametrize("case", _cases(), ids=str)
def test_sparse_oracle_equals_the_dense_oracle(case):
    orig, new, L = case
    o, n, width, K = ro.geometry(orig, new)
    x = _clips(orig, new, L)
    y, bound = so.resample(x, orig, new)
    want, want_bound = ro.resample(x, orig, new, with_bound=True)
    assert y.shape == want.shape == (3, ro.out_len(orig, new, L))
    assert np.array_equal(y, _dense_chain(x, orig, new))                  # the same order: the same number
    assert np.array_equal(bound, _dense_chain(x, orig, new, absolute=True))
    err = np.abs(y - want)
    print(case, "against np.einsum's order: largest |difference| / bound", float((err / ((K + 2) * EPS64 * want_bound + 1e-300)).max()))
    assert np.all(err <= (K + 2) * EPS64 * want_bound)
    # at most one nonzero sample under any window (K apart), each a power of two: every order of summation gives tap * 2^e exactly
    z = np.zeros((3, L))
    for b in range(3):
        pos = np.arange(b * 7 % max(L, 1), L, K + 1)
        z[b, pos] = 2.0 ** ((pos % 5) - 2) * np.where(pos % 2, -1.0, 1.0)
    got, _ = so.resample(z, orig, new)
    assert np.array_equal(got, ro.resample(z, orig, new))


@pytest.mark.parametrize("pair", sorted(LARGE), ids=str)
def test_support_and_first_of_the_large_pairs(pair):
    geo, f0, f1, f2, flast = LARGE[pair]
    o, n, width, K, S = geo
    assert so.geometry(*pair) == geo and S == (2 * width + 1 + 3) // 4 * 4
    first = so.first(*pair)
    assert first.shape == (n,) and (int(first[0]), int(first[1]), int(first[2]), int(first[-1])) == (f0, f1, f2, flast)
    # from the formula, on whole dense rows of sampled phases: the first k with t > -6, and a run |t| < 6 no longer than 2 * width + 1
    base = min(o, n) * ro.ROLLOFF
    k = np.arange(K, dtype=np.float64)
    for i in sorted(set([0, 1, 2, n // 2, n - 1] + np.random.default_rng([o, n]).integers(0, n, 40).tolist())):
        phase = np.float64(np.float32(-i) / np.float32(n))
        t = (phase + (k - width) / o) * base
        run = np.flatnonzero((t > -6) & (t < 6))
        assert run[0] == first[i] and np.array_equal(run, np.arange(run[0], run[-1] + 1)) and len(run) <= 2 * width + 1 <= S, i
    d = first - np.arange(n) * o // n
    assert d.min() >= 0 and d.max() <= 3                                  # what the kernel's LDS window is sized by


def test_every_dropped_tap_of_sampled_phases_is_zero():
    pair = (8979, 8000)
    o, n, width, K, S = so.geometry(*pair)
    taps, first = so.taps32(*pair)
    assert taps.dtype == np.float32 and taps.shape == (n, S)
    phases = np.unique(np.concatenate([[0, 1, n - 1], np.random.default_rng(8979).integers(0, n, 200)]))
    rows = so.taps64_at(*pair, phases[:, None], np.arange(K)[None, :]).astype(np.float32)      # 200 dense rows, not 8000
    longest = 0
    for r, i in zip(rows, phases):
        lo, hi = int(first[i]), min(int(first[i]) + S, K)
        assert not r[:lo].any() and not r[hi:].any(), i                   # 0.0f, every one
        assert np.array_equal(r[lo:hi], taps[i, :hi - lo]) and not taps[i, hi - lo:].any(), i
        longest = max(longest, int(np.flatnonzero(r)[-1] - np.flatnonzero(r)[0] + 1))
    assert longest == 14
