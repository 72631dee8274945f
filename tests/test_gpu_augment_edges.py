"""GPU: the AugmentFP signal-chain kernels (csrc/augment.hip) at their edges, each called through its C entry point and compared with
a float64 / int64 restatement written here (no oracle import, no golden file).

Why the exact cases are exact
  fir_kernel      samples and taps are integers in [-3, 3] stored as float32.  Every product is an integer of magnitude <= 9 and every
                  partial sum -- the float32 accumulators, whatever the order or the FMA contraction, and the two float64 edge sums
                  times the replicated end samples -- an integer of magnitude <= 9 * 3100 = 27 900 < 2^24 (3100 = the longest filter of
                  the grid), so float32 holds all of them exactly.  _fir_reference() asserts that of the reference before it is used.
  scale_rows      one IEEE float32 multiplication or division per sample: the CPU's is the same operation.
  gather          a slice of +-2^k has sum of squares L * 4^k (L <= 3001 < 2^24: exact in any order), mean 4^k, root 2^k, and
                  2^k + 1e-8f rounds back to 2^k for k >= -1 (half an ulp of 0.5 is 3e-8); the row of +-1 has RMS 1.  The output is the
                  sign pattern.
  mix, noise NULL one IEEE division by the row's peak.
  clip_kernel     order statistics and torch.quantile's own float32 rank and lerp arithmetic (the existing tests' assertion).

Which launch geometry each size selects
  fir_kernel      1024 outputs per workgroup: T = 1, 3, 1023 and 1024 are one tile (masked stores), 1025 is a second tile with one
                  output, 2050 a third with two; in the impulse-response mode Tout = T + 3099 adds up to three tiles that only feed
                  `peak`.  512 taps per LDS chunk: n = 511 and 512 are one chunk, 513 one tap of a second, 1029 three, 3100 seven.
                  n = 3100 > T + 1023 leaves taps outside [klo, khi) on BOTH sides of one workgroup (both edge sums), off = 0 puts
                  every tap after the signal start, off = n + 7 reads 8 samples before it even with the first tap.
  scale_rows      the grid is capped at 256 blocks x 256 threads: T = 65536 + 300 makes the first 300 threads stride once.
  gather / mix    one 1024-thread workgroup per row: T = 5, 7, 1000, 1023 leave threads idle, 1024 is one pass, 1025 .. 5000 stride.
  clip_kernel     one workgroup per row; the flat form walks every selected row, and 9 000 000 pooled samples is past 2^23, where the
                  float32 rank q * (n - 1) has no fractional bit left.
Every device tensor stays referenced until after the synchronise (or the .cpu() copy) that follows the call using it."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64
FAR = 1 << 40                                   # a `src` offset (in floats) that must never be dereferenced


def _lib():
    from musicfpaugment_amd._lib import check, lib, ptr, stream
    return check, lib(), ptr, stream


def _guarded(shape, dtype=torch.float32):
    """A NaN-filled buffer and the view of `shape` in its middle."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _guards_intact(buf):
    b = buf.cpu()
    return bool(torch.isnan(b[:GUARD]).all()) and bool(torch.isnan(b[-GUARD:]).all())


def _dev(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=dtype).cuda()


# ----------------------------------------------------------------------------------------------------------------- A.1 / A.2: fir_kernel
FIR_T = (1, 3, 1023, 1024, 1025, 2050)
FIR_N = (1, 2, 5, 511, 512, 513, 1029, 3100)
FIR_MODES = [(0, 0), (0, 1), (1, 0), (1, 2)]                  # (pad_mode, out_mode)


def _fir_rows():
    """(ntaps, off) of every row of one launch: the whole n x off grid."""
    return [(n, off) for n in FIR_N for off in (0, n // 2, n - 1, n + 7)]


def _fir_one(x, taps, off, pad_mode, Tout):
    """y[t] = sum_k taps[k] * xpad[t + k - off], t < Tout: the plain correlation over the padded signal, float64."""
    T, n = len(x), len(taps)
    s = np.arange(Tout + n - 1) - off                                  # sample index behind xpad[j]
    if pad_mode == 0:
        xpad = x[np.clip(s, 0, T - 1)]
    else:
        xpad = np.where((s >= 0) & (s < T), x[np.clip(s, 0, T - 1)], 0.0)
    return np.correlate(xpad.astype(np.float64), taps.astype(np.float64), mode="valid")


def _fir_problem(seed, T, rows):
    g = np.random.default_rng(seed)
    x = g.integers(-3, 4, size=(len(rows), T)).astype(np.float64)
    taps = [g.integers(-3, 4, size=n).astype(np.float64) for n, _ in rows]
    return x, taps


def _fir_reference(x, taps, rows, pad_mode, Tout):
    """Full-length (Tout) float64 outputs of every row; checks that the reference itself is exact."""
    ys = np.stack([_fir_one(x[b], taps[b], rows[b][1], pad_mode, Tout) for b in range(len(rows))])
    assert ys.dtype == np.float64 and np.array_equal(ys, np.round(ys))
    assert float(np.abs(ys).max()) < 2 ** 24 and 9 * max(n for n, _ in rows) < 2 ** 24        # the peak is one of these values
    return ys


@functools.lru_cache(maxsize=None)
def _fir_grid_case(T, pad_mode, full):
    rows = _fir_rows()
    Tout = T + max(FIR_N) - 1 if full else T
    x, taps = _fir_problem(1000 + T, T, rows)
    return rows, x, taps, Tout, _fir_reference(x, taps, rows, pad_mode, Tout)


def _fir_launch(x, taps, rows, gate, pad_mode, out_mode, Tout):
    """One mfpa_fir launch over ragged rows.  Returns (y, peak or None, guards intact)."""
    check, L, ptr, stream = _lib()
    B, T = x.shape
    nt = [n for n, _ in rows]
    xd = _dev(x, torch.float32)
    td = _dev(np.concatenate(taps), torch.float32)
    toff = _dev(np.concatenate([[0], np.cumsum(nt)[:-1]]), torch.int64)
    nd, od = _dev(nt, torch.int32), _dev([o for _, o in rows], torch.int32)
    gd = _dev(gate, torch.uint8)
    ybuf, y = _guarded((B, T))
    pbuf = torch.full((B + 2,), float("nan"), device="cuda")           # 1-element guards around `peak`
    peak = pbuf[1:B + 1]
    assert peak.data_ptr() == pbuf.data_ptr() + 4
    check(L.mfpa_fir(ptr(xd), B, T, Tout, ptr(td), ptr(toff), ptr(nd), ptr(od), ptr(gd), pad_mode, out_mode, ptr(y),
                     peak.data_ptr() if out_mode == 2 else 0, stream()), "fir")
    torch.cuda.synchronize()
    got, pk = y.cpu().numpy(), pbuf.cpu().numpy()
    ok = _guards_intact(ybuf) and bool(np.isnan(pk[0]) and np.isnan(pk[-1]))
    if out_mode != 2:
        ok = ok and bool(np.isnan(pk).all())                           # `peak` is not touched outside the impulse-response mode
    del xd, td, toff, nd, od, gd
    return got, (pk[1:-1] if out_mode == 2 else None), ok


@pytest.mark.parametrize("pad_mode,out_mode", FIR_MODES, ids=["replicate-lowpass", "replicate-highpass", "zero-lowpass", "zero-ir"])
def test_fir_exact_on_small_integers(pad_mode, out_mode):
    for T in FIR_T:
        rows, x, taps, Tout, ref = _fir_grid_case(T, pad_mode, out_mode == 2)
        got, peak, intact = _fir_launch(x, taps, rows, np.ones(len(rows), np.uint8), pad_mode, out_mode, Tout)
        want = x - ref[:, :T] if out_mode == 1 else ref[:, :T]
        bad = np.argwhere(got != want)
        assert np.array_equal(got, want.astype(np.float32)), (T, len(bad), [(rows[b], int(t)) for b, t in bad[:4]])
        if out_mode == 2:
            np.testing.assert_array_equal(peak, np.abs(ref).max(axis=1).astype(np.float32), err_msg=f"peak, T={T}")
        assert intact, T


@pytest.mark.parametrize("pad_mode,out_mode", FIR_MODES, ids=["replicate-lowpass", "replicate-highpass", "zero-lowpass", "zero-ir"])
def test_fir_one_ragged_launch(pad_mode, out_mode):
    T = 1025
    rows = [(5, 0), (513, 256), (1029, 1028), (2, 9), (3100, 1550), (512, 511)]
    gate = np.array([1, 0, 1, 0, 1, 1], np.uint8)
    Tout = T + max(n for n, _ in rows) - 1 if out_mode == 2 else T
    x, taps = _fir_problem(77, T, rows)
    ref = _fir_reference(x, taps, rows, pad_mode, Tout)
    got, peak, intact = _fir_launch(x, taps, rows, gate, pad_mode, out_mode, Tout)
    for b in range(len(rows)):
        if not gate[b]:
            np.testing.assert_array_equal(got[b], x[b].astype(np.float32), err_msg=f"gated-off row {b}")
            if out_mode == 2:
                assert peak[b] == 0.0, (b, peak[b])
        else:
            want = x[b] - ref[b, :T] if out_mode == 1 else ref[b, :T]
            np.testing.assert_array_equal(got[b], want.astype(np.float32), err_msg=f"row {b} {rows[b]}")
            if out_mode == 2:
                assert peak[b] == np.abs(ref[b]).max(), (b, peak[b])
    assert intact


# ----------------------------------------------------------------------------------------------------------------- A.3: lowpass_taps_kernel
def test_lowpass_taps_at_their_ends():
    """taps[k] = 2c hann(k) sinc(2c pi (k - half)), k <= 2 half, normalised to unit sum (the kernel's comment), in float64."""
    check, L, ptr, stream = _lib()
    cases = [(0.5, 8),            # the shortest filter the host asks for: sin(pi t) is rounding noise, the taps are a unit impulse
             (0.25, 1),           # the three taps of a gated-off row: hann = (0, 1, 0)
             (0.03125, 128),      # n = 257 = 256 + 1: one thread takes a second tap
             (0.015625, 256)]     # n = 513 = 2 * 256 + 1
    half = [h for _, h in cases]
    nt = [2 * h + 1 for h in half]
    toff = np.concatenate([[0], np.cumsum(nt)[:-1]])
    cd, hd, td = _dev([c for c, _ in cases], torch.float32), _dev(half, torch.int32), _dev(toff, torch.int64)
    buf, taps = _guarded((sum(nt),))
    check(L.mfpa_lowpass_taps(ptr(cd), ptr(hd), ptr(td), len(cases), ptr(taps), stream()), "taps")
    torch.cuda.synchronize()
    got = taps.cpu().numpy()
    assert _guards_intact(buf)
    for (c, h), n, o in zip(cases, nt, toff):
        k = np.arange(n, dtype=np.float64)
        arg = 2 * c * np.pi * (k - h)
        sinc = np.where(k == h, 1.0, np.sin(arg) / np.where(k == h, 1.0, arg))
        want = 2 * c * (0.5 - 0.5 * np.cos(2 * np.pi * k / (n - 1))) * sinc
        want = want / want.sum()
        np.testing.assert_allclose(got[o:o + n], want, rtol=0, atol=2e-7, err_msg=f"cutoff {c} half {h}")
        assert abs(got[o:o + n].astype(np.float64).sum() - 1.0) <= n * 2.0 ** -24, (c, h)


# ----------------------------------------------------------------------------------------------------------------- A.4: scale_rows_kernel
def _scale(x, f, gate, invert, in_place=False):
    check, L, ptr, stream = _lib()
    B, T = x.shape
    xd, fd = x.cuda(), f.cuda()
    gd = None if gate is None else gate.cuda()
    ybuf, y = _guarded((B, T))
    if in_place:
        y.copy_(xd)
    check(L.mfpa_scale_rows(ptr(y) if in_place else ptr(xd), B, T, ptr(fd), ptr(gd), invert, ptr(y), stream()), "scale")
    torch.cuda.synchronize()
    got = y.cpu()
    assert _guards_intact(ybuf)
    del xd, fd, gd
    return got


@pytest.mark.parametrize("T", [65536 + 300, 1])
def test_scale_rows_past_the_grid_cap(T):
    g = torch.Generator().manual_seed(T)
    B = 4
    x = torch.randn(B, T, generator=g)
    f = torch.rand(B, generator=g) * 3 + 0.25
    gate = torch.tensor([1, 0, 0, 1], dtype=torch.uint8)
    for invert in (0, 1):
        full = x / f[:, None] if invert else x * f[:, None]                # float32 on the CPU: the same single rounding
        assert full.dtype == torch.float32
        assert torch.equal(_scale(x, f, None, invert), full), invert       # apply == NULL scales every row
        mixed = torch.where(gate[:, None] != 0, full, x)
        for in_place in (False, True):                                     # in place is how the chain divides by the peak
            got = _scale(x, f, gate, invert, in_place)
            assert torch.equal(got, mixed), (invert, in_place, int((got != mixed).sum()))
            assert torch.equal(got[1].view(torch.int32), x[1].view(torch.int32))   # gated off: bit-identical
            assert torch.equal(got[2].view(torch.int32), x[2].view(torch.int32))
        assert torch.equal(_scale(x, f, None, invert, True), full), invert


# ----------------------------------------------------------------------------------------------------------------- A.5: gather_background_kernel
def _gather(bank, src, ln, T):
    check, L, ptr, stream = _lib()
    B, P = src.shape
    bd, sd, ld = _dev(bank, torch.float32), _dev(src, torch.int64), _dev(ln, torch.int32)
    obuf, out = _guarded((B, T))
    check(L.mfpa_gather_background(ptr(bd), ptr(sd), ptr(ld), B, P, T, ptr(out), stream()), "gather")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert _guards_intact(obuf)
    del bd, sd, ld
    return got


def _gather_rows(T):
    """Rows as lists of (region, offset within the region, length); the bank has three regions of T samples."""
    a = max(1, T // 3)
    rows = [[(1, 0, T)],                                                    # one slice of length T
            [(0, 1, a), (2, T - 1, 1), (1, 2, T - a - 1)],                  # three slices, one of length 1
            [(2, 0, T - a), (0, 0, a)]]                                     # fewer slices than P
    assert all(sum(n for _, _, n in r) == T and all(n >= 1 and o + n <= T for _, o, n in r) for r in rows)
    return rows


def _gather_tables(rows, T, P=3):
    src = np.full((len(rows), P), FAR, dtype=np.int64)                       # unused entries must not be read
    ln = np.zeros((len(rows), P), dtype=np.int32)
    for b, r in enumerate(rows):
        for p, (reg, o, n) in enumerate(r):
            src[b, p], ln[b, p] = reg * T + o, n
    return src, ln


@pytest.mark.parametrize("T", [5, 1000, 1024, 3001])
def test_gather_background_places_slices_bit_for_bit(T):
    g = np.random.default_rng(T)
    sign = g.choice([-1.0, 1.0], size=(3, T))
    bank = sign * np.array([0.5, 1.0, 8.0])[:, None]                         # +-2^k, one k in {-1, 0, 3} per region
    rows = _gather_rows(T)
    src, ln = _gather_tables(rows, T)
    got = _gather(bank.reshape(-1), src, ln, T)
    want = np.stack([np.concatenate([sign[reg, o:o + n] for reg, o, n in r]) for r in rows])
    assert set(np.unique(want)) <= {-1.0, 1.0}
    np.testing.assert_array_equal(got, want.astype(np.float32))


@pytest.mark.parametrize("T", [5, 1000, 1024, 3001])
def test_gather_background_arithmetic(T):
    """Each slice / (rms + 1e-8), then the whole row again (utils.py:190-205 twice), in float64."""
    g = np.random.default_rng(100 + T)
    bank = (g.standard_normal((3, T)) * np.array([0.02, 1.0, 37.0])[:, None]).astype(np.float32)
    rows = _gather_rows(T)
    src, ln = _gather_tables(rows, T)
    got = _gather(bank.reshape(-1), src, ln, T)
    norm = lambda v: v / (np.sqrt(np.mean(v * v)) + 1e-8)
    b64 = bank.astype(np.float64)
    want = np.stack([norm(np.concatenate([norm(b64[reg, o:o + n]) for reg, o, n in r])) for r in rows])
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-6)


# ----------------------------------------------------------------------------------------------------------------- A.6: mix_kernel
def _mix(x, noise, snr, gate):
    check, L, ptr, stream = _lib()
    B, T = x.shape
    xd = x.cuda()
    nd = None if noise is None else noise.cuda()
    sd = None if snr is None else snr.cuda()
    gd = None if gate is None else gate.cuda()
    ybuf, y = _guarded((B, T))
    check(L.mfpa_mix_background(ptr(xd), B, T, ptr(nd), ptr(sd), ptr(gd), ptr(y), stream()), "mix")
    torch.cuda.synchronize()
    got = y.cpu()
    assert _guards_intact(ybuf)
    del xd, nd, sd, gd
    return got


@pytest.mark.parametrize("T", [1, 7, 1023, 1025, 5000])
def test_mix_background_against_float64(T):
    """y = x + rms(x) / 10^(snr/20) * noise; y /= max|y| -- an absolute bound on a unit-peak signal."""
    g = torch.Generator().manual_seed(T)
    snr = torch.tensor([-5.0, 0.0, 30.0, -5.0, 0.0, 30.0])
    B = len(snr)
    x = torch.randn(B, T, generator=g) * 0.3
    noise = torch.randn(B, T, generator=g)
    xd, nd = x.double(), noise.double()
    y = xd + xd.square().mean(dim=1, keepdim=True).sqrt() / 10 ** (snr.double()[:, None] / 20) * nd
    want = y / y.abs().amax(dim=1, keepdim=True)
    got = _mix(x, noise, snr, None)                                          # apply == NULL with a noise row: every row is mixed
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=2e-6)
    gate = torch.tensor([1, 0, 1, 0, 0, 1], dtype=torch.uint8)
    got = _mix(x, noise, snr, gate)
    on = gate != 0
    np.testing.assert_allclose(got[on].numpy(), want[on].numpy(), rtol=0, atol=2e-6)
    assert torch.equal(got[~on], x[~on])                                     # gated off: copied through


@pytest.mark.parametrize("T", [1, 7, 1023, 1025, 5000])
def test_peak_normalisation_form(T):
    g = torch.Generator().manual_seed(50 + T)
    x = torch.randn(3, T, generator=g) * torch.tensor([0.3, 0.0, 40.0])[:, None]
    x[1] = 0.0                                                                # a silent row comes back unchanged
    want = x.clone()
    for b in (0, 2):
        want[b] = x[b] / x[b].abs().max()                                     # float32: the same single division
    assert torch.equal(_mix(x, None, None, None), want)
    got = _mix(x, None, None, torch.tensor([0, 1, 1], dtype=torch.uint8))
    assert torch.equal(got[0], x[0]) and torch.equal(got[1:], want[1:])


# ----------------------------------------------------------------------------------------------------------------- A.7: clip_kernel
def _clip(x, pct, gate, flat):
    check, L, ptr, stream = _lib()
    B, T = x.shape
    xd, pd, gd = x.cuda(), pct.cuda(), gate.cuda()
    ybuf, y = _guarded((B, T))
    if flat:
        check(L.mfpa_clip_quantile_flat(ptr(xd), B, T, ptr(pd), ptr(gd), int(gate.sum()), ptr(y), stream()), "clip_flat")
    else:
        check(L.mfpa_clip_quantile(ptr(xd), B, T, ptr(pd), ptr(gd), ptr(y), stream()), "clip")
    torch.cuda.synchronize()
    got = y.cpu()
    assert _guards_intact(ybuf)
    del xd, pd, gd
    return got


def _clip_rows(x, pct):
    """clipping.py:67-100 one example at a time: clamp to torch.quantile(x, p/2) and torch.quantile(x, 1 - p/2)."""
    return torch.stack([torch.clip(x[b], min=torch.quantile(x[b], pct[b] / 2), max=torch.quantile(x[b], 1 - pct[b] / 2))
                        for b in range(x.shape[0])])


def _clip_flat(x, pct, gate):
    """The same as batch_augment runs it: torch.quantile has no dim argument there, so a selected row is clamped to the quantiles
    of all selected rows flattened together; the others are copied through."""
    sel = torch.nonzero(gate).flatten()
    flat = x[sel].reshape(-1)
    lo, hi = torch.quantile(flat, torch.cat([pct[sel] / 2, 1 - pct[sel] / 2])).chunk(2)      # one sort serves both ends
    want = x.clone()
    want[sel] = torch.clip(x[sel], min=lo[:, None], max=hi[:, None])
    return want


@pytest.mark.parametrize("T", [2, 1000])
def test_clip_per_example_edges(T):
    g = torch.Generator().manual_seed(T)
    x = torch.randn(5, T, generator=g)
    x[2] = -x[2].abs() - 0.5                                                  # an all-negative row
    x[3] = 0.37                                                               # one repeated value
    x[4, : T // 2] = 0.0                                                      # +0.0 and -0.0 both present
    x[4, T // 2: T // 2 + max(1, T // 4)] = -0.0
    pct = torch.tensor([0.0, 1.0, 0.01, 0.3, 0.5])
    want = _clip_rows(x, pct)
    assert torch.equal(want[0], x[0])                                         # pct = 0 returns the input
    assert bool((want[1] == torch.quantile(x[1], 0.5)).all())                 # pct = 1: a constant row at the median
    got = _clip(x, pct, torch.ones(5, dtype=torch.uint8), False)
    np.testing.assert_array_equal(got.numpy(), want.numpy())                  # `==`: does not see the sign of a zero


@pytest.mark.parametrize("T", [2, 1000])
def test_clip_flat_gated_rows_and_ties(T):
    g = torch.Generator().manual_seed(10 + T)
    x = torch.randn(5, T, generator=g)
    x[2, : T // 2] = x[0, 0]                                                  # ties across the selected rows
    x[3, T // 2:] = x[0, 0]
    x[1] *= 100.0                                                             # gated-off rows must stay out of the pool
    x[4] *= 100.0
    gate = torch.tensor([1, 0, 1, 1, 0], dtype=torch.uint8)
    for pct in (torch.tensor([0.003, 0.9, 0.5, 0.01, 0.9]), torch.tensor([0.0, 0.9, 1.0, 0.2, 0.9])):
        got = _clip(x, pct, gate, True)
        np.testing.assert_array_equal(got.numpy(), _clip_flat(x, pct, gate).numpy())
        assert torch.equal(got[1], x[1]) and torch.equal(got[4], x[4])


def test_clip_flat_past_2_to_the_23_pooled_samples():
    """9 000 000 pooled samples: the float32 rank q * (n - 1) has no fractional bit left; torch.quantile rounds the same way."""
    T = 3_000_000
    g = torch.Generator().manual_seed(9)
    x = torch.randn(3, T, generator=g)
    pct = torch.tensor([0.003, 0.0077, 0.5])
    gate = torch.ones(3, dtype=torch.uint8)
    assert 3 * T > 2 ** 23
    got = _clip(x, pct, gate, True)
    want = _clip_flat(x, pct, gate)
    assert bool((want != x).any(dim=1).all())                                 # every row is really clamped
    assert torch.equal(got, want), [int((got[b] != want[b]).sum()) for b in range(3)]
