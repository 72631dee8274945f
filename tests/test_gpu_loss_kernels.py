"""GPU: the kernels around the DFT GEMM of the spectral loss (csrc/loss.hip) -- reflect_pad, reflect_pad_adjoint, frames_adjoint,
dft_mag, stft_loss_partial / finish and stft_loss_grad -- each called through its C entry point and compared, element by element, with
a float64 restatement written here (no oracle import, no golden file).

Why the exact cases are exact
  reflect_pad           a copy (and a zero fill).
  reflect_pad_adjoint   upstream values are integers in [-3, 3]; an output adds at most three of them (both reflections land on one
                        sample when pad = T - 1) and, accumulating, one more integer: |sum| <= 12.
  frames_adjoint        integers in [-3, 3]; an output adds at most ceil(win / hop) <= 16 of them ((16, 1)): |sum| <= 48.
  adjoint identities    both sides are sums of at most 2024 * 16 products of such integers: |sum| < 2^24 even in float32, and they are
                        formed in int64 on the CPU from the device outputs.
  loss sums, cx == cy   every per-element difference is x - x = 0.
  All far below 2^24, so float32 holds every partial sum whatever the order; each reference asserts that of itself before it is used.

Which launch geometry each size selects
  reflect_pad, frames_adjoint, reflect_pad_adjoint   256 threads a block, the grid capped at 1024 blocks: a row of 1024 * 256 + 300
                        elements makes the first 300 threads stride once; the other sizes are below one block (2, 9, 100) or a few.
  dft_mag, stft_loss_grad   capped at 8192 blocks of 256: rows * bins = 8200 * 257 > 8192 * 256 strides.
  stft_loss_partial     (rows * bins) / 2048 blocks capped at 1024: 37 rows are 5 blocks of four to five passes, 8200 rows are the cap.
Every device tensor stays referenced until after the synchronise that follows the call using it."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GUARD = 64
BIG = 1024 * 256 + 300
BINS, IM_OFF, LDC = 257, 264, 528                      # the zero gap _dft_matrix leaves between the two halves, here NaN


def _lib():
    from musicfpaugment_amd._lib import check, lib, ptr, stream
    return check, lib(), ptr, stream


def _guarded(shape, fill=float("nan"), dtype=torch.float32):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device="cuda")
    view = buf[GUARD:GUARD + n].view(*shape)
    view.fill_(fill)
    return buf, view


def _guards_intact(buf):
    b = buf.cpu()
    return bool(torch.isnan(b[:GUARD]).all()) and bool(torch.isnan(b[-GUARD:]).all())


def _ints(g, *shape):
    return torch.randint(-3, 4, shape, generator=g).double()


def _exact(t, bound=2 ** 24):
    assert t.dtype == torch.float64 and torch.equal(t, t.round()) and float(t.abs().max()) < bound
    return t


# ----------------------------------------------------------------------------------------------------------------- device calls
def _reflect_pad(x, pad, shift, Lout):
    check, L, ptr, stream = _lib()
    B, T = x.shape
    xd = x.float().cuda()
    obuf, out = _guarded((B, Lout))
    check(L.mfpa_reflect_pad(ptr(xd), B, T, pad, shift, Lout, ptr(out), stream()), "reflect_pad")
    torch.cuda.synchronize()
    got = out.cpu()
    assert _guards_intact(obuf)
    del xd
    return got


def _reflect_pad_adjoint(u, T, pad, accumulate, prefill):
    """u (B, L) upstream; prefill (B, T) or None (NaN: the kernel must overwrite without reading)."""
    check, L, ptr, stream = _lib()
    B, Lp = u.shape
    ud = u.float().cuda()
    obuf, dx = _guarded((B, T))
    if prefill is not None:
        dx.copy_(prefill.float())
    check(L.mfpa_reflect_pad_adjoint(ptr(ud), B, T, pad, Lp, accumulate, ptr(dx), stream()), "reflect_pad_adjoint")
    torch.cuda.synchronize()
    got = dx.cpu()
    assert _guards_intact(obuf)
    del ud
    return got


def _frames_adjoint(df, win, hop, off, Lp):
    """df (B, frames, ldf) with ldf >= win."""
    check, L, ptr, stream = _lib()
    B, frames, ldf = df.shape
    dd = df.float().contiguous().cuda()
    obuf, out = _guarded((B, Lp))
    check(L.mfpa_frames_adjoint(ptr(dd), B, frames, ldf, win, hop, off, Lp, ptr(out), stream()), "frames_adjoint")
    torch.cuda.synchronize()
    got = out.cpu()
    assert _guards_intact(obuf)
    del dd
    return got


# ----------------------------------------------------------------------------------------------------------------- B.1: reflect_pad_kernel
TP = [(2, 1), (9, 8), (100, 0), (1000, 512)]            # (T, pad): pad = T - 1 twice, pad = 0 once


def _reflect_pad_reference(x, pad, shift, Lout):
    full = F.pad(x[:, None], (pad, pad), mode="reflect")[:, 0] if pad else x
    full = full[:, shift:]
    out = torch.zeros(x.shape[0], Lout, dtype=x.dtype)
    n = min(Lout, full.shape[1])
    out[:, :n] = full[:, :n]
    return out


@pytest.mark.parametrize("T,pad", TP + [(BIG - 2 * 512, 512)])
def test_reflect_pad_is_the_shifted_copy(T, pad):
    g = torch.Generator().manual_seed(T + pad)
    x = torch.randn(3, T, generator=g)
    full = T + 2 * pad
    for shift in (0, 2, 3):
        for Lout in ([full] if full == BIG else [max(1, full // 2), full, full + 37]):
            want = _reflect_pad_reference(x, pad, shift, Lout)
            got = _reflect_pad(x, pad, shift, Lout)
            assert torch.equal(got, want), (shift, Lout, int((got != want).sum()))
            tail = got[:, max(0, full - shift):]
            assert torch.equal(tail, torch.zeros_like(tail))                 # past the padded signal: exactly 0.0


# ----------------------------------------------------------------------------------------------------------------- B.2: reflect_pad_adjoint_kernel
def _reflect_pad_adjoint_reference(u, T, pad):
    """float64 autograd through F.pad(mode="reflect"); u (B, >= T + 2 pad), the surplus is not part of the padded signal."""
    x = torch.zeros(u.shape[0], T, dtype=torch.float64, requires_grad=True)
    xp = F.pad(x[:, None], (pad, pad), mode="reflect")[:, 0] if pad else x * 1.0
    xp.backward(u[:, :T + 2 * pad])
    return _exact(x.grad, 16)


@pytest.mark.parametrize("T,pad", TP + [(BIG, 512)])
def test_reflect_pad_adjoint_exact_on_small_integers(T, pad):
    g = torch.Generator().manual_seed(7 * T + pad)
    B = 2
    for surplus in (0, 29):
        u = _ints(g, B, T + 2 * pad)
        ref = _reflect_pad_adjoint_reference(u, T, pad)
        if surplus:                                                          # L larger than the padded signal: the rest must not be read
            u = torch.cat([u, torch.full((B, surplus), float("nan"), dtype=torch.float64)], dim=1)
        got = _reflect_pad_adjoint(u, T, pad, 0, None)                       # dx starts as NaN
        assert torch.equal(got.double(), ref), ("overwrite", surplus, int((got.double() != ref).sum()))
        pre = _ints(g, B, T)
        got = _reflect_pad_adjoint(u, T, pad, 1, pre)
        assert torch.equal(got.double(), _exact(ref + pre, 16)), ("accumulate", surplus)


# ----------------------------------------------------------------------------------------------------------------- B.3: frames_adjoint_kernel
WH = [(600, 120), (240, 50), (7, 7), (5, 9), (16, 1)]   # overlap 5, ragged 4.8, touching, gaps (must read 0), hop 1


def _frames_adjoint_reference(df, win, hop, off, Lp):
    """dxp[b, off + t*hop + j] += df[b, t, j] for indices below Lp."""
    B, frames, _ = df.shape
    out = torch.zeros(B, Lp, dtype=torch.float64)
    for t in range(frames):
        lo = off + t * hop
        n = min(win, Lp - lo)
        if n > 0:
            out[:, lo:lo + n] += df[:, t, :n]
    return _exact(out, 64)


@pytest.mark.parametrize("win,hop", WH)
def test_frames_adjoint_exact_on_small_integers(win, hop):
    g = torch.Generator().manual_seed(win * 31 + hop)
    B = 2
    for frames in (1, 2, 41):
        for off in (0, 3, 212):
            end = off + (frames - 1) * hop + win
            for pad_cols in (0, 13):
                df = _ints(g, B, frames, win)
                dfp = df if not pad_cols else torch.cat([df, torch.full((B, frames, pad_cols), float("nan"), dtype=torch.float64)], dim=2)
                for Lp in (end + 19, end, max(1, end - win // 2 - 1)):       # a zero tail; exactly the end; a truncated overlap-add
                    ref = _frames_adjoint_reference(df, win, hop, off, Lp)
                    got = _frames_adjoint(dfp, win, hop, off, Lp)
                    assert bool(torch.isfinite(got).all()), (frames, off, pad_cols, Lp)
                    assert torch.equal(got.double(), ref), (frames, off, pad_cols, Lp, int((got.double() != ref).sum()))


def test_frames_adjoint_row_past_the_grid_cap():
    g = torch.Generator().manual_seed(5)
    win, hop, off = 600, 120, 212
    frames = (BIG - off - win) // hop + 3                                    # the last frames reach past L: truncated
    df = _ints(g, 1, frames, win)
    ref = _frames_adjoint_reference(df, win, hop, off, BIG)
    got = _frames_adjoint(df, win, hop, off, BIG)
    assert torch.equal(got.double(), ref)


# ----------------------------------------------------------------------------------------------------------------- B.4: adjoint identities
@pytest.mark.parametrize("T,pad,win,hop,off", [(1000, 512, 600, 120, 212), (9, 8, 7, 7, 3), (100, 0, 16, 1, 0), (2, 1, 5, 9, 0)])
def test_forward_and_adjoint_kernels_are_adjoint(T, pad, win, hop, off):
    """<reflect_pad(x), u> = <x, reflect_pad_adjoint(u)> and <frames(xp), df> = <xp, frames_adjoint(df)> on integers: the one test that
    ties the forward and backward kernels to each other.  Left sides from the device's reflect_pad and a CPU framing of it."""
    g = torch.Generator().manual_seed(T + win)
    B, Lp = 2, T + 2 * pad
    frames = 1 + T // hop                                                    # torch.stft's count; the last frame may reach past Lp
    i64 = lambda t: _exact(t.double()).long()
    x, u, df = _ints(g, B, T), _ints(g, B, Lp), _ints(g, B, frames, win)
    xp = _reflect_pad(x, pad, 0, Lp)
    lhs = int((i64(xp) * i64(u)).sum())
    rhs = int((i64(x) * i64(_reflect_pad_adjoint(u, T, pad, 0, None))).sum())
    assert lhs == rhs and abs(lhs) < 2 ** 24
    fr = torch.zeros(B, frames, win, dtype=torch.int64)                      # frames(xp)[t, j] = xp[off + t*hop + j], 0 past the end
    for t in range(frames):
        n = min(win, Lp - off - t * hop)
        if n > 0:
            fr[:, t, :n] = i64(xp)[:, off + t * hop: off + t * hop + n]
    dxp = _frames_adjoint(df, win, hop, off, Lp)
    lhs = int((fr * i64(df)).sum())
    rhs = int((i64(xp) * i64(dxp)).sum())
    assert lhs == rhs and abs(lhs) < 2 ** 24
    # ... and the chain: <frames(reflect_pad(x)), df> = <x, reflect_pad_adjoint(frames_adjoint(df))>
    assert lhs == int((i64(x) * i64(_reflect_pad_adjoint(dxp.double(), T, pad, 0, None))).sum())


# ----------------------------------------------------------------------------------------------------------------- B.5 / B.6: magnitudes, sums, gradient
CLAMP = 1e-7


def _layout(re, im):
    """(rows, LDC) float32: re at [:BINS], im at [IM_OFF:IM_OFF + BINS], NaN everywhere else."""
    c = torch.full((re.shape[0], LDC), float("nan"), dtype=torch.float32)
    c[:, :BINS], c[:, IM_OFF:IM_OFF + BINS] = re, im
    return c


def _only_owned_columns_written(c):
    return bool(torch.isnan(c[:, BINS:IM_OFF]).all()) and bool(torch.isnan(c[:, IM_OFF + BINS:]).all())


@functools.lru_cache(maxsize=None)
def _spectra(rows):
    """x and y as float32 (re, im) pairs whose re^2 + im^2 is exactly 0, about 2e-8 (re = im = 1e-4) or at least 1e-6 -- float32 and
    float64 cannot disagree about the 1e-7 clamp -- a tenth of the elements in each of the first two classes.  Where x is above the
    clamp (|x| >= 1e-2), |y| is either clamped (3e-4) or f |x| with f in [0.3, 0.8] or [1.25, 3]: | |y| - |x| | >= 0.2 |y|, so the
    sign of the log term is robust and both terms of the gradient have the same sign (no cancellation).  Planted: x == y above the
    clamp at [0, 3] and [rows - 1, 200]; x tiny with y large at [0, 5]; x zero with y large at [0, 6]."""
    g = torch.Generator().manual_seed(rows)
    shape = (rows, BINS)
    u = lambda: torch.rand(shape, generator=g, dtype=torch.float64)
    cls_x, cls_y = u(), u()
    mag_x = 10 ** (u() * 3 - 2)                                              # [1e-2, 10]
    f = torch.where(u() < 0.5, 0.3 + 0.5 * u(), 1.25 + 1.75 * u())
    mag_y = mag_x * f
    ph_x, ph_y = u() * 2 * np.pi, u() * 2 * np.pi
    xr, xi = mag_x * torch.cos(ph_x), mag_x * torch.sin(ph_x)
    yr, yi = mag_y * torch.cos(ph_y), mag_y * torch.sin(ph_y)
    big_y = 10 ** (u() * 3 - 2)                                              # where x is clamped, a large y is free
    yr = torch.where(cls_x < 0.2, big_y * torch.cos(ph_y), yr)
    yi = torch.where(cls_x < 0.2, big_y * torch.sin(ph_y), yi)
    for cls, (r, i) in ((cls_x, (xr, xi)), (cls_y, (yr, yi))):
        r[cls < 0.1], i[cls < 0.1] = 0.0, 0.0
        tiny = (cls >= 0.1) & (cls < 0.2)
        r[tiny], i[tiny] = 1e-4, 1e-4
    xr, xi, yr, yi = (t.float() for t in (xr, xi, yr, yi))
    xr[0, 5], xi[0, 5], yr[0, 5], yi[0, 5] = 1e-4, 1e-4, 0.3, -0.4
    xr[0, 6], xi[0, 6], yr[0, 6], yi[0, 6] = 0.0, 0.0, 0.3, -0.4
    for r, k in ((0, 3), (rows - 1, 200)):
        xr[r, k], xi[r, k] = 0.6, -0.8
        yr[r, k], yi[r, k] = xr[r, k], xi[r, k]
    for r, i in ((xr, xi), (yr, yi)):                                        # the three classes, decided in float64 from the float32 values
        p = r.double() ** 2 + i.double() ** 2
        assert bool(((p == 0) | ((p > 1.9e-8) & (p < 2.1e-8)) | (p >= 1e-6)).all())
    return xr, xi, yr, yi


def _mag64(re, im):
    return torch.sqrt(torch.clamp(re.double() ** 2 + im.double() ** 2, min=CLAMP))


def _mag32(re, im):
    return torch.sqrt(torch.clamp(re * re + im * im, min=torch.tensor(CLAMP, dtype=torch.float32)))


def _device_sums(cxd, cyd, rows):
    check, L, ptr, stream = _lib()
    out3 = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
    work = torch.empty(3 * L.mfpa_loss_blocks(), dtype=torch.float64, device="cuda")
    check(L.mfpa_stft_loss_sums(ptr(cxd), ptr(cyd), rows, BINS, LDC, IM_OFF, ptr(out3), ptr(work), stream()), "sums")
    torch.cuda.synchronize()
    del work
    return out3


@pytest.mark.parametrize("rows", [1, 37, 8200])
def test_dft_mag_and_loss_sums(rows):
    check, L, ptr, stream = _lib()
    xr, xi, yr, yi = _spectra(rows)
    cxd, cyd = _layout(xr, xi).cuda(), _layout(yr, yi).cuda()
    mbuf, mag = _guarded((rows, BINS))
    check(L.mfpa_dft_mag(ptr(cxd), rows, BINS, LDC, IM_OFF, ptr(mag), stream()), "dft_mag")
    torch.cuda.synchronize()
    got, want = mag.cpu().double(), _mag64(xr, xi)
    assert _guards_intact(mbuf)
    rel = ((got - want).abs() / want).max()
    assert float(rel) <= 1e-6, float(rel)                  # three float32 roundings and a correctly rounded root: < 3 * 2^-24 = 1.8e-7
    # the sums: float32 per-element terms, added in float64
    xm, ym = _mag32(xr, xi), _mag32(yr, yi)
    d = ym - xm
    want3 = [float((d * d).double().sum()), float((ym * ym).double().sum()), float((torch.log(ym) - torch.log(xm)).abs().double().sum())]
    got3 = _device_sums(cxd, cyd, rows).cpu().tolist()
    np.testing.assert_allclose(got3, want3, rtol=2e-5, atol=0)
    # cx == cy: the first and the third sum are exactly 0
    same = _device_sums(cyd, cyd.clone(), rows).cpu().tolist()
    assert same[0] == 0.0 and same[2] == 0.0
    np.testing.assert_allclose(same[1], want3[1], rtol=2e-5, atol=0)
    # all clamped: sums[1] = rows * bins * 1e-7f up to the float32 square of the root
    z = torch.zeros(rows, BINS)
    zd, td = _layout(z, z).cuda(), _layout(z + 1e-4, z + 1e-4).cuda()
    clamped = _device_sums(zd, td, rows).cpu().tolist()
    assert clamped[0] == 0.0 and clamped[2] == 0.0
    np.testing.assert_allclose(clamped[1], rows * BINS * float(np.float32(CLAMP)), rtol=1e-6, atol=0)
    assert _only_owned_columns_written(cxd.cpu()) and _only_owned_columns_written(cyd.cpu())
    del cxd, cyd, zd, td


def _grad_reference(xr, xi, yr, yi, w_sc, w_mag):
    """float64 autograd of w_sc * || |Y| - |X| ||_F / || Y ||_F + w_mag * mean | log|Y| - log|X| | through sqrt(clamp(re^2 + im^2, 1e-7))."""
    re, im = xr.double().requires_grad_(True), xi.double().requires_grad_(True)
    xm, ym = _mag64(re, im), _mag64(yr, yi)
    loss = w_sc * torch.linalg.norm(ym - xm) / torch.linalg.norm(ym) + w_mag * (torch.log(ym) - torch.log(xm)).abs().mean()
    loss.backward()
    return re.grad, im.grad


@pytest.mark.parametrize("w_sc,w_mag", [(0.5 / 3, 0.5 / 3), (0.1, 0.0), (0.0, 0.1)])
def test_stft_loss_grad_element_by_element(w_sc, w_mag):
    check, L, ptr, stream = _lib()
    rows = 37
    xr, xi, yr, yi = _spectra(rows)
    cxd, cyd = _layout(xr, xi).cuda(), _layout(yr, yi).cuda()
    sums = _device_sums(cxd, cyd, rows)                                      # the forward's, on the same data
    check(L.mfpa_stft_loss_grad(ptr(cxd), ptr(cyd), rows, BINS, LDC, IM_OFF, ptr(sums), w_sc, w_mag, stream()), "grad")
    torch.cuda.synchronize()
    out = cxd.cpu()
    assert _only_owned_columns_written(out)                                  # the kernel writes only what it owns
    got_re, got_im = out[:, :BINS].double(), out[:, IM_OFF:IM_OFF + BINS].double()
    ref_re, ref_im = _grad_reference(xr, xi, yr, yi, w_sc, w_mag)
    clamped = (xr.double() ** 2 + xi.double() ** 2) < CLAMP
    assert int(clamped.sum()) > 0.15 * rows * BINS
    for got, ref in ((got_re, ref_re), (got_im, ref_im)):
        assert bool(torch.isfinite(got).all())
        assert bool((ref[clamped] == 0).all()) and bool((got[clamped] == 0).all())       # below the clamp: exactly 0.0
        for r, k in ((0, 3), (rows - 1, 200), (0, 5), (0, 6)):                            # the planted zeros
            assert ref[r, k] == 0 and got[r, k] == 0, (r, k, float(got[r, k]))
        err = (got - ref).abs()
        bad = err > 1e-5 * ref.abs()
        assert not bool(bad.any()), (int(bad.sum()), float((err / ref.abs().clamp_min(1e-300)).max()))
    assert int((ref_re != 0).sum()) > 0.7 * rows * BINS                      # ... and the rest is a real gradient
    del cyd, sums


def test_stft_loss_grad_of_equal_spectra_is_zero():
    """cx == cy: n_diff = 0, so k_sc must be 0 (not w_sc / 0); every output is exactly 0."""
    check, L, ptr, stream = _lib()
    rows = 37
    _, _, yr, yi = _spectra(rows)
    cxd, cyd = _layout(yr, yi).cuda(), _layout(yr, yi).cuda()
    sums = _device_sums(cxd, cyd, rows)
    assert float(sums[0]) == 0.0
    check(L.mfpa_stft_loss_grad(ptr(cxd), ptr(cyd), rows, BINS, LDC, IM_OFF, ptr(sums), 0.5 / 3, 0.5 / 3, stream()), "grad")
    torch.cuda.synchronize()
    out = cxd.cpu()
    assert _only_owned_columns_written(out)
    owned = torch.cat([out[:, :BINS], out[:, IM_OFF:IM_OFF + BINS]], dim=1)
    assert bool((owned == 0).all()), int((owned != 0).sum())                 # NaN != 0: this is also the no-NaN check
    del cyd, sums
