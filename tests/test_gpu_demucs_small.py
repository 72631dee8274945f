"""GPU: the Demucs VALU kernels (csrc/demucs.hip: mfpa_demucs_prep, mfpa_upsample2, mfpa_downsample2, mfpa_conv1d_c1, mfpa_convT1d_c1 and
its _dev form) and the training step's small kernels (csrc/demucs_train.hip: mfpa_downsample2_adjoint, mfpa_c1_wgrad, mfpa_colsum_any,
mfpa_glu_bwd and the six kernels of mfpa_gemm_tn), element by element, through the C entry points.

The case tables, the float64 restatements and the exactness argument are tests/_demucs_small_oracle.py (pinned on the CPU by
tests/test_demucs_small_oracle.py).  Operands are small integers (asymmetric integer taps, power-of-two scales, a + b 2^-10 for the bf16
GEMMs), so the expected float32 output is exact under any summation or atomic order and the comparison is torch.equal; mfpa_demucs_prep
and mfpa_glu_bwd have derived bounds instead and print their worst error / bound as a DEMUCS-SMALL line (a record for NOTES.md, not a
threshold).  Every output buffer starts as a NaN sentinel that must survive wherever the kernel has no business writing; row pads and
the gaps between the clips of every input hold NaN, which a correct kernel never reads.

Not reached at test size (each would need an allocation of gigabytes): the 65536-block cap of mfpa_glu_bwd (2^24 threads: rows * npad / 8
above that) and the 2048-block cap of mfpa_colsum_any (rows * C above 2^26)."""
import ctypes

import pytest
import torch

from tests import _demucs_small_oracle as so

pytestmark = pytest.mark.gpu


def _api():
    from musicfpaugment_amd import _lib
    return _lib


def _dev(t):
    return None if t is None else t.contiguous().cuda()


def _run(name, built, call):
    """Upload the inputs, pre-fill the outputs, make the call, compare every flat output buffer with its expected contents."""
    L = _api()
    inp = {k: _dev(v) for k, v in built.inp.items()}
    out = {k: init.clone().cuda() for k, (init, _) in built.out.items()}
    L.check(call(L.lib(), L.ptr, inp, out, L.stream()), name)
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, v in out.items()}
    for k, (_, want) in built.out.items():
        msg = so.mismatch(got[k], want)
        assert msg is None, f"{name}: {k}: {msg}"
    return inp, got


# ------------------------------------------------------------------------------------------------ resamplers
def _rs_call(c, aux):
    if c.kind == "up":
        return lambda lib, p, i, o, st: lib.mfpa_upsample2(p(i["x"]), c.B, c.T, p(i["ker"]), p(o["y"]), st)
    if c.kind == "down":
        return lambda lib, p, i, o, st: lib.mfpa_downsample2(p(i["x"]), c.B, c.T, p(i["ker"]), p(o["y"]), aux["To"], p(i["scale"]), c.keep, st)
    return lambda lib, p, i, o, st: lib.mfpa_downsample2_adjoint(p(i["dy"]), c.B, aux["ldy"], c.keep, p(i["ker"]), p(i["scale"]), c.T,
                                                                 p(o["dx"]), st)


@pytest.mark.parametrize("case", so.RS_CASES, ids=lambda c: c.name)
def test_resamplers_exact(case):
    b = so.rs_build(case)
    _run(case.name, b, _rs_call(case, b.aux))


@pytest.mark.parametrize("T", [2, 57, 1025, 2052])
def test_downsample_inner_product_identity_on_the_device(T):
    """<down(x), dy> == <x, adj(dy)> with both sides from the device on the same integer data: every term is a multiple of 1/4 below 2^24."""
    th = (T + 1) // 2
    for nout in sorted({th, max(1, th - 1)}):
        down, adj = so.RsCase("down", 3, T, nout, 3, True), so.RsCase("adj", 3, T, nout, 3, True)
        bd, ba = so.rs_build(down), so.rs_build(adj)
        _, gd = _run(down.name, bd, _rs_call(down, bd.aux))
        _, ga = _run(adj.name, ba, _rs_call(adj, ba.aux))
        y = gd["y"][:-so.GUARD].view(3, nout + 3)[:, :nout].double()
        dx = ga["dx"][:-so.GUARD].view(3, T).double()
        assert float((y * ba.aux["dy64"]).sum()) == float((bd.inp["x"].view(3, T).double() * dx).sum())


# ------------------------------------------------------------------------------------------------ 1-channel convolutions
@pytest.mark.parametrize("case", so.CONV_CASES, ids=lambda c: c.name)
def test_conv1d_c1_exact(case):
    c = case
    _run(c.name, so.conv_build(c), lambda lib, p, i, o, st: lib.mfpa_conv1d_c1(p(i["x"]), c.B, c.lin, c.L, c.C, p(i["w"]), p(i["bias"]),
                                                                               c.relu, p(o["y"]), st))


@pytest.mark.parametrize("case", so.CONVT_CASES, ids=lambda c: c.name)
def test_convT1d_c1_exact_and_both_entry_points_agree(case):
    c = case
    b = so.convT_build(c)
    _, host = _run(c.name, b, lambda lib, p, i, o, st: lib.mfpa_convT1d_c1(p(i["P"]), c.B, c.L, c.C, p(i["w"]), b.aux["bias"], p(o["y"]), st))
    _, dev = _run(c.name + "-dev", b, lambda lib, p, i, o, st: lib.mfpa_convT1d_c1_dev(p(i["P"]), c.B, c.L, c.C, p(i["w"]), p(i["bias"]),
                                                                                     p(o["y"]), st))
    assert so.same_bits(host["y"], dev["y"])


@pytest.mark.parametrize("case", so.C1W_CASES, ids=lambda c: c.name)
def test_c1_wgrad_exact(case):
    c = case
    _run(c.name, so.c1w_build(c), lambda lib, p, i, o, st: lib.mfpa_c1_wgrad(p(i["x"]), c.ldx, p(i["g"]) + 4 * c.g_offset, c.ldg, c.stride_g,
                                                                             c.B, c.L, c.C, p(o["dw"]), st))


@pytest.mark.parametrize("case", so.COLSUM_CASES, ids=lambda c: c.name)
def test_colsum_any_exact(case):
    c = case
    _run(c.name, so.colsum_build(c), lambda lib, p, i, o, st: lib.mfpa_colsum_any(p(i["x"]), c.rows, c.C, c.ld, p(o["out"]), st))


# ------------------------------------------------------------------------------------------------ TN weight-gradient GEMM
def _tn_desc(c, p, i, o, **over):
    L = _api()
    f = dict(A=p(i["A"]), lda=c.lda, strideA=c.stride_a, Bm=p(i["Bm"]), ldb=c.ldb, strideB=c.stride_b, C=p(o["C"]), ldc=c.ldc, batch=c.batch,
             R=c.R, M=c.M, N=c.N, colsum=p(o.get("colsum")), precision=c.precision)
    f.update(over)
    return L.GemmTnDesc(**f)


@pytest.mark.parametrize("case", so.TN_CASES, ids=lambda c: c.name)
def test_gemm_tn_exact(case):
    c = case

    def call(lib, p, i, o, st):
        d = _tn_desc(c, p, i, o)
        return lib.mfpa_gemm_tn(ctypes.byref(d), st)

    _run(c.name, so.tn_build(c), call)


# ------------------------------------------------------------------------------------------------ the two bounded kernels
@pytest.mark.parametrize("case", so.PREP_CASES, ids=lambda c: c.name)
def test_demucs_prep_within_bound(case):
    c, L = case, _api()
    floor32 = float(torch.tensor(so.PREP_FLOOR, dtype=torch.float32))
    x = so.prep_inputs(c)
    xd, out, std = x.cuda(), so.sentinel(c.B * c.VL + so.GUARD).cuda(), so.sentinel(c.B + so.GUARD).cuda()
    L.check(L.lib().mfpa_demucs_prep(L.ptr(xd), c.B, c.T, c.VL, floor32, L.ptr(out), L.ptr(std), L.stream()), c.name)
    torch.cuda.synchronize()
    out, std = out.cpu(), std.cpu()
    assert bool((out.view(torch.int32)[-so.GUARD:] == so.SENTINEL_BITS).all()) and bool((std.view(torch.int32)[-so.GUARD:] == so.SENTINEL_BITS).all())
    got, got_std = out[:-so.GUARD].view(c.B, c.VL), std[:-so.GUARD]
    ref, ref_std = so.prep(x.double(), c.VL, floor32)
    b_out, b_std = so.prep_bounds(ref, ref_std)
    assert bool((got[:, c.T:].view(torch.int32) == 0).all()), "the pad to VL is not exactly +0.0"
    r_out, r_std = so.ratio((got.double() - ref).abs()[:, :c.T], b_out[:, :c.T]), so.ratio((got_std.double() - ref_std).abs(), b_std)
    print(f"\nDEMUCS-SMALL prep {c.name} out={r_out:.4f} std={r_std:.4f}")
    assert r_out <= 1.0 and r_std <= 1.0, (r_out, r_std)


@pytest.mark.parametrize("case", so.GLU_CASES, ids=lambda c: c.name)
def test_glu_bwd_within_bound(case):
    c, L = case, _api()
    u, dg_flat, dg = so.glu_inputs(c)
    ud = torch.cat([u.reshape(-1), so.sentinel(so.GUARD)]).cuda()
    dgd = dg_flat.cuda()
    L.check(L.lib().mfpa_glu_bwd(L.ptr(ud), c.rows, c.npad, c.N, L.ptr(dgd), c.ldg, L.stream()), c.name)
    torch.cuda.synchronize()
    got = ud.cpu()
    assert bool((got.view(torch.int32)[-so.GUARD:] == so.SENTINEL_BITS).all())
    got = got[:-so.GUARD].view(c.rows, c.npad)
    ref, scale = so.glu_bwd(u.double(), dg.double(), c.N)
    pad = scale == 0                                           # n >= N in both halves (|d| and |d v| are 0 there and, with random d and v, only there)
    assert int(pad.sum()) == c.rows * (c.npad - 2 * c.N) and bool((got[pad] == 0).all()), "a pad column is not exactly 0"
    r = so.ratio((got.double() - ref).abs()[~pad], so.glu_bound(scale)[~pad])
    print(f"\nDEMUCS-SMALL glu_bwd {c.name} ratio={r:.4f}")
    assert r <= 1.0, r


# ------------------------------------------------------------------------------------------------ argument checks
def test_invalid_arguments_are_refused_and_an_empty_batch_is_a_no_op():
    L = _api()
    lib, p, st, EINVAL = L.lib(), L.ptr, L.stream(), L.EINVAL
    buf = so.sentinel(4096).cuda()                             # any valid address: every call below returns before a launch
    a = p(buf)
    tn = so.TnCase(8, 8, 4, 1, 0, False)
    io = ({"A": buf, "Bm": buf}, {"C": buf})
    bad_tn = [dict(M=6), dict(N=6), dict(lda=10), dict(ldc=4), dict(precision=3)]
    for over in bad_tn:
        d = _tn_desc(tn, p, *io, **over)
        assert lib.mfpa_gemm_tn(ctypes.byref(d), st) == EINVAL, over
    assert lib.mfpa_downsample2(a, 1, 10, a, a, 8, 0, 6, st) == EINVAL                   # Tkeep 6 > Th 5
    assert lib.mfpa_downsample2(a, 1, 10, a, a, 4, 0, 0, st) == EINVAL                   # To 4 < nout 5
    assert lib.mfpa_downsample2_adjoint(a, 1, 6, 6, a, 0, 10, a, st) == EINVAL           # nout 6 > Th 5
    assert lib.mfpa_conv1d_c1(a, 1, 8, 1, 6, a, a, 0, a, st) == EINVAL                   # C % 4
    assert lib.mfpa_convT1d_c1(a, 1, 1, 6, a, 0.0, a, st) == EINVAL
    assert lib.mfpa_convT1d_c1_dev(a, 1, 1, 6, a, a, a, st) == EINVAL
    assert lib.mfpa_colsum_any(a, 1, 6, 8, a, st) == EINVAL
    assert lib.mfpa_c1_wgrad(a, 8, a, 6, 8, 1, 1, 6, a, st) == EINVAL                    # C % 4
    assert lib.mfpa_c1_wgrad(a, 8, a, 260, 260, 1, 1, 260, a, st) == EINVAL              # C > 256
    assert lib.mfpa_glu_bwd(a, 1, 64, 36, a, 36, st) == EINVAL                           # N > npad / 2
    # B == 0: MFPA_OK without a launch, whatever the other arguments
    d = _tn_desc(tn, p, *io, batch=0)
    assert lib.mfpa_gemm_tn(ctypes.byref(d), st) == 0
    assert lib.mfpa_demucs_prep(a, 0, 10, 10, 1e-3, a, a, st) == 0
    assert lib.mfpa_upsample2(a, 0, 10, a, a, st) == 0
    assert lib.mfpa_downsample2(a, 0, 10, a, a, 5, 0, 0, st) == 0
    assert lib.mfpa_downsample2_adjoint(a, 0, 5, 5, a, 0, 10, a, st) == 0
    assert lib.mfpa_conv1d_c1(a, 0, 8, 1, 4, a, a, 0, a, st) == 0
    assert lib.mfpa_convT1d_c1(a, 0, 1, 4, a, 0.0, a, st) == 0
    assert lib.mfpa_convT1d_c1_dev(a, 0, 1, 4, a, a, a, st) == 0
    assert lib.mfpa_c1_wgrad(a, 8, a, 4, 4, 0, 1, 4, a, st) == 0
    assert lib.mfpa_colsum_any(a, 0, 4, 4, a, st) == 0
    assert lib.mfpa_glu_bwd(a, 0, 64, 4, a, 4, st) == 0
    torch.cuda.synchronize()
    assert bool((buf.cpu().view(torch.int32) == so.SENTINEL_BITS).all())
