"""CPU: the host oracle of mfpa_gemm_mfma (tests/_gemm_oracle.py) is the operation torch computes, the case table of
tests/test_gpu_gemm.py reaches every kernel with its preconditions met (mfpa_gemm_mfma_route: host arithmetic, no GPU), and the
bounds that test asserts are met by correct arithmetic with room to spare and missed tenfold by faulty arithmetic."""
import ctypes
from dataclasses import replace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _gemm_oracle as go


@pytest.fixture(scope="module")
def lib():
    import os
    from musicfpaugment_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from musicfpaugment_amd.csrc.build import build
        build(verbose=False)
    return _lib


def _route(lib, d):
    k = ctypes.c_int(-7)
    rc = lib.lib().mfpa_gemm_mfma_route(ctypes.byref(d), ctypes.byref(k))
    return rc, k.value


def _flat_a(c, rows):
    """rows (batch, region_a) float32 -> the flat A of the case's geometry, NaN in the gaps."""
    A = torch.full((c.batch * c.stride_a,), float("nan"))
    for b in range(c.batch):
        A[b * c.stride_a:b * c.stride_a + c.region_a] = rows[b]
    return A


def _pad(t, npad):
    out = torch.zeros((npad,) + tuple(t.shape[1:]))
    out[:t.shape[0]] = t
    return out


@pytest.mark.parametrize("B,Cin,Cout,Lout", [(2, 4, 5, 7), (1, 8, 70, 3)])
def test_reference_is_conv1d_relu_and_glu(B, Cin, Cout, Lout):
    g = torch.Generator().manual_seed(1)
    Lin = 4 * (Lout - 1) + 8
    h = torch.randn(B, Cin, Lin, generator=g)
    w = torch.randn(Cout, Cin, 8, generator=g) / np.sqrt(8 * Cin)
    bias = torch.randn(Cout, generator=g)
    want = F.relu(F.conv1d(h.double(), w.double(), bias.double(), stride=4))                  # (B, Cout, Lout)
    npad = (Cout + 63) // 64 * 64
    c = go.Case(go.MFMA, 0, 8 * Cin, npad, Cout, Lout, B, lda=4 * Cin, mode=0, relu=1)         # row t = h[4t : 4t+8] flattened
    inp = {"A": _flat_a(c, h.permute(0, 2, 1).reshape(B, -1)), "W": _pad(w.permute(0, 2, 1).reshape(Cout, -1), npad),
           "bias": _pad(bias, npad), "addend": None}
    got = go.reference(c, inp)["C"]
    assert got.shape == (B, Lout, Cout)
    torch.testing.assert_close(got.permute(0, 2, 1), want, rtol=1e-12, atol=1e-12)
    # 1x1 + GLU on that output, K padded to a multiple of 16 with zero columns
    K = (Cout + 15) // 16 * 16
    wg = torch.randn(2 * Cout, Cout, generator=g) / np.sqrt(Cout)
    bg = torch.randn(2 * Cout, generator=g)
    a = got.float()
    want_g = F.glu(F.conv1d(a.double().permute(0, 2, 1), wg.double()[:, :, None], bg.double()), dim=1)
    npad = (Cout + 31) // 32 * 64
    c = go.Case(go.MFMA, 0, K, npad, Cout, Lout, B, mode=1)
    ak = torch.zeros(B, Lout, K)
    ak[..., :Cout] = a
    wk = torch.zeros(2 * Cout, K)
    wk[:, :Cout] = wg
    wp, bp = go.pack_glu(wk, bg, npad)
    from musicfpaugment_amd.ops_demucs import _pack_glu
    assert torch.equal(wp, _pack_glu(wk, bg)[0]) and torch.equal(bp, _pack_glu(wk, bg)[1])      # the product's packing order
    r = go.reference(c, {"A": _flat_a(c, ak.reshape(B, -1)), "W": wp, "bias": bp, "addend": None})
    torch.testing.assert_close(r["C"].permute(0, 2, 1), want_g, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("B,H,Cout,L", [(2, 8, 3, 5), (1, 16, 20, 2)])
def test_reference_is_the_transposed_convolution_as_a_gemm(B, H, Cout, L):
    """ConvTranspose1d(k8, s4) + ReLU + skip as _demucs_forward lays it out: row t = [g[t-1] | g[t]] of a buffer with a zero row at
    each end, W row j*Cout + co = [taps j+4 | taps j], output row t = positions 4t .. 4t+3; mode 2, relu 2, C2 = the ReLU output."""
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, H, L, generator=g)
    w = torch.randn(H, Cout, 8, generator=g) / np.sqrt(2 * H)
    bias = torch.randn(Cout, generator=g)
    skip = torch.randn(B, Cout, 4 * (L + 1), generator=g)
    pre = F.relu(F.conv_transpose1d(x.double(), w.double(), bias.double(), stride=4))
    want = pre + skip.double()
    N, npad = 4 * Cout, (4 * Cout + 63) // 64 * 64
    c = go.Case(go.MFMA, 0, 2 * H, npad, N, L + 1, B, lda=H, mode=2, relu=2, c2=True)
    P = torch.zeros(B, L + 2, H)
    P[:, 1:L + 1] = x.permute(0, 2, 1)
    wt = torch.cat([w[:, :, 4:8].permute(2, 1, 0), w[:, :, 0:4].permute(2, 1, 0)], dim=2).reshape(N, 2 * H)
    ad = torch.full((B * c.stride_add,), float("nan"))
    for b in range(B):
        ad[b * c.stride_add:b * c.stride_add + c.M * c.ldadd].view(c.M, c.ldadd)[:, :N] = skip[b].t().reshape(L + 1, N)
    r = go.reference(c, {"A": _flat_a(c, P.reshape(B, -1)), "W": _pad(wt, npad), "bias": _pad(bias.repeat(4), npad), "addend": ad})
    torch.testing.assert_close(r["C"].reshape(B, 4 * (L + 1), Cout).permute(0, 2, 1), want, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(r["C2"].reshape(B, 4 * (L + 1), Cout).permute(0, 2, 1), pre, rtol=1e-12, atol=1e-12)


def test_reference_c1_source_and_mask_modes():
    """The fused first layer is Conv1d(1 -> K, k8, s4) + ReLU; mode 3 is the ReLU-backward mask (zero where the addend is <= 0)."""
    c = next(x for x in go.CASES if x.kid == go.MFMA_C1 and x.mode == 3)
    inp = go.inputs_for(c)
    A = go._windows(c, inp)
    want = F.relu(F.conv1d(inp["x"].double()[:, None, :], inp["c1_w"].double().t()[:, None, :], inp["c1_b"].double(), stride=4))
    torch.testing.assert_close(A, want.permute(0, 2, 1)[:, :c.M], rtol=1e-12, atol=1e-12)
    assert float((go._c1_windows_f32(c, inp).double() - A).abs().max()) < 1e-5
    r = go.reference(c, inp)
    ad = go._addend(c, inp)
    assert int((ad == 0).sum()) > 0 and float(ad[ad != 0].abs().min()) >= 0.1
    assert torch.equal(r["C"] == 0, (ad <= 0) | (r["pre"][..., :c.N] == 0))
    torch.testing.assert_close(r["C"][ad > 0], r["pre"][..., :c.N][ad > 0], rtol=0, atol=0)


def test_every_case_routes_to_the_kernel_it_names(lib):
    seen = set()
    for c in go.CASES:
        rc, kid = _route(lib, go.descriptor(go.fixed(c)))
        assert (rc, kid) == (0, c.kid), c.name
        seen.add(kid)
        if c.walk:                                    # more tiles than workgroups on a 256-CU device, and no multiple of 8
            f = go.fixed(c, 256)
            tiles = (f.npad // 128) * ((f.M + 255) // 256) * f.batch
            assert tiles > 256 and tiles % 8
    assert seen == set(range(12))
    assert len(go.CASES) <= 110                       # launches of the GPU suite (the identity groups add ~ 20)


def test_route_preconditions_over_a_sweep(lib):
    """For every accepted descriptor of the sweep the chosen kernel's own preconditions hold; a pre-split W reaches only a WSPLIT
    instantiation and c1_x only a C1SRC one."""
    accepted = 0
    for prec in (0, 1, 2):
        for K in list(range(16, 321, 16)) + [768]:
            for npad in (64, 128, 192, 256):
                for M in (1, 191, 192):
                    for c1 in (False, True):
                        base = go.Case(go.MFMA, prec, K, npad, 30, M, 2, c1=c1)
                        rc, kid = _route(lib, go.descriptor(base))
                        assert rc in (0, lib.EINVAL)
                        if rc:
                            assert kid == go.NONE
                            continue
                        accepted += 1
                        tag = (prec, K, npad, M, c1, kid)
                        assert 0 <= kid < 12, tag
                        if kid in (go.PIPE, go.PIPE_WSPLIT):
                            assert K % 64 == 0 and K >= 128 and npad % 128 == 0 and M >= 192, tag
                        if kid in (go.WIDE, go.WIDE_WSPLIT):
                            assert K % 32 == 0 and K >= 128 and npad % 128 == 0, tag
                        if kid == go.BF16X3:
                            assert K % 32 == 0 and K >= 128, tag
                        if kid in (go.SHORTK48_C1, go.SHORTK48, go.SMALLK48_C1, go.SMALLK48):
                            assert K == 48, tag
                        if kid == go.SHORTK96:
                            assert K == 96, tag
                        assert (prec == 2) == (kid in go.WSPLIT_IDS), tag
                        assert c1 == (kid in go.C1SRC_IDS), tag
                        if c1:
                            assert K <= 256, tag
                        if prec == 0:
                            assert kid in go.FP32_IDS, tag
    assert accepted > 500


_ratio = go.ratio


@pytest.mark.parametrize("case", go.CASES, ids=lambda c: c.name)
def test_bounds_are_satisfiable(case):
    """Correct arithmetic sits well inside the bounds: the bf16x3 model is within half of 2^-15 S of the reference, and a float32
    accumulation of the same products within half of the fp32 bound."""
    c = go.fixed(case)
    inp = go.inputs_for(c)
    ref = go.reference(c, inp)
    c1 = 9 * go.U24 * ref["c1"] if c.c1 else 0.0
    assert torch.isfinite(ref["C"]).all() and torch.isfinite(ref["S"]).all()         # no gap NaN inside a window
    if c.kid not in go.FP32_IDS:
        m = go.model_bf16x3(c, inp)
        assert _ratio((m["pre"] - ref["pre"]).abs(), 0.5 * go.U15 * ref["S"] + c1) <= 1.0
    A32 = (go._c1_windows_f32(c, inp) if c.c1 else go._windows(c, inp, torch.float32)).numpy()
    pre32 = np.matmul(A32, inp["W"].numpy().T)
    if inp["bias"] is not None:
        pre32 = pre32 + inp["bias"].numpy()
    assert pre32.dtype == np.float32
    assert _ratio((torch.from_numpy(pre32).double() - ref["pre"]).abs(), 0.5 * go.pre_bound(c, ref, "fp32")) <= 1.0


_BITE = [c for c in go.CASES if c.M >= 2 and not c.walk and c.precision != 2]


@pytest.mark.parametrize("case", _BITE, ids=lambda c: c.name)
def test_faulty_variants_miss_the_bounds_tenfold(case):
    """Each faulty variant of the arithmetic exceeds the bound the GPU test asserts, by 10 x or more in at least one element: a dropped
    cross term (against the model bound: only that check can see it), a skipped 32-wide K chunk, the last row taken from the row
    before it, value and gate swapped in one GLU tile (against the loosest bound their kernel is held to)."""
    c, inp = case, go.inputs_for(case)
    ref = go.reference(c, inp)
    fp32 = c.kid in go.FP32_IDS
    build = go.model_fp32_exact if fp32 else go.model_bf16x3
    loose = "fp32" if fp32 else "reference"
    if not fp32:
        m = go.model_bf16x3(c, inp)
        for drop in ("ah_bl", "al_bh"):
            f = go.model_bf16x3(c, inp, drop=drop)
            assert _ratio((f["pre"] - m["pre"]).abs(), go.pre_bound(c, ref, "model")) >= 10.0, drop
    if c.K >= 32:
        f = build(c, inp, skip_chunk=c.K // 32 - 1)
        assert _ratio((f["pre"] - ref["pre"]).abs(), go.pre_bound(c, ref, loose)) >= 10.0
    f = build(c, inp, dup_last_row=True)
    assert _ratio((f["pre"] - ref["pre"])[:, c.M - 1].abs(), go.pre_bound(c, ref, loose)[:, c.M - 1]) >= 10.0
    if c.mode == 1:
        f = build(c, inp, swap_glu_tile=(c.N - 1) // 32)
        assert _ratio((f["C"] - ref["C"]).abs(), go.out_bound(c, ref, loose)) >= 10.0


def test_glu_tolerance_from_stored_preactivations_holds_in_float32():
    """v sigma(g) evaluated in float32 as 1 / (1 + exp2(-g log2 e)) stays within (|g| + 4) 2^-23 relative of the float64 value."""
    g = torch.Generator().manual_seed(5)
    v, gate = torch.randn(100000, generator=g) * 3, torch.randn(100000, generator=g) * 6
    got = v * (1.0 / (1.0 + torch.exp2(-(gate * np.float32(1.4426950408889634)))))
    want = v.double() * torch.sigmoid(gate.double())
    assert bool(((got.double() - want).abs() <= go.glu_from_c2_bound(v.double(), gate.double())).all())
