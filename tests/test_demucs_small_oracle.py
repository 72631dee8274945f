"""CPU: tests/_demucs_small_oracle.py is pinned against torch (the resamplers against oracle/demucs.py with the real sinc taps, the
adjoints and weight gradients against autograd, the convolutions against torch's own, prep against torch.std); every case of its tables
satisfies the preconditions of its exactness argument; and the tables discriminate: each deliberately faulty variant changes the expected
output of at least one case -- by ten times the bound for the two tolerance models -- while the real, symmetric sinc taps would have
hidden a flipped tap walk, which is why the tables use asymmetric taps."""
import pytest
import torch
import torch.nn.functional as F

from oracle import demucs as od
from tests import _demucs_small_oracle as so

REAL_TAPS = od.sinc_kernel().double().reshape(-1)


def _close(a, b, tol=1e-12):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


# ------------------------------------------------------------------------------------------------ the restatements against torch
@pytest.mark.parametrize("T", [1, 2, 57, 300, 301])
def test_resamplers_match_the_oracle_with_the_real_taps(T):
    x = torch.randn(2, T, generator=torch.Generator().manual_seed(T), dtype=torch.float64)
    assert _close(so.upsample2(x, REAL_TAPS), od.upsample2(x))
    if T >= 2:
        assert _close(so.downsample2(x, REAL_TAPS), od.downsample2(x))


@pytest.mark.parametrize("T,keep", [(2, 1), (57, 29), (300, 150), (301, 151), (301, 77)])
def test_downsample_adjoint_matches_autograd_and_the_inner_product_identity(T, keep):
    g = torch.Generator().manual_seed(T + keep)
    x = torch.randn(2, T, generator=g, dtype=torch.float64).requires_grad_(True)
    sc = torch.tensor([0.5, 4.0], dtype=torch.float64)
    dy = torch.randn(2, keep, generator=g, dtype=torch.float64)
    (od.downsample2(x)[:, :keep] * sc[:, None]).backward(dy)
    adj = so.downsample2_adjoint(dy, REAL_TAPS, T, sc)
    assert _close(adj, x.grad)
    # <down(x), dy> == <x, adj(dy)>, exactly on the integer data of the table
    taps = so.int_taps()
    xi, dyi = so.ints(g, 2, T), so.ints(g, 2, keep)
    lhs = (so.downsample2(xi, taps, sc, keep) * dyi).sum()
    rhs = (xi * so.downsample2_adjoint(dyi, taps, T, sc)).sum()
    assert float(lhs) == float(rhs)


def test_one_channel_convolutions_match_torch():
    g = torch.Generator().manual_seed(5)
    B, C, L = 2, 12, 9
    x = torch.randn(B, 4 * (L - 1) + 8 + 3, generator=g, dtype=torch.float64)
    w = torch.randn(8, C, generator=g, dtype=torch.float64)                     # tap-major (8, C) = Conv1d weight (C, 1, 8) transposed
    b = torch.randn(C, generator=g, dtype=torch.float64)
    want = F.conv1d(x[:, None, :4 * (L - 1) + 8], w.t()[:, None, :], b, stride=4)         # (B, C, L)
    assert _close(so.conv1d_c1(x, w, b, L, False), want.permute(0, 2, 1))
    assert _close(so.conv1d_c1(x, w, None, L, True), F.relu(want - b[None, :, None]).permute(0, 2, 1))
    # ConvTranspose1d(C -> 1, k8, s4) of the (B, L, C) rows between the two zero rows; weight (C, 1, 8) = w tap-major transposed
    P = torch.zeros(B, L + 2, C, dtype=torch.float64)
    P[:, 1:-1] = torch.randn(B, L, C, generator=g, dtype=torch.float64)
    wantT = F.conv_transpose1d(P[:, 1:-1].permute(0, 2, 1), w.t()[:, None, :], torch.tensor([0.7], dtype=torch.float64), stride=4)
    assert _close(so.convT1d_c1(P, w, 0.7), wantT[:, 0])
    # weight gradient of the 1 -> C convolution
    wt = w.t()[:, None, :].clone().requires_grad_(True)
    gr = torch.randn(B, L, C, generator=g, dtype=torch.float64)
    F.conv1d(x[:, None, :4 * (L - 1) + 8], wt, stride=4).backward(gr.permute(0, 2, 1))
    assert _close(so.c1_wgrad(x, gr), wt.grad[:, 0].t())


def test_gemm_tn_reference_is_the_conv1d_weight_gradient():
    c = next(c for c in so.TN_CASES if c.cin and c.precision == 0 and c.M == 48)
    A, Bv, C0, cs0 = so._tn_operands(c.operand_key)                              # dy (B, L, cout), x (B, Lin, cin)
    b = so.tn_build(c)
    got = b.out["C"][1].as_strided((c.M, c.N), (c.ldc, 1)).double() - C0
    w = torch.zeros(c.M, c.cin, 8, dtype=torch.float64, requires_grad=True)
    F.conv1d(Bv.permute(0, 2, 1), w, stride=4).backward(A.permute(0, 2, 1))
    assert torch.equal(got, w.grad.permute(0, 2, 1).reshape(c.M, 8 * c.cin))    # dW[co][j cin + c]
    assert torch.equal(b.out["colsum"][1][:c.M].double() - cs0, A.sum((0, 1)))


def test_glu_bwd_matches_autograd():
    c = so.GluCase(128, 48, 5, 4)
    u, _, dg = so.glu_inputs(c)
    t = u.double().reshape(c.rows, c.npad // 64, 2, 32)
    v = t[:, :, 0].reshape(c.rows, -1)[:, :c.N].clone().requires_grad_(True)
    s = t[:, :, 1].reshape(c.rows, -1)[:, :c.N].clone().requires_grad_(True)
    F.glu(torch.cat([v, s], dim=1), dim=1).backward(dg.double())
    du, _ = so.glu_bwd(u.double(), dg.double(), c.N)
    dt = du.reshape(c.rows, c.npad // 64, 2, 32)
    assert _close(dt[:, :, 0].reshape(c.rows, -1)[:, :c.N], v.grad) and _close(dt[:, :, 1].reshape(c.rows, -1)[:, :c.N], s.grad)
    assert bool((dt[:, :, 0].reshape(c.rows, -1)[:, c.N:] == 0).all()) and bool((dt[:, :, 1].reshape(c.rows, -1)[:, c.N:] == 0).all())
    assert float(u.reshape(c.rows, c.npad // 64, 2, 32)[:, :, 1].abs().max()) == so.GLU_SMAX


def test_prep_matches_torch_std():
    c = so.PREP_CASES[-1]
    x = so.prep_inputs(c).double()
    out, std = so.prep(x, c.VL, so.PREP_FLOOR)
    assert torch.equal(std, torch.std(x, dim=1)) and out.shape == (c.B, c.VL)
    assert torch.equal(out[:, :c.T], x / (torch.std(x, dim=1, keepdim=True) + so.PREP_FLOOR)) and bool((out[:, c.T:] == 0).all())


# ------------------------------------------------------------------------------------------------ every case's preconditions
_EXACT = ([("rs", c) for c in so.RS_CASES] + [("conv", c) for c in so.CONV_CASES] + [("convT", c) for c in so.CONVT_CASES] +
          [("c1w", c) for c in so.C1W_CASES] + [("colsum", c) for c in so.COLSUM_CASES] + [("tn", c) for c in so.TN_CASES])
_BUILD = {"rs": so.rs_build, "conv": so.conv_build, "convT": so.convT_build, "c1w": so.c1w_build, "colsum": so.colsum_build,
          "tn": so.tn_build}


@pytest.mark.parametrize("kind", list(_BUILD))
def test_every_exact_case_meets_its_preconditions(kind):
    """The makers assert integer-valuedness, the 2^24 bound and the exact bf16 split; here every case is built, and its buffers checked:
    sentinels behind every output and in every unwritten position, NaN in no position a reference read."""
    n = 0
    for k, c in _EXACT:
        if k != kind:
            continue
        b = _BUILD[kind](c)
        for name, (init, want) in b.out.items():
            assert init.shape == want.shape and bool((want.view(torch.int32)[-so.GUARD:] == so.SENTINEL_BITS).all())
            keep = want.view(torch.int32) == so.SENTINEL_BITS
            assert not bool(torch.isnan(want[~keep]).any()) and bool((init.view(torch.int32)[keep] == so.SENTINEL_BITS).all()), (c.name, name)
            assert so.mismatch(want, want) is None and so.mismatch(init, want) is not None
        n += 1
    assert n == {"rs": len(so.RS_CASES), "conv": 53, "convT": 10, "c1w": 24, "colsum": 24, "tn": len(so.TN_CASES)}[kind]


def test_gemm_tn_table_covers_every_kernel_and_branch():
    kernels = {(big, p) for big in (False, True) for p in (0, 1, 2)}
    assert {c.kernel for c in so.TN_CASES} == kernels                             # host rule: big = M > 64 and N > 64
    for k in kernels:
        mine = [c for c in so.TN_CASES if c.kernel == k]
        assert {c.colsum for c in mine} == {False, True}
        assert any(c.colsum and c.plan[4] > 1 for c in mine)                      # colsum with more than one n tile
        assert any(c.workgroups % 8 == 0 for c in mine) and any(c.workgroups % 8 for c in mine)
        assert any(c.N % (128 if k[0] else 64) for c in mine) and any(c.M % (128 if k[0] else 64) for c in mine)
        assert {c.plan[3] for c in mine} >= {1, 2, 3}                             # splits per clip
        assert any(c.lda > c.M for c in mine) and any(c.ldb > c.N for c in mine) and any(c.cin for c in mine)
    long = [c for c in so.TN_CASES if c.R == 9000]
    assert len(long) == 3 and all(c.plan[2:4] == (96, 94) for c in long)
    assert all(c.batch * c.R <= 1500 for c in so.TN_CASES if c.precision and c.split_ints)


def test_case_counts():
    assert len(so.TN_CASES) == 3 * (7 * 7 * 2 + 2 + 4 + 1) and len(so.GLU_CASES) == 16 and len(so.PREP_CASES) == 18
    assert len({c.name for c in so.RS_CASES}) == len(so.RS_CASES)


# ------------------------------------------------------------------------------------------------ the tables discriminate
def _differs(build, cases, fault):
    return [c.name for c in cases if any(not so.same_bits(build(c).out[k][1], build(c, fault=fault).out[k][1]) for k in build(c).out)]


_SMALL_RS = [c for c in so.RS_CASES if c.T <= 2052]


@pytest.mark.parametrize("fault,kinds", [("taps_flipped", ("up", "down")), ("tap_offset", ("up", "down")), ("xodd_even", ("down",)),
                                         ("adjoint_sign", ("adj",))])
def test_faulty_resamplers_differ_on_the_table(fault, kinds):
    for kind in kinds:
        cases = [c for c in _SMALL_RS if c.kind == kind]
        hit = _differs(so.rs_build, cases, fault)
        assert len(hit) >= len(cases) // 2, (fault, kind, len(hit), len(cases))


@pytest.mark.parametrize("fault", ["last_split_dropped", "split_straddles_clip", "colsum_every_tile"])
def test_faulty_gemm_tn_differs_on_the_table(fault):
    cases = [c for c in so.TN_CASES if c.R <= 130]
    hit = _differs(so.tn_build, cases, fault)
    assert hit, fault
    if fault == "colsum_every_tile":                                              # every colsum case with more than one n tile sees it
        assert set(hit) == {c.name for c in cases if c.colsum and c.plan[4] > 1}
    for p in (0, 1, 2):
        assert any(f"-p{p}" in n for n in hit)


def test_bf16_references_tell_the_three_precisions_apart():
    """The a + b 2^-10 operands: the bf16x3 reference differs from the plain-bf16 one and from the full product (al bl dropped)."""
    c1 = next(c for c in so.TN_CASES if c.precision == 1 and (c.M, c.N, c.R, c.batch) == (68, 68, 33, 3))
    c2 = next(c for c in so.TN_CASES if c.precision == 2 and (c.M, c.N, c.R, c.batch) == (68, 68, 33, 3))
    w1, w2 = so.tn_build(c1).out["C"][1], so.tn_build(c2).out["C"][1]
    keep = w1.view(torch.int32) != so.SENTINEL_BITS
    assert float((w1[keep] != w2[keep]).double().mean()) > 0.9


@pytest.mark.parametrize("fault", ["halves_swapped", "one_minus_dropped"])
def test_faulty_glu_bwd_misses_the_bound_tenfold(fault):
    worst = 0.0
    for c in so.GLU_CASES:
        u, _, dg = so.glu_inputs(c)
        ref, scale = so.glu_bwd(u.double(), dg.double(), c.N)
        bad, _ = so.glu_bwd(u.double(), dg.double(), c.N, fault=fault)
        assert so.ratio((ref.float().double() - ref).abs(), so.glu_bound(scale)) <= 1.0 / 16      # float32 rounding of the truth fits easily
        worst = max(worst, so.ratio((bad - ref).abs(), so.glu_bound(scale)))
    assert worst >= 10.0


def test_biased_std_misses_the_prep_bound_tenfold():
    for c in so.PREP_CASES:
        x = so.prep_inputs(c).double()
        (ref, std), (bad, bstd) = so.prep(x, c.VL, so.PREP_FLOOR), so.prep(x, c.VL, so.PREP_FLOOR, fault="biased_std")
        b_out, b_std = so.prep_bounds(ref, std)
        assert so.ratio((bad - ref).abs()[:, :c.T], b_out[:, :c.T]) >= 10.0 and so.ratio((bstd - std).abs(), b_std) >= 10.0, c.name
        assert so.ratio((ref.float().double() - ref).abs(), b_out) <= 0.25


def test_symmetric_taps_would_have_hidden_the_flipped_walk():
    """With the real sinc taps (symmetric to 1.5e-8) a flipped tap walk, and the mirrored walk with the offsets 55 and 56 exchanged
    (x[i + 56 - k] for x[i + k - 55]: the same thing), stay within 1e-6 of the reference: an aggregate 1e-6 tolerance cannot see them."""
    assert float((REAL_TAPS - REAL_TAPS.flip(0)).abs().max()) < 2e-8
    x = torch.randn(3, 1001, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    rel = lambda a, b: float((a - b).abs().sum() / b.abs().sum())
    assert rel(so.upsample2(x, REAL_TAPS, fault="taps_flipped"), so.upsample2(x, REAL_TAPS)) < 1e-6
    assert rel(so.downsample2(x, REAL_TAPS, fault="taps_flipped"), so.downsample2(x, REAL_TAPS)) < 1e-6
    # the mirrored walk: sum_k x[i + 56 - k] ker[k], written out
    xp = F.pad(x, (56, 56))
    mirrored = torch.stack([xp[:, i + 1:i + 113].flip(1) @ REAL_TAPS for i in range(0, 1001, 97)], dim=1)
    assert float((mirrored - so.upsample2(x, REAL_TAPS)[:, 1::2][:, ::97]).abs().max()) < 1e-6
    # a plain exchange of the offsets with the walk kept (the "tap_offset" variant) is a one-sample delay: no symmetry hides that
    assert rel(so.upsample2(x, REAL_TAPS, fault="tap_offset"), so.upsample2(x, REAL_TAPS)) > 0.1
