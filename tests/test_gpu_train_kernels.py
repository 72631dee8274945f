"""The non-convolution kernels of the UNet training step (csrc/unet_train.hip) over the C ABI, entry point by entry point.

The engine's whole-step tests (test_gpu_train.py) run these kernels at one image size only; nine entry points were named by no test.
This file pins them:

  * four identities the file's own comments claim and that hold by construction -- a fused entry point is the same kernels as its
    parts, launched in one call -- asserted with torch.equal on every output;
  * a bfloat16 z against the same call on z.float() (the widening is exact);
  * the fused pool + BatchNorm backward against its two-call form;
  * mfpa_bn_relu_pool, mfpa_outconv_fwd and mfpa_colsum against float64 torch restatements, each tolerance taken from the arithmetic type;
  * the argument contract of every entry point.

Where two DIFFERENT kernels compute the same formula (the 8-wide and the 4-wide apply pass; the pool kernel's own apply), the compiler may
contract their multiply-adds differently.  Those differences were measured on the library of the commit before the shared helpers
(csrc/unet_train.hip at f3dc153), over all cases of the test, and decide the assertion: zero -> equality, otherwise twice the figure.
Measured (every such test prints its figure with -s):

  apply pass, bfloat16 z (8-wide) against z.float() (4-wide):  0 float32 ulps, no bf16 dz differs, in all 14 cases -> equality
  fused pool backward's dz against add_sums + from_part:       0 bf16 ulps, no element differs, in all 64 cases -> equality
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

EPS, MOM = 1e-5, 0.1
DROPS = {"nodrop": (0, 0, 1.0), "drop": (7, int(0.3 * 2 ** 32), 1.0 / 0.7)}
SHAPES = [(8, 1), (8, 3219), (64, 1), (64, 3219), (1024, 1), (1024, 3219), (1024, 8601)]      # (C, npix); 8601 pixels cap chan_reduce's grid
POOLS = [(1, 2, 2), (3, 17, 13), (2, 9, 8), (2, 8, 11)]
U32, U16 = 2.0 ** -24, 2.0 ** -8            # unit roundoff of float32 and of bfloat16

# largest difference between two kernels of one formula, in float32 ulps of max |dz| (apply pass) / in bfloat16 ulps of max |dz| (pool):
# the bound is twice the figure measured on the earlier library (0: equality)
APPLY_BF16Z_ULPS = 0.0
POOL_FUSED_DZ_ULPS = 0.0


def _dev():
    return torch.device("cuda:0")


def call(name, *a):
    from musicfpaugment_amd._lib import lib, ptr, stream
    return getattr(lib(), name)(*[ptr(x) if isinstance(x, torch.Tensor) else (0 if x is None else x) for x in a], stream())


def ok(name, *a):
    rc = call(name, *a)
    assert rc == 0, (name, rc)


def rnd(seed, *shape, dtype=torch.float32):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=dtype).to(_dev())


def zeros(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype, device=_dev())


@functools.lru_cache(maxsize=None)
def layer(C, npix):
    """One layer's tensors, made once and shared (no test writes into them): z as float32 and bfloat16, BatchNorm constants, gradient."""
    z = rnd(C + npix, npix, C)
    gamma, beta = 1 + 0.1 * rnd(1, C), 0.1 * rnd(2, C)
    mean = z.mean(0)
    invstd = 1 / torch.sqrt(z.var(0, unbiased=False) + EPS)
    scale = gamma * invstd
    return dict(z=z, z16=z.bfloat16(), gamma=gamma, beta=beta, mean=mean, invstd=invstd, scale=scale, shift=beta - mean * scale,
                dy=rnd(C + npix + 3, npix, C), ws=torch.zeros(1024 * (2 * C + 2), dtype=torch.float64, device=_dev()))


def stats_out(C):
    return [zeros(C), zeros(C), zeros(C), zeros(C), 0.5 + zeros(C), 2 + zeros(C)]     # mean, invstd, scale, shift, running mean / var


def bwd_out(C):
    return [zeros(C), zeros(C), zeros(3, C)]                                          # dgamma, dbeta, coef


def same(a, b, what):
    for k, (x, y) in enumerate(zip(a, b)):
        if x is None and y is None:
            continue
        assert torch.equal(x, y), f"{what}: output {k} differs (max |d| {float((x.double() - y.double()).abs().max())})"


def keep_mask(seed, thresh, scale, n):
    """csrc/mfpa_common.h::mfpa_keep over flat element indices 0 .. n-1 -> multiplicative float64 mask"""
    from musicfpaugment_amd import synth
    if thresh == 0:
        return torch.ones(n, dtype=torch.float64)
    idx = np.arange(n, dtype=np.uint64)
    lo, hi = (idx & np.uint64(0xFFFFFFFF)).astype(np.uint32), (idx >> np.uint64(32)).astype(np.uint32)
    with np.errstate(over="ignore"):
        h = synth._mix32(synth._mix32(lo + np.uint32(seed)) ^ (hi * np.uint32(0x7F4A7C15) + np.uint32(seed)))
    return torch.from_numpy((h >= np.uint32(thresh)).astype(np.float64) * float(np.float32(scale)))


def ulps_of_max(a, b, unit):
    """max |a - b| in units of the spacing (unit = 2 * unit roundoff) of the format at max |b|"""
    a, b = a.double(), b.double()
    top = float(b.abs().max())
    if top == 0.0:
        return 0.0 if float((a - b).abs().max()) == 0.0 else float("inf")
    return float((a - b).abs().max()) / (2.0 ** np.floor(np.log2(top)) * unit)


# ------------------------------------------------------------------ identities that hold by construction
@gpu
@pytest.mark.parametrize("zk", ["z", "z16"])
@pytest.mark.parametrize("C,npix", SHAPES)
def test_bn_stats_is_sums_plus_finish(C, npix, zk):
    L = layer(C, npix)
    a, b, sums = stats_out(C), stats_out(C), zeros(C, 2, dtype=torch.float64)
    ok("mfpa_bn_stats", L[zk], npix, C, L["gamma"], L["beta"], EPS, MOM, *a, L["ws"], int(zk == "z16"))
    ok("mfpa_bn_stats_sums", L[zk], npix, C, sums, L["ws"], int(zk == "z16"))
    ok("mfpa_bn_stats_finish", sums, float(npix), C, L["gamma"], L["beta"], EPS, MOM, *b)
    same(a, b, "mfpa_bn_stats")
    assert not torch.equal(a[4], 0.5 + zeros(C)) and not torch.equal(a[5], 2 + zeros(C))          # the running statistics moved


@gpu
@pytest.mark.parametrize("rows", [1, 37, 9000])
@pytest.mark.parametrize("C", [8, 64, 1024])
def test_conv_stats_bn_finish_is_reduce_plus_finish(C, rows):
    part = rnd(C + rows, rows, 2, C)
    part[:, 1] = part[:, 0] ** 2 + part[:, 1] ** 2
    ws, gamma, beta = torch.zeros(1024 * 2 * C, dtype=torch.float64, device=_dev()), 1 + 0.1 * rnd(1, C), 0.1 * rnd(2, C)
    a, b, sums = stats_out(C), stats_out(C), zeros(C, 2, dtype=torch.float64)
    ok("mfpa_conv_stats_bn_finish", part, rows, C, 50.0 * rows, gamma, beta, EPS, MOM, *a, ws)
    ok("mfpa_conv_stats_reduce", part, rows, C, sums, ws)
    ok("mfpa_bn_stats_finish", sums, 50.0 * rows, C, gamma, beta, EPS, MOM, *b)
    same(a, b, "mfpa_conv_stats_bn_finish")
    torch.testing.assert_close(sums[:, 0], part[:, 0].double().sum(0), rtol=1e-12, atol=1e-7)       # and the sums are the rows' sums


@gpu
@pytest.mark.parametrize("dk", list(DROPS))
@pytest.mark.parametrize("zk", ["z", "z16"])
@pytest.mark.parametrize("C,npix", SHAPES)
def test_bn_relu_bwd_is_sums_plus_finish(C, npix, zk, dk):
    """local = global sums and count = npix: the single-GPU backward, in one call and in two"""
    L, z16, drop = layer(C, npix), int(zk == "z16"), DROPS[dk]
    bn = (L["gamma"], L["scale"], L["shift"], L["mean"], L["invstd"])
    for write_f32 in (1, 0):
        dy_a, dy_b, dz_a, dz_b = L["dy"].clone(), L["dy"].clone(), zeros(npix, C, dtype=torch.bfloat16), zeros(npix, C, dtype=torch.bfloat16)
        a, b, sums = bwd_out(C), bwd_out(C), zeros(C, 2, dtype=torch.float64)
        ok("mfpa_bn_relu_bwd", dy_a, L[zk], npix, C, *bn, *a, L["ws"], *drop, dz_a, write_f32, z16)
        ok("mfpa_bn_relu_bwd_sums", dy_b, L[zk], npix, C, *bn[1:], sums, L["ws"], *drop, z16)
        ok("mfpa_bn_relu_bwd_finish", dy_b, L[zk], npix, C, *bn, sums, sums, float(npix), *b, *drop, dz_b, write_f32, z16, 0)
        same(a + [dy_a, dz_a], b + [dy_b, dz_b], f"mfpa_bn_relu_bwd write_f32={write_f32}")
        assert torch.equal(dy_a, L["dy"]) == (write_f32 == 0)                                     # dy is left alone exactly when asked


@gpu
@pytest.mark.parametrize("dk", list(DROPS))
@pytest.mark.parametrize("zk", ["z", "z16"])
@pytest.mark.parametrize("C,npix", SHAPES)
def test_bn_relu_bwd_from_part_is_reduce_plus_finish(C, npix, zk, dk):
    L, z16, drop = layer(C, npix), int(zk == "z16"), DROPS[dk]
    bn = (L["gamma"], L["scale"], L["shift"], L["mean"], L["invstd"])
    part = rnd(C + 5, 7, 2, C)
    for dy16, write_f32 in ((0, 1), (0, 0), (1, 0)):
        src = L["dy"].bfloat16() if dy16 else L["dy"]
        dy_a, dy_b, dz_a, dz_b = src.clone(), src.clone(), zeros(npix, C, dtype=torch.bfloat16), zeros(npix, C, dtype=torch.bfloat16)
        a, b, sums = bwd_out(C), bwd_out(C), zeros(C, 2, dtype=torch.float64)
        ok("mfpa_bn_relu_bwd_from_part", dy_a, L[zk], npix, C, *bn, part, 7, *a, L["ws"], *drop, dz_a, write_f32, z16, dy16)
        ok("mfpa_conv_stats_reduce", part, 7, C, sums, L["ws"])
        ok("mfpa_bn_relu_bwd_finish", dy_b, L[zk], npix, C, *bn, sums, sums, float(npix), *b, *drop, dz_b, write_f32, z16, dy16)
        same(a + [dy_a, dz_a], b + [dy_b, dz_b], f"mfpa_bn_relu_bwd_from_part dy16={dy16} write_f32={write_f32}")
        assert float(dz_a.float().abs().max()) > 0


# ------------------------------------------------------------------ a bfloat16 z against the same call on z.float()
@gpu
@pytest.mark.parametrize("C,npix", SHAPES)
def test_sums_of_a_bf16_z_equal_those_of_its_widening(C, npix):
    """the same kernel reads both: equality"""
    L = layer(C, npix)
    zw = L["z16"].float()
    a, b = zeros(C, 2, dtype=torch.float64), zeros(C, 2, dtype=torch.float64)
    ok("mfpa_bn_stats_sums", L["z16"], npix, C, a, L["ws"], 1)
    ok("mfpa_bn_stats_sums", zw, npix, C, b, L["ws"], 0)
    same([a], [b], "mfpa_bn_stats_sums")
    torch.testing.assert_close(a[:, 0], zw.double().sum(0), rtol=1e-12, atol=1e-7)
    for drop in DROPS.values():
        ok("mfpa_bn_relu_bwd_sums", L["dy"], L["z16"], npix, C, L["scale"], L["shift"], L["mean"], L["invstd"], a, L["ws"], *drop, 1)
        ok("mfpa_bn_relu_bwd_sums", L["dy"], zw, npix, C, L["scale"], L["shift"], L["mean"], L["invstd"], b, L["ws"], *drop, 0)
        same([a], [b], "mfpa_bn_relu_bwd_sums")


@gpu
@pytest.mark.parametrize("dk", list(DROPS))
@pytest.mark.parametrize("C,npix", SHAPES)
def test_apply_pass_of_a_bf16_z_against_its_widening(C, npix, dk):
    """bn_bwd_apply8_kernel (bfloat16 z, 8 channels per thread) against bn_bwd_apply_kernel on z.float(): one formula in two kernels.
    Measured on the earlier library: see the module docstring; the bound is twice that (0: equality)."""
    L, drop = layer(C, npix), DROPS[dk]
    bn = (L["gamma"], L["scale"], L["shift"], L["mean"], L["invstd"])
    sums = rnd(C + 9, C, 2, dtype=torch.float64)
    dy_a, dy_b, dz_a, dz_b, a, b = L["dy"].clone(), L["dy"].clone(), zeros(npix, C, dtype=torch.bfloat16), zeros(npix, C, dtype=torch.bfloat16), bwd_out(C), bwd_out(C)
    ok("mfpa_bn_relu_bwd_finish", dy_a, L["z16"], npix, C, *bn, sums, sums, float(npix), *a, *drop, dz_a, 1, 1, 0)
    ok("mfpa_bn_relu_bwd_finish", dy_b, L["z16"].float(), npix, C, *bn, sums, sums, float(npix), *b, *drop, dz_b, 1, 0, 0)
    same(a, b, "coefficients")
    d = ulps_of_max(dy_a, dy_b, 2 * U32)
    print(f"apply pass bf16 z vs widened, C={C} npix={npix} {dk}: {d:.3f} float32 ulps of max |dz|, "
          f"{int((dz_a != dz_b).sum())} bf16 dz differ of {dz_a.numel()}")
    if APPLY_BF16Z_ULPS == 0.0:
        same([dy_a, dz_a], [dy_b, dz_b], "dz")
    else:
        assert d <= 2 * APPLY_BF16Z_ULPS


# ------------------------------------------------------------------ the fused pool + BatchNorm backward against its two calls
@gpu
@pytest.mark.parametrize("dk", list(DROPS))
@pytest.mark.parametrize("dy16", [0, 1])
@pytest.mark.parametrize("C", [64, 512])
@pytest.mark.parametrize("B,H,W", POOLS)
def test_fused_pool_backward_against_add_sums_plus_from_part(B, H, W, C, dy16, dk):
    npix, drop = B * H * W, DROPS[dk]
    L = layer(C, npix)
    bn = (L["gamma"], L["scale"], L["shift"], L["mean"], L["invstd"])
    dp = rnd(C + H, B, H // 2, W // 2, C)
    skip = L["dy"].bfloat16() if dy16 else L["dy"].clone()
    for zk in ("z", "z16"):
        z16 = int(zk == "z16")
        part_a, part_b, dz_a, dz_b, a, b = zeros(B * (H // 2), 2, C), zeros(B * (H // 2), 2, C), zeros(npix, C, dtype=torch.bfloat16), zeros(npix, C, dtype=torch.bfloat16), bwd_out(C), bwd_out(C)
        before = skip.clone()
        ok("mfpa_maxpool2_bwd_bn_relu_bwd", L[zk], B, H, W, C, *bn, dp, skip, dy16, *drop, part_a, *a, L["ws"], dz_a, z16)
        assert torch.equal(skip, before)                                                          # the skip gradient is only read
        dy = skip.float()                                                                         # (the two-call form widens a bfloat16 one first)
        ok("mfpa_maxpool2_bwd_add_sums", L[zk], B, H, W, C, *bn[1:], dp, dy, *drop, part_b, z16)
        ok("mfpa_bn_relu_bwd_from_part", dy, L[zk], npix, C, *bn, part_b, B * (H // 2), *b, L["ws"], *drop, dz_b, 0, z16, 0)
        same([part_a] + a, [part_b] + b, "part, dgamma, dbeta, coef")
        d = ulps_of_max(dz_a, dz_b, 2 * U16)
        print(f"fused pool backward, {B}x{H}x{W} C={C} dy16={dy16} {dk} {zk}: {d:.3f} bf16 ulps of max |dz|, {int((dz_a != dz_b).sum())} differ of {dz_a.numel()}")
        if POOL_FUSED_DZ_ULPS == 0.0:
            same([dz_a], [dz_b], "dz")
        else:
            assert d <= 2 * POOL_FUSED_DZ_ULPS
        assert float(dz_a.float().abs().max()) > 0


# ------------------------------------------------------------------ float64 restatements
@gpu
@pytest.mark.parametrize("dk", list(DROPS))
@pytest.mark.parametrize("C", [8, 64])
@pytest.mark.parametrize("B,H,W", [(3, 17, 13), (2, 9, 8), (2, 8, 11)])
def test_bn_relu_pool_against_float64(B, H, W, C, dk):
    """p = maxpool2(dropout(relu(z*scale+shift))), floor.  The selection is exact; the value carries the float32 affine (two roundings of
    |z*scale| + |shift|: 2 * 2^-24 of it), with dropout one more of the scaled value, and as bfloat16 one rounding to 8 bits."""
    npix, (seed, thr, ds) = B * H * W, DROPS[dk]
    L = layer(C, npix)
    for zk in ("z", "z16"):
        zz = L[zk].double()
        pre = zz * L["scale"].double() + L["shift"].double()
        y = torch.relu(pre) * keep_mask(seed, thr, ds, npix * C).to(_dev()).view(npix, C)
        want = torch.nn.functional.max_pool2d(y.view(B, H, W, C).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
        mag = float(((zz * L["scale"].double()).abs() + L["shift"].double().abs()).max()) * float(np.float32(ds))
        tol32 = 2 * U32 * mag + (U32 * float(want.max()) if thr else 0.0)
        for p16 in (0, 1):
            p = zeros(B, H // 2, W // 2, C, dtype=torch.bfloat16 if p16 else torch.float32)
            ok("mfpa_bn_relu_pool", L[zk], B, H, W, C, L["scale"], L["shift"], p, seed, thr, ds, int(zk == "z16"), p16)
            err = (p.double() - want).abs()
            bound = tol32 + (U16 * (want.abs() + tol32) if p16 else 0.0)
            print(f"bn_relu_pool {B}x{H}x{W} C={C} {dk} {zk} p16={p16}: max err {float(err.max()):.3e}, float32 allowance {tol32:.3e}")
            assert bool((err <= bound).all())
            assert float(p.float().max()) > 0


@gpu
@pytest.mark.parametrize("C,npix", [(4, 1), (4, 3219), (64, 1), (64, 3219), (256, 1), (256, 3219)])
def test_outconv_fwd_against_float64(C, npix):
    """pred[p] = sum_c relu(z*scale+shift)[c] * w[c] + bias: float32 products, four per lane and then C/4 lanes, summed in float32 -- at most
    C additions deep and one for the bias; each term carries the float32 affine's two roundings."""
    L = layer(C, npix)
    wb = rnd(C + 11, C + 1)
    for zk in ("z", "z16"):
        zz = L[zk].double()
        y = torch.relu(zz * L["scale"].double() + L["shift"].double())
        want = (y * wb[:C].double()).sum(1) + wb[C].double()
        aff = ((zz * L["scale"].double()).abs() + L["shift"].double().abs()) * wb[:C].double().abs()
        tol = U32 * ((C + 2) * (y * wb[:C].double()).abs().sum(1) + 2 * aff.sum(1) + want.abs() + float(wb[C].abs()))
        pred = zeros(npix)
        ok("mfpa_outconv_fwd", L[zk], npix, C, L["scale"], L["shift"], wb, wb[C:], pred, int(zk == "z16"))
        err = (pred.double() - want).abs()
        print(f"outconv_fwd C={C} npix={npix} {zk}: max err / allowance {float((err / tol).max()):.3f}")
        assert bool((err <= tol).all())


@gpu
@pytest.mark.parametrize("C,npix", SHAPES + [(2048, 3219)])
def test_colsum_against_float64(C, npix):
    """float64 sums (their own error is 2^-53 per addition) rounded once to float32"""
    L = layer(C, npix) if C <= 1024 else dict(dy=rnd(5, npix, C), ws=torch.zeros(1024 * C, dtype=torch.float64, device=_dev()))
    out = zeros(C)
    ok("mfpa_colsum", L["dy"], npix, C, out, L["ws"])
    want = L["dy"].double().sum(0)
    assert bool(((out.double() - want).abs() <= U32 * want.abs() + npix * 2.0 ** -53 * L["dy"].double().abs().sum(0)).all())


# ------------------------------------------------------------------ the argument contract
def _contract_cases():
    """entry -> (valid arguments at C = 8 and six pixels (1 x 2 x 3), positions of its required pointers, position of C (None: no shape rule on
    C), position of H, needs a power-of-two C).  Every buffer has room for C = 64, so that even a call that should have been refused and
    was not stays inside its buffers."""
    F = lambda: zeros(8192)
    D = lambda: zeros(8192, dtype=torch.float64)
    d0 = (0, 0, 1.0)
    return {
        "mfpa_bn_stats": ([F(), 6, 8, F(), F(), EPS, MOM, F(), F(), F(), F(), F(), F(), D(), 0], [0, 3, 4, 7, 8, 9, 10, 13], 2, None, False),
        "mfpa_bn_relu_bwd": ([F(), F(), 6, 8, F(), F(), F(), F(), F(), F(), F(), F(), D(), *d0, F(), 1, 0], [0, 1, 4, 5, 6, 7, 8, 9, 10, 11, 12], 3, None, True),
        "mfpa_bn_stats_sums": ([F(), 6, 8, D(), D(), 0], [0, 3, 4], 2, None, False),
        "mfpa_conv_stats_reduce": ([F(), 3, 8, D(), D()], [0, 3, 4], 2, None, False),
        "mfpa_conv_stats_bn_finish": ([F(), 3, 8, 6.0, F(), F(), EPS, MOM, F(), F(), F(), F(), F(), F(), D()], [0, 4, 5, 8, 9, 10, 11, 14], 2, None, False),
        "mfpa_bn_relu_bwd_from_part": ([F(), F(), 6, 8, F(), F(), F(), F(), F(), F(), 3, F(), F(), F(), D(), *d0, F(), 1, 0, 0],
                                       [0, 1, 4, 5, 6, 7, 8, 9, 11, 12, 13, 14], 3, None, True),
        "mfpa_bn_stats_finish": ([D(), 6.0, 8, F(), F(), EPS, MOM, F(), F(), F(), F(), F(), F()], [0, 3, 4, 7, 8, 9, 10], None, None, False),
        "mfpa_bn_relu_bwd_sums": ([F(), F(), 6, 8, F(), F(), F(), F(), D(), D(), *d0, 0], [0, 1, 4, 5, 6, 7, 8, 9], 3, None, True),
        "mfpa_bn_relu_bwd_finish": ([F(), F(), 6, 8, F(), F(), F(), F(), F(), D(), D(), 6.0, F(), F(), F(), *d0, F(), 1, 0, 0],
                                    [0, 1, 4, 5, 6, 7, 8, 9, 10, 12, 13, 14], 3, None, True),
        "mfpa_bn_relu_bwd_finish_rank1": ([F(), F(), F(), 6, 8, F(), F(), F(), F(), F(), D(), D(), 6.0, F(), F(), F(), F(), F(), 0],
                                          [0, 1, 2, 5, 6, 7, 8, 9, 10, 11, 13, 14, 15], 4, None, True),
        "mfpa_colsum": ([F(), 6, 8, F(), D()], [0, 3, 4], 2, None, False),
        "mfpa_bn_relu_pool": ([F(), 1, 2, 3, 8, F(), F(), F(), *d0, 0, 0], [0, 5, 6, 7], 4, 2, False),
        "mfpa_maxpool2_bwd_add": ([F(), 1, 2, 3, 8, F(), F(), F(), F(), *d0, 0], [0, 5, 6, 7, 8], 4, 2, False),
        "mfpa_maxpool2_bwd_add_sums": ([F(), 1, 2, 3, 8, F(), F(), F(), F(), F(), F(), *d0, F(), 0], [0, 5, 6, 7, 8, 9, 10, 14], 4, 2, False),
        "mfpa_maxpool2_bwd_bn_relu_bwd": ([F(), 1, 2, 3, 8, F(), F(), F(), F(), F(), F(), F(), 0, *d0, F(), F(), F(), F(), D(), F(), 0],
                                          [0, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 20, 21], 4, 2, True),
        "mfpa_act_to_bf16": ([F(), 48, 8, F(), F(), *d0, F()], [0, 8], 2, None, False),
        "mfpa_outconv_fwd": ([F(), 6, 8, F(), F(), F(), F(), F(), 0], [0, 3, 4, 5, 6, 7], 2, None, True),
        "mfpa_outconv_bwd": ([F(), F(), 6, 8, F(), F(), F(), F(), F(), D(), 0], [0, 1, 4, 5, 6, 7, 8, 9], 3, None, True),
        "mfpa_outconv_bwd_sums": ([F(), F(), 6, 8, F(), F(), F(), F(), F(), F(), D(), F(), 0], [0, 1, 4, 5, 6, 7, 8, 9, 10, 11], 3, None, True),
        "mfpa_l1_loss": ([F(), D(), 6, F(), D(), D()], [0, 1, 4, 5], None, None, False),
        "mfpa_adam_step": ([F(), F(), F(), F(), 6, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0], [0, 1, 2, 3], None, None, False),
    }


@gpu
def test_argument_contract_of_every_entry_point():
    from musicfpaugment_amd._lib import EINVAL, lib
    for name, (args, ptrs, c_at, h_at, pow2) in _contract_cases().items():
        ok(name, *args)                                                                           # the unchanged arguments are accepted

        def refused(at, value, why):
            bad = list(args)
            bad[at] = value
            assert call(name, *bad) == EINVAL, (name, why)
        for at in ptrs:
            refused(at, None, f"null pointer at {at}")
        if c_at is not None:
            refused(c_at, 6, "C = 6")
            if pow2:
                refused(c_at, 48, "C = 48")
        if h_at is not None:
            refused(h_at, 1, "H = 1")
    torch.cuda.synchronize()
    c = _contract_cases()
    # write_f32 = 0 without dz_bf16; a bfloat16 dy with write_f32 = 1
    for name, dz_at, wf_at, dy16_at in (("mfpa_bn_relu_bwd", 16, 17, None), ("mfpa_bn_relu_bwd_from_part", 18, 19, 21), ("mfpa_bn_relu_bwd_finish", 18, 19, 21)):
        bad = list(c[name][0])
        bad[dz_at], bad[wf_at] = None, 0
        assert call(name, *bad) == EINVAL, name
        if dy16_at is not None:
            bad = list(c[name][0])
            bad[dy16_at] = 1
            assert call(name, *bad) == EINVAL, name
    bad = list(c["mfpa_bn_relu_bwd_finish_rank1"][0])
    bad[16] = bad[17] = None                                                                      # neither dz_f32 nor dz_bf16
    assert call("mfpa_bn_relu_bwd_finish_rank1", *bad) == EINVAL
    rows = ctypes.c_int(-1)
    assert lib().mfpa_outconv_bwd_rows(6, 8, ctypes.byref(rows)) == 0 and rows.value == 1
    assert lib().mfpa_outconv_bwd_rows(6, 8, None) == EINVAL
    assert lib().mfpa_outconv_bwd_rows(6, 6, ctypes.byref(rows)) == EINVAL and lib().mfpa_outconv_bwd_rows(6, 48, ctypes.byref(rows)) == EINVAL
    assert call("mfpa_pack_conv_weights", None, 4, 32, 32, 0, 0, 32, 0, zeros(4096)) == EINVAL
    assert call("mfpa_pack_conv_weights", zeros(4096), 4, 32, 32, 0, 0, 32, 0, None) == EINVAL
    assert call("mfpa_pack_conv_weights_batch", None, 1, 1) == EINVAL
    torch.cuda.synchronize()
