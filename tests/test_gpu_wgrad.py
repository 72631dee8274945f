"""GPU: every instantiation of the UNet weight-gradient family (mfpa_wgrad_mfma), pinned bit for bit at the block
level through ops_train.wgrad_mfma.

Every operand value is an integer in [-3, 3] (the in-affine is scale 1 and an integer shift, so ReLU(x + shift) is an integer in [0, 5]).
Such values are exact in bfloat16 -- the bf16x3 split has a zero low half -- and every product and partial sum is an integer below 2^24,
so the float32 result is exact whatever the accumulation or atomic order: the assertion is torch.equal against a float64 CPU reference
(conv2d_weight for the 3 x 3 layers, autograd through conv_transpose2d for the transposed ones), no tolerance.  _reference() checks that
the reference itself is integer-valued and below 2^24 before anything is compared with it.

Shapes: W = 15 selects the 8 x 16 patches (PW 16), W = 33 the 4 x 32 ones with a ragged second tile column; H = 9 is ragged against patch
heights 2, 4 and 8.  The expected grids assume 256 CUs (the bf16-operand 3 x 3 kernel sizes its patch split by the CU count)."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (id, mode, precision, bf16 operands, B, H, W, C0, C1, Cout, in-affine)           kernel <MODE, PW, PLAIN, BF16IN, CI128> or <PW, COT>, grid (x, y, z)
CASES = [
    # ---- fp32 operands, precisions 0 / 1 / 2: one (co, ci) tile; two sources with the in-affine; the transposed convolution
    ("p0-m0-w15", 0, 0, False, 2, 9, 15, 64, 0, 64, False),                       # wgrad_mfma_kernel<0>, (1, 1, 10)
    ("p0-m0-w33", 0, 0, False, 2, 9, 33, 64, 0, 64, False),                       # wgrad_mfma_kernel<0>, (1, 1, 20)
    ("p0-m0-w15-x1-affine", 0, 0, False, 2, 9, 15, 64, 64, 128, True),            # wgrad_mfma_kernel<0>, (2, 2, 10)
    ("p0-m0-w33-x1-affine", 0, 0, False, 2, 9, 33, 64, 64, 128, True),            # wgrad_mfma_kernel<0>, (2, 2, 20)
    ("p0-m1-w15", 1, 0, False, 2, 9, 15, 128, 0, 64, False),                      # wgrad_mfma_kernel<1>, (1, 2, 10)
    ("p0-m1-w33", 1, 0, False, 2, 9, 33, 128, 0, 64, False),                      # wgrad_mfma_kernel<1>, (1, 2, 20)
    ("p1-m0-w15", 0, 1, False, 2, 9, 15, 64, 0, 64, False),                       # wgrad_bf16x3_kernel<0, 16, false>, (1, 1, 4)
    ("p1-m0-w33", 0, 1, False, 2, 9, 33, 64, 0, 64, False),                       # wgrad_bf16x3_kernel<0, 32, false>, (1, 1, 12)
    ("p1-m0-w15-x1-affine", 0, 1, False, 2, 9, 15, 64, 64, 128, True),            # wgrad_bf16x3_kernel<0, 16, false>, (2, 2, 4): 16 workgroups, XCD order
    ("p1-m0-w33-x1-affine", 0, 1, False, 2, 9, 33, 64, 64, 128, True),            # wgrad_bf16x3_kernel<0, 32, false>, (2, 2, 12): 48 workgroups, XCD order
    ("p1-m1-w15", 1, 1, False, 2, 9, 15, 128, 0, 64, False),                      # wgrad_bf16x3_kernel<1, 16, false>, (1, 2, 4): XCD order
    ("p1-m1-w33", 1, 1, False, 2, 9, 33, 128, 0, 64, False),                      # wgrad_bf16x3_kernel<1, 32, false>, (1, 2, 12): XCD order
    ("p2-m0-w15", 0, 2, False, 2, 9, 15, 64, 0, 64, False),                       # wgrad_bf16x3_kernel<0, 16, true>, (1, 1, 4)
    ("p2-m0-w33", 0, 2, False, 2, 9, 33, 64, 0, 64, False),                       # wgrad_bf16x3_kernel<0, 32, true>, (1, 1, 12)
    ("p2-m0-w15-x1-affine", 0, 2, False, 2, 9, 15, 64, 64, 128, True),            # wgrad_bf16x3_kernel<0, 16, true>, (2, 2, 4): XCD order
    ("p2-m0-w33-x1-affine", 0, 2, False, 2, 9, 33, 64, 64, 128, True),            # wgrad_bf16x3_kernel<0, 32, true>, (2, 2, 12): XCD order
    ("p2-m1-w15", 1, 2, False, 2, 9, 15, 128, 0, 64, False),                      # wgrad_bf16x3_kernel<1, 16, true>, (1, 2, 4): XCD order
    ("p2-m1-w33", 1, 2, False, 2, 9, 33, 128, 0, 64, False),                      # wgrad_bf16x3_kernel<1, 32, true>, (1, 2, 12): XCD order
    # ---- bf16 operands (the wrapper turns precision 2 into 3), 3 x 3: 64- and 128-channel output tiles at both patch widths
    ("p3-m0-w15-co64", 0, 2, True, 2, 9, 15, 64, 0, 64, False),                   # wgrad_bf16_kernel<16, 2>, (1, 1, 4)
    ("p3-m0-w33-co64", 0, 2, True, 2, 9, 33, 64, 0, 64, False),                   # wgrad_bf16_kernel<32, 2>, (1, 1, 12)
    ("p3-m0-w15-co128", 0, 2, True, 2, 9, 15, 64, 0, 128, False),                 # wgrad_bf16_kernel<16, 4>, (1, 1, 4)
    ("p3-m0-w33-co128", 0, 2, True, 2, 9, 33, 64, 0, 128, False),                 # wgrad_bf16_kernel<32, 4>, (1, 1, 12)
    ("p3-m0-w33-x1", 0, 2, True, 2, 9, 33, 64, 64, 128, False),                   # wgrad_bf16_kernel<32, 4>, (1, 2, 12): bf16 second source; 24 workgroups, XCD order
    ("p3-m0-w33-ci192", 0, 2, True, 2, 9, 33, 192, 0, 64, False),                 # wgrad_bf16_kernel<32, 2>, (1, 3, 12): 36 workgroups, plain order
    # ---- bf16 operands, transposed: the 64 x 64 form (C0 = 64 * odd) and the 64 x 128 one (CI128)
    ("p3-m1-w15-ci64", 1, 2, True, 2, 9, 15, 64, 0, 64, False),                   # wgrad_bf16x3_kernel<1, 16, true, true, false>, (1, 1, 4)
    ("p3-m1-w33-ci64", 1, 2, True, 2, 9, 33, 64, 0, 64, False),                   # wgrad_bf16x3_kernel<1, 32, true, true, false>, (1, 1, 12)
    ("p3-m1-w33-ci64-co128", 1, 2, True, 2, 9, 33, 64, 0, 128, False),            # wgrad_bf16x3_kernel<1, 32, true, true, false>, (2, 1, 12): 24 workgroups, XCD order
    ("p3-m1-w15-ci128", 1, 2, True, 2, 9, 15, 128, 0, 64, False),                 # wgrad_bf16x3_kernel<1, 16, true, true, true>, (1, 1, 4)
    ("p3-m1-w33-ci128", 1, 2, True, 2, 9, 33, 128, 0, 64, False),                 # wgrad_bf16x3_kernel<1, 32, true, true, true>, (1, 1, 12)
    # ---- a workgroup walks more than one patch (prefetch, double buffer, grid-stride loop): 64 tiles of 512 x 512 channels
    ("p0-m0-walk", 0, 0, False, 4, 9, 33, 512, 0, 512, False),                    # wgrad_mfma_kernel<0>, (8, 8, 32): 40 patches
    ("p1-m0-walk", 0, 1, False, 4, 9, 33, 512, 0, 512, False),                    # wgrad_bf16x3_kernel<0, 32, false>, (8, 8, 16): 24 patches
    ("p2-m0-walk", 0, 2, False, 4, 9, 33, 512, 0, 512, False),                    # wgrad_bf16x3_kernel<0, 32, true>, (8, 8, 16): 24 patches
    ("p3-m0-walk", 0, 2, True, 4, 9, 33, 512, 0, 512, False),                     # wgrad_bf16_kernel<32, 4>, (4, 8, 8): 24 patches, three per workgroup
    ("p3-m0-walk-co64", 0, 2, True, 6, 9, 33, 512, 0, 64, False),                 # wgrad_bf16_kernel<32, 2>, (1, 8, 32): 36 patches
    # transposed, 512 -> 256.  With 4 clips the patch split is clamped to the patch count (40 / 24 / 24 patches against 64 / 32 / 64) and
    # every workgroup has one patch; 12 clips (120 / 72 / 72 patches) are the smallest batch at which all four forms walk
    ("p0-m1-b4", 1, 0, False, 4, 9, 33, 512, 0, 256, False),                      # wgrad_mfma_kernel<1>, (4, 8, 40)
    ("p1-m1-b4", 1, 1, False, 4, 9, 33, 512, 0, 256, False),                      # wgrad_bf16x3_kernel<1, 32, false>, (4, 8, 24)
    ("p2-m1-b4", 1, 2, False, 4, 9, 33, 512, 0, 256, False),                      # wgrad_bf16x3_kernel<1, 32, true>, (4, 8, 24)
    ("p3-m1-b4", 1, 2, True, 4, 9, 33, 512, 0, 256, False),                       # wgrad_bf16x3_kernel<1, 32, true, true, true>, (4, 4, 24)
    ("p0-m1-walk", 1, 0, False, 12, 9, 33, 512, 0, 256, False),                   # wgrad_mfma_kernel<1>, (4, 8, 64): 120 patches
    ("p1-m1-walk", 1, 1, False, 12, 9, 33, 512, 0, 256, False),                   # wgrad_bf16x3_kernel<1, 32, false>, (4, 8, 32): 72 patches
    ("p2-m1-walk", 1, 2, False, 12, 9, 33, 512, 0, 256, False),                   # wgrad_bf16x3_kernel<1, 32, true>, (4, 8, 32): 72 patches
    ("p3-m1-walk", 1, 2, True, 12, 9, 33, 512, 0, 256, False),                    # wgrad_bf16x3_kernel<1, 32, true, true, true>, (4, 4, 64): 72 patches
    ("p3-m1-walk-ci192", 1, 2, True, 60, 9, 33, 192, 0, 64, False),               # wgrad_bf16x3_kernel<1, 32, true, true, false>, (1, 3, 342): 360 patches, plain order
]


def _ints(g, *shape):
    return torch.randint(-3, 4, shape, generator=g).double()


@functools.lru_cache(maxsize=None)
def _reference(mode, B, H, W, C0, C1, Cout, affine):
    """NCHW float64 operands and the packed float32 weight gradient [taps][Cout][C0 + C1]; shared by the precisions of one shape."""
    from musicfpaugment_amd import ops_unet as K
    g = torch.Generator().manual_seed(1000 * mode + 100 * B + W + C0 + C1 + Cout)
    x0 = _ints(g, B, C0, H, W)
    shift = torch.randint(-2, 3, (C0,), generator=g).double() if affine else None
    a0 = F.relu(x0 + shift[None, :, None, None]) if affine else x0
    if mode == 0:
        x1 = _ints(g, B, C1, H - 1, W - 1) if C1 else None                  # the second source is zero-padded to (H, W)
        dz = _ints(g, B, Cout, H, W)
        xin = a0 if x1 is None else torch.cat([a0, F.pad(x1, [0, 1, 0, 1])], dim=1)
        pack, full = K.pack_conv3x3, torch.nn.grad.conv2d_weight(xin, (Cout, C0 + C1, 3, 3), dz, padding=1)
    else:
        x1 = None
        dz = _ints(g, B, Cout, 2 * H, 2 * W)
        w = torch.zeros(C0, Cout, 2, 2, dtype=torch.float64, requires_grad=True)
        F.conv_transpose2d(a0, w, stride=2).backward(dz)
        pack, full = K.pack_convT2x2, w.grad
    # the reference itself is exact: integers below 2^24, and so is every partial sum (at most 3 * 5 * B * H * W in magnitude)
    assert full.dtype == torch.float64 and torch.equal(full, full.round())
    assert float(full.abs().max()) < 2 ** 24 and 15 * B * H * W < 2 ** 24
    return x0, shift, x1, dz, pack(full)                                     # float32: exact for such values


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_wgrad_exact_on_small_integers(case, monkeypatch):
    from musicfpaugment_amd import ops_train as T
    _, mode, precision, bf16, B, H, W, C0, C1, Cout, affine = case
    if not bf16:      # float32 operands stay float32 at every channel count: the wrapper would cast them (precision 3) from 128 channels up
        monkeypatch.setattr(T, "BF16_WGRAD_MIN_CH", 1 << 30)
    x0, shift, x1, dz, ref = _reference(mode, B, H, W, C0, C1, Cout, affine)
    nhwc = lambda t: None if t is None else t.float().permute(0, 2, 3, 1).contiguous().cuda()
    x0d, x1d, dzd = nhwc(x0), nhwc(x1), nhwc(dz)
    st = None
    if affine:
        st = T.Stats(C0, "cuda")
        st.scale.fill_(1.0)
        st.shift.copy_(shift.float())
    copies = {}
    if bf16:                                                                 # these copies are what makes the wrapper choose precision 3
        assert st is None
        copies = dict(dz_bf16=dzd.bfloat16(), x0_bf16=x0d.bfloat16(), x1_bf16=None if x1d is None else x1d.bfloat16())
        assert torch.equal(copies["dz_bf16"].float(), dzd) and torch.equal(copies["x0_bf16"].float(), x0d)
    dw = torch.zeros(ref.shape, dtype=torch.float32, device="cuda")
    T.wgrad_mfma(dzd, x0d, dw, Cout, mode=mode, in_affine=st, x1=x1d, precision=precision, **copies)
    torch.cuda.synchronize()
    got = dw.cpu()
    bad = got != ref
    assert torch.equal(got, ref), (case[0], int(bad.sum()), float((got - ref).abs().max()), bad.nonzero()[:4].tolist())
