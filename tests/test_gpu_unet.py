"""GPU parity: UNet eval forward on float32 MFMA vs the torch-CPU fp32 oracle (tolerance: relative L1 <= 1e-4,
BASELINE.json) and the golden outputs of the real reference module."""
import numpy as np
import pytest
import torch

from musicfpaugment_amd import synth
from musicfpaugment_amd.training.weights import formula_state_dict

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(scope="module")
def net():
    from musicfpaugment_amd.training.unet import UNet
    m = UNet(1, 1, rate=0.05)
    m.load_state_dict(formula_state_dict(0))
    return m.cuda().eval()


def test_state_dict_keys_match_reference_inventory(net):
    from musicfpaugment_amd.training.weights import state_dict_shapes
    sd = net.state_dict()
    shapes = state_dict_shapes()
    assert list(sd.keys()) == list(shapes.keys()) and len(sd) == 118
    assert all(tuple(sd[k].shape) == shapes[k] for k in shapes)


def test_building_blocks_vs_torch(net):
    """Each kernel against the plain torch fp32 op on ragged shapes (odd extents, tile tails)."""
    import torch.nn.functional as F
    from musicfpaugment_amd import ops_unet as K
    from oracle.unet import relative_l1
    g = torch.Generator().manual_seed(1)
    for (B, H, W, C0, C1, Cout) in [(2, 9, 37, 64, 0, 64), (1, 16, 15, 512, 0, 1024), (2, 33, 31, 64, 64, 128),
                                   (1, 5, 70, 32, 0, 128), (1, 13, 16, 96, 32, 64)]:
        x0 = torch.randn(B, C0, H, W, generator=g)
        w = torch.randn(Cout, C0 + C1, 3, 3, generator=g) / np.sqrt(9 * (C0 + C1))
        sc, sh = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.1
        if C1:
            x1 = torch.randn(B, C1, H - 1, W - 1, generator=g)
            xin = torch.cat([x0, F.pad(x1, [0, 1, 0, 1])], dim=1)
        else:
            x1, xin = None, x0
        want = F.relu(F.conv2d(xin, w, padding=1) * sc[None, :, None, None] + sh[None, :, None, None])
        got = K.conv3x3_bn_relu(x0.permute(0, 2, 3, 1).contiguous().cuda(), K.pack_conv3x3(w).cuda(), sc.cuda(), sh.cuda(),
                                x1=None if x1 is None else x1.permute(0, 2, 3, 1).contiguous().cuda())
        assert relative_l1(got.cpu().permute(0, 3, 1, 2), want) < 1e-5, (B, H, W, C0, C1, Cout)
    for (B, H, W, Cin) in [(2, 16, 15, 1024), (1, 7, 33, 128)]:
        x = torch.randn(B, Cin, H, W, generator=g)
        w = torch.randn(Cin, Cin // 2, 2, 2, generator=g) / np.sqrt(Cin)
        bias = torch.randn(Cin // 2, generator=g)
        want = F.conv_transpose2d(x, w, bias, stride=2)
        got = K.convT2x2(x.permute(0, 2, 3, 1).contiguous().cuda(), K.pack_convT2x2(w).cuda(), bias.cuda())
        assert relative_l1(got.cpu().permute(0, 3, 1, 2), want) < 1e-5
    x = torch.randn(2, 64, 257, 251, generator=g)
    got = K.maxpool2(x.permute(0, 2, 3, 1).contiguous().cuda())
    assert torch.equal(got.cpu().permute(0, 3, 1, 2), F.max_pool2d(x, 2))
    wv, b0 = torch.randn(64, generator=g), 0.3
    got = K.conv1x1_out(x.permute(0, 2, 3, 1).contiguous().cuda(), wv.cuda(), b0)
    want = F.conv2d(x, wv.view(1, 64, 1, 1), torch.tensor([b0]))[:, 0]
    assert relative_l1(got.cpu(), want) < 1e-5
    x1c = torch.rand(2, 1, 30, 45, generator=g)
    w1 = torch.randn(64, 1, 3, 3, generator=g)
    sc, sh = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.1
    want = F.relu(F.conv2d(x1c, w1, padding=1) * sc[None, :, None, None] + sh[None, :, None, None])
    got = K.conv3x3_c1_bn_relu(w1.permute(2, 3, 1, 0).reshape(9, 64).contiguous().cuda(), sc.cuda(), sh.cuda(),
                               x32=x1c[:, 0].contiguous().cuda())
    assert relative_l1(got.cpu().permute(0, 3, 1, 2), want) < 1e-5


def test_forward_golden_reference_module(net, golden):
    from oracle.unet import relative_l1
    g = golden("g6_unet_forward")
    y = net(torch.from_numpy(g["x"]).cuda())
    assert y.shape == g["y"].shape and y.dtype == torch.float32
    assert relative_l1(y.cpu(), torch.from_numpy(g["y"])) <= TOL
    from oracle import stft as ostft
    wav8 = synth.batch(1, seed=int(g["seed8"]))
    x8 = torch.from_numpy(ostft.spectrogram(wav8)).float().unsqueeze(1)
    y8 = net(x8.cuda()).cpu()
    assert relative_l1(y8[0, 0, ::4, ::4], torch.from_numpy(g["y8_sub"])) <= TOL
    assert abs(float(y8.double().abs().sum()) - float(g["y8_abs_sum"])) <= TOL * float(g["y8_abs_sum"])


def test_forward_vs_oracle_batch_and_fused_entry(net):
    from oracle import stft as ostft
    from oracle import unet as ou
    from musicfpaugment_amd import ops
    wav = synth.batch(3, seed=900, n=24000)                       # the reference's 3 s training length: 257 x 94
    sd = formula_state_dict(0)
    spec = ostft.spectrogram(wav)
    x = torch.from_numpy(spec).float().unsqueeze(1)
    with torch.no_grad():
        want = ou.forward(x, sd)
    got = net(x.cuda()).cpu()
    assert ou.relative_l1(got, want) <= TOL
    # fused entry: raw float64 |STFT| + maxima straight from the STFT kernel
    mag, cmax = ops.stft_mag(torch.from_numpy(wav).cuda(), torch.float64)
    got2 = net.denoise_spectrogram(mag, cmax, per_clip=False).cpu()
    assert ou.relative_l1(got2.unsqueeze(1), want) <= TOL
    saved_pass = net.max_clips_per_pass
    try:
        net.max_clips_per_pass = 2                                 # sub-batching must not change results
        got3 = net(x.cuda()).cpu()
    finally:
        net.max_clips_per_pass = saved_pass
    assert torch.equal(got3, got)


def test_cpu_inputs_fail_loudly(net):
    from musicfpaugment_amd._lib import MfpaError
    with pytest.raises(MfpaError):
        net(torch.zeros(1, 1, 257, 32))
    with pytest.raises(TypeError):
        net(torch.zeros(1, 1, 257, 32, device="cuda", dtype=torch.float64))


def test_bf16x3_precision_meets_the_tolerance(net, golden):
    """precision=1: every fp32 product as three bf16 MFMAs (hi*hi + hi*lo + lo*hi).  Same 1e-4 gate as fp32."""
    from oracle import stft as ostft
    from oracle import unet as ou
    g = golden("g6_unet_forward")
    net.precision = 1
    try:
        y = net(torch.from_numpy(g["x"]).cuda())
        r1 = ou.relative_l1(y.cpu(), torch.from_numpy(g["y"]))
        wav = synth.batch(2, seed=900, n=64000)
        x = torch.from_numpy(ostft.spectrogram(wav)).float().unsqueeze(1)
        with torch.no_grad():
            want = ou.forward(x[:1], formula_state_dict(0))
        r2 = ou.relative_l1(net(x.cuda())[:1].cpu(), want)
    finally:
        net.precision = 0
    assert r1 <= TOL and r2 <= TOL, (r1, r2)
    assert r1 > 1e-7          # it really is the split path


@pytest.mark.parametrize("family", ["bn_spread", "heavy_tail", "trained"])
def test_bf16x3_gate_on_stressed_and_trained_weight_families(family, trained_sd):
    """The 1e-4 forward gate of the headline arithmetic (bf16x3: hi*hi + hi*lo + lo*hi, fp32 accumulate) on weights that are NOT the
    benign formula family: BatchNorm scales spread over five decades with large running means, heavy-tailed (Cauchy) convolution
    weights, and weights after 50 optimiser steps of the training engine.  Full 8 s clips; the oracle (torch-CPU fp32, the
    reference's arithmetic) is the yardstick; the margin is printed and the fp32 MFMA path is held to 1e-5 on the same weights."""
    from musicfpaugment_amd.training.unet import UNet
    from musicfpaugment_amd.training.weights import stress_state_dict
    from oracle import stft as ostft
    from oracle import unet as ou
    sd = trained_sd() if family == "trained" else stress_state_dict(family, 0)
    m = UNet(1, 1, rate=0.05)
    m.load_state_dict(sd)
    m = m.cuda().eval()
    wav = synth.batch(2, seed=900, n=64000)
    x = torch.from_numpy(ostft.spectrogram(wav)).float().unsqueeze(1)
    with torch.no_grad():
        want = ou.forward(x, sd)
    assert torch.isfinite(want).all()
    got32 = m(x.cuda()).cpu()
    m.precision = 1
    got3 = m(x.cuda()).cpu()
    r32, r3 = ou.relative_l1(got32, want), ou.relative_l1(got3, want)
    print(f"[bf16x3 gate] family {family}: relative L1 bf16x3 {r3:.3e} (gate {TOL:g}, margin x{TOL / r3:.1f}), fp32 MFMA {r32:.3e}")
    assert r32 <= 1e-5, (family, r32)
    assert r3 <= TOL, (family, r3)
    assert r3 > 1e-7


def test_weights_direct_kernels_against_the_lds_staged_kernel():
    """The "weights direct" bf16x3 convolutions (csrc/unet_wd16.hip, csrc/unet_ws.hip: weight fragments from a fragment-ordered image straight into the MFMA
    operand registers, no weight tile in LDS, one barrier per chunk) against the pipelined kernel with LDS-staged weight tiles.
    conv_wd16_kernel (v_mfma_f32_16x16x32_bf16, w_layout 2) forms the same products but sums a 32-channel chunk inside one
    instruction: equal to fp32 rounding (<= 2e-6 of the largest output), bit-reproducible from run to run.  Ragged patch
    edges, the zero-padded second source of the decoder, the fused max-pool, the 16 x 16 patches of the 16 x 15 level, far more
    workgroups than CUs, and torch."""
    import torch.nn.functional as F
    from musicfpaugment_amd import ops_unet as K
    from musicfpaugment_amd._lib import lib
    from oracle.unet import relative_l1
    g = torch.Generator().manual_seed(7)
    lay = K.frag_layout()
    assert lay == 2

    def same(got, ref):
        return (got - ref).abs().max().item() <= 2e-6 * ref.abs().max().item()

    for (B, H, W, C0, C1, Cout, pool) in [(2, 9, 37, 64, 0, 128, False), (3, 33, 31, 128, 128, 128, False), (2, 16, 15, 512, 0, 1024, False),
                                          (1, 64, 62, 256, 0, 256, True), (40, 128, 125, 64, 0, 128, True), (1, 17, 16, 128, 0, 256, False),
                                          (2, 16, 16, 128, 0, 128, True),
                                          # >= 512 input channels: the loop form in which the three vertical taps share their fragment reads
                                          (1, 33, 31, 512, 0, 128, True), (1, 9, 34, 512, 512, 128, False),
                                          # 64-channel output tiles (4 x 2 waves of 64 pixels x 32 channels, persistent tile loop: more tiles than CUs below)
                                          (2, 9, 37, 64, 0, 64, False), (2, 33, 31, 64, 64, 64, False), (70, 64, 62, 128, 0, 64, True), (2, 16, 34, 128, 0, 64, True),
                                          (24, 257, 251, 64, 64, 64, False)]:
        assert lib().mfpa_conv_weight_layout(H, W, C0 + C1, Cout, 0, 1) == lay
        x0 = torch.randn(B, H, W, C0, generator=g).cuda()
        x1 = torch.randn(B, H - 1, W - 1, C1, generator=g).cuda() if C1 else None
        w = torch.randn(Cout, C0 + C1, 3, 3, generator=g) / np.sqrt(9 * (C0 + C1))
        sc, sh = (torch.rand(Cout, generator=g) + 0.5).cuda(), (torch.randn(Cout, generator=g) * 0.1).cuda()
        wk = K.pack_conv3x3(w).cuda()
        w3, wf = K.split_bf16x3(wk), (lay, K.split_bf16x3_frag(wk, lay))
        ref, ref_p, _ = K.conv3x3_fused(x0, w3, sc, sh, x1=x1, precision=1, pool=pool)
        first = None
        for _ in range(2):
            got, got_p, _ = K.conv3x3_fused(x0, w3, sc, sh, x1=x1, precision=1, pool=pool, wf=wf)
            assert same(got, ref), (B, H, W, C0, C1, Cout)
            assert (not pool) or same(got_p, ref_p)
            if first is None:
                first = (got, got_p)
            else:                                            # run-to-run: the same bits
                assert torch.equal(got, first[0]) and ((not pool) or torch.equal(got_p, first[1]))
        if pool:                                             # the fused pool is the pool of the kernel's own output, bit for bit
            assert torch.equal(got_p, F.max_pool2d(got.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1))
        if B <= 3:
            xin = x0.permute(0, 3, 1, 2).cpu()
            if C1:
                xin = torch.cat([xin, F.pad(x1.permute(0, 3, 1, 2).cpu(), [0, 1, 0, 1])], dim=1)
            want = F.relu(F.conv2d(xin, w, padding=1) * sc.cpu()[None, :, None, None] + sh.cpu()[None, :, None, None])
            assert relative_l1(got.cpu().permute(0, 3, 1, 2), want) < 1e-4
    # shapes the weights-direct kernels do not take keep the row image
    assert lib().mfpa_conv_weight_layout(257, 251, 32, 64, 0, 1) == 0 and lib().mfpa_conv_weight_layout(128, 125, 32, 128, 0, 1) == 0
    assert lib().mfpa_conv_weight_layout(128, 125, 64, 128, 0, 0) == 0 and lib().mfpa_conv_weight_layout(128, 125, 64, 128, 1, 1) == 0


def test_wave_specialised_64_channel_kernel_equals_conv_wd16_bit_for_bit():
    """conv_ws64_kernel (csrc/unet_ws.hip, round 5: 4 compute waves of 128 px x 32 ch + 4 loader waves; serves the inference launches with
    64 output channels) against conv_wd16_kernel<.., WMW = 4> (all eight waves do everything), which still serves the training step:
    asking for the bf16 copy of the output (a training side output) keeps a launch on the older kernel.  Same products, same order of
    the three bf16x3 terms, same 32-channel sums inside an instruction: IDENTICAL bits -- on ragged edges, one and two sources (the
    decoder's zero-padded concat), two and four chunks, fewer tiles than CUs, a tile count that is not a multiple of the grid, with the
    fused max-pool and the fused OutConv (stored and not stored)."""
    import torch.nn.functional as F
    from musicfpaugment_amd import ops_unet as K, ops_train as T
    from musicfpaugment_amd._lib import lib
    g = torch.Generator().manual_seed(17)
    if K.frag_layout() != 2:
        pytest.skip("the library was built without the 16 x 16 x 32 weights-direct kernels")
    for (B, H, W, C0, C1, pool, outc) in [(2, 9, 37, 64, 0, False, False), (2, 33, 31, 64, 64, False, False), (3, 40, 70, 64, 64, True, False),
                                          (1, 257, 251, 64, 0, True, True), (5, 64, 62, 128, 0, True, False), (2, 16, 34, 128, 128, False, True),
                                          (26, 257, 251, 64, 64, False, False), (26, 257, 251, 64, 0, False, True)]:
        assert lib().mfpa_conv_weight_layout(H, W, C0 + C1, 64, 0, 1) == 2
        x0 = torch.randn(B, H, W, C0, generator=g).cuda()
        x1 = torch.randn(B, H - 1, W - 1, C1, generator=g).cuda() if C1 else None
        w = torch.randn(64, C0 + C1, 3, 3, generator=g) / np.sqrt(9 * (C0 + C1))
        sc, sh = (torch.rand(64, generator=g) + 0.5).cuda(), (torch.randn(64, generator=g) * 0.1).cuda()
        wk = K.pack_conv3x3(w).cuda()
        w3, wf = K.split_bf16x3(wk), (2, K.split_bf16x3_frag(wk, 2))
        o1 = (torch.randn(64, generator=g).cuda(), 0.25) if outc else None
        got, got_p, got_1 = K.conv3x3_fused(x0, w3, sc, sh, x1=x1, precision=1, pool=pool, out1x1=o1, wf=wf)
        yb = []
        ref = T.conv_mfma(x0, wf[1], 64, x1=x1, out_scale=sc, out_shift=sh, relu=True, precision=1, packed=True, w_layout=2, y_bf16_out=yb)
        assert len(yb) == 1                                  # the side output was written: conv_wd16_kernel<SIDE> ran
        assert torch.equal(got, ref), (B, H, W, C0, C1)
        assert torch.equal(yb[0], ref.to(torch.bfloat16))
        if pool:
            assert torch.equal(got_p, F.max_pool2d(got.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1))
        if outc:
            want = (got.double() * o1[0].double()).sum(-1) + o1[1]
            assert float((got_1.double() - want).abs().max()) <= 1e-5 * float(want.abs().max())
            _, _, only = K.conv3x3_fused(x0, w3, sc, sh, x1=x1, precision=1, out1x1=o1, store=False, wf=wf)      # up4's form: no 64-channel store
            assert torch.equal(only, got_1)
        again, _, _ = K.conv3x3_fused(x0, w3, sc, sh, x1=x1, precision=1, pool=pool, out1x1=o1, wf=wf)
        assert torch.equal(again, got)                       # run to run
        if not pool and not outc:
            # without ReLU (and without a scale): the raw convolution, negative values and all -- the training forward's form of the call
            raw = T.conv_mfma(x0, wf[1], 64, x1=x1, precision=1, packed=True, w_layout=2)
            yb2 = []
            raw_ref = T.conv_mfma(x0, wf[1], 64, x1=x1, precision=1, packed=True, w_layout=2, y_bf16_out=yb2)
            assert len(yb2) == 1 and float(raw.min()) < 0 and torch.equal(raw, raw_ref)
        # the scale-folded form the UNet's eval chain uses (mfpa_conv_scale_folds): the scale in the weights (w * scale, then split), the
        # shift as the accumulators' start value, a bare ReLU in the epilogue -- the same numbers to bf16x3's own rounding
        assert lib().mfpa_conv_scale_folds(H, W, C0 + C1, 64) == 1
        wff = (2, K.split_bf16x3_frag(wk * sc[None, :, None], 2))
        fold, fold_p, fold_1 = K.conv3x3_fused(x0, w3, sc, sh, x1=x1, precision=1, pool=pool, out1x1=o1, wf=wf, wff=wff)
        scale_ = float(got.abs().max())
        assert float((fold - got).abs().max()) <= 2e-5 * scale_ and float((fold - got).abs().mean()) <= 2e-6 * scale_, (B, H, W, C0, C1)
        assert float((fold - got).abs().max()) > 0           # (it really is the other arithmetic)
        if pool:
            assert torch.equal(fold_p, F.max_pool2d(fold.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1))
        if outc:
            assert float((fold_1 - got_1).abs().max()) <= 2e-5 * float(got_1.abs().max())
        if B <= 3:
            xin = x0.permute(0, 3, 1, 2).cpu()
            if C1:
                xin = torch.cat([xin, F.pad(x1.permute(0, 3, 1, 2).cpu(), [0, 1, 0, 1])], dim=1)
            want = F.relu(F.conv2d(xin, w, padding=1) * sc.cpu()[None, :, None, None] + sh.cpu()[None, :, None, None])
            from oracle.unet import relative_l1
            assert relative_l1(got.cpu().permute(0, 3, 1, 2), want) < 1e-4


def test_first_layer_on_the_matrix_cores_inside_the_loader_waves():
    """conv_ws64_kernel<C1SRC> (round 5): the UNet's first layer (Conv2d(1, 64, 3, padding 1) + folded BatchNorm + ReLU, training/unet.py:16-18)
    is computed by the LOADER waves of the second layer's kernel on the matrix cores (the nine taps padded to K = 16, bf16x3 like every other
    layer) instead of ~1300 exact-fp32 vector instructions per chunk and thread in conv_mfma_kernel<.., C1SRC>'s loader.  Against that
    older launch (ops_unet.C1_ON_MFMA = False): the same output to bf16x3's rounding of ONE more layer (relative L1 < 2e-5, the chain's gate
    is 1e-4), the fused max-pool = the pool of its own output bit for bit, both source forms (float32 input, float64 spectrogram / per-clip
    maximum), ragged sizes, fewer tiles than CUs and many more; and against torch on the small shapes."""
    import torch.nn.functional as F
    from musicfpaugment_amd import ops_unet as K
    from musicfpaugment_amd._lib import lib
    from oracle.unet import relative_l1
    g = torch.Generator().manual_seed(23)
    if K.frag_layout() != 2:
        pytest.skip("the library was built without the 16 x 16 x 32 weights-direct kernels")
    for (B, H, W, use64) in [(2, 9, 37, False), (3, 40, 70, True), (1, 257, 251, True), (20, 257, 251, False), (2, 17, 33, True)]:
        assert lib().mfpa_conv_c1_layout(H, W) == 2
        w1 = (torch.randn(64, 1, 3, 3, generator=g) / 3.0)
        w2 = torch.randn(64, 64, 3, 3, generator=g) / np.sqrt(9 * 64)
        s1, b1 = (torch.rand(64, generator=g) + 0.5).cuda(), (torch.randn(64, generator=g) * 0.2).cuda()
        s2, b2 = (torch.rand(64, generator=g) + 0.5).cuda(), (torch.randn(64, generator=g) * 0.1).cuda()
        w1k = w1.permute(2, 3, 1, 0).reshape(9, 64).contiguous().cuda()
        wk = K.pack_conv3x3(w2).cuda()
        w3, wf = K.split_bf16x3(wk), (2, K.split_bf16x3_frag(wk, 2))
        wff = (2, K.split_bf16x3_frag(wk * s2[None, :, None], 2))
        x = torch.rand(B, H, W, generator=g)
        if use64:
            den = (torch.rand(B, generator=g) + 0.5).double()
            c1 = dict(spec64=(x.double() * den[:, None, None]).cuda(), denom=den.cuda(), w=w1k, scale=s1, shift=b1)
            xin = ((x.double() * den[:, None, None]) / den[:, None, None]).float()
        else:
            c1 = dict(x32=x.cuda(), w=w1k, scale=s1, shift=b1)
            xin = x
        K.C1_ON_MFMA = False
        try:
            ref, ref_p, _ = K.conv3x3_fused(None, w3, s2, b2, precision=1, pool=True, wf=wf, c1=c1)
        finally:
            K.C1_ON_MFMA = True
        got, got_p, _ = K.conv3x3_fused(None, w3, s2, b2, precision=1, pool=True, wf=wf, c1=c1)
        fold, fold_p, _ = K.conv3x3_fused(None, w3, s2, b2, precision=1, pool=True, wf=wf, wff=wff, c1=c1)
        r = relative_l1(got.cpu(), ref.cpu())
        assert 0 < r < 2e-5, (B, H, W, r)
        assert relative_l1(fold.cpu(), ref.cpu()) < 2e-5
        assert torch.equal(got_p, F.max_pool2d(got.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1))
        assert torch.equal(fold_p, F.max_pool2d(fold.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1))
        again, _, _ = K.conv3x3_fused(None, w3, s2, b2, precision=1, pool=True, wf=wf, c1=c1)
        assert torch.equal(again, got)
        if B <= 3:
            m = F.relu(F.conv2d(xin[:, None], w1, padding=1) * s1.cpu()[None, :, None, None] + b1.cpu()[None, :, None, None])
            want = F.relu(F.conv2d(m, w2, padding=1) * s2.cpu()[None, :, None, None] + b2.cpu()[None, :, None, None])
            assert relative_l1(got.cpu().permute(0, 3, 1, 2), want) < 1e-4


def _to_split(x):
    """float32 NHWC (C % 32 == 0) -> the SPLIT layout of include/mfpa.h (mfpa_conv_desc.x0_split ...): per pixel and 32-channel chunk
    [32 bf16 hi | 32 bf16 lo], returned as a float32 tensor of the same shape (same bytes)."""
    B, H, W, C = x.shape
    x4 = x.reshape(B, H, W, C // 32, 32)
    hi = x4.to(torch.bfloat16)
    lo = (x4 - hi.float()).to(torch.bfloat16)
    return torch.cat([hi, lo], dim=-1).contiguous().view(torch.float32).reshape(B, H, W, C)


def test_split_layout_between_wave_specialised_convolutions():
    """Round 5: between two conv_ws64_kernel launches a tensor travels in the SPLIT layout -- [32 bf16 hi | 32 bf16 lo] per 32-channel chunk of a
    pixel, the very pieces a bf16x3 loader makes of float32 values -- so the producer splits each value ONCE and the consumer's loader waves
    only copy.  (1) A source handed over in that layout gives the SAME BITS as the float32 tensor it was made from (source 0, source 1, both;
    two and four chunks; ragged edges and many tiles).  (2) `y_split` / `pool_split` outputs ARE the split of the float32 outputs, bit for
    bit (64- and 128-channel outputs, with the fused first layer too).  (3) The whole UNet with and without split edges: identical output.
    (4) A launch conv_ws64_kernel does not serve refuses the flags."""
    import torch.nn.functional as F
    from musicfpaugment_amd import ops_unet as K
    from musicfpaugment_amd._lib import lib
    g = torch.Generator().manual_seed(29)
    if K.frag_layout() != 2:
        pytest.skip("the library was built without the 16 x 16 x 32 weights-direct kernels")
    for (B, H, W, C0, C1, Cout, pool) in [(2, 9, 37, 64, 0, 64, False), (3, 40, 70, 64, 64, 64, True), (6, 128, 125, 64, 0, 128, True),
                                          (2, 33, 31, 128, 0, 128, True), (20, 257, 251, 64, 64, 64, False), (2, 64, 62, 128, 0, 256, False)]:
        assert lib().mfpa_conv_scale_folds(H, W, C0 + C1, Cout) == 1
        x0 = torch.randn(B, H, W, C0, generator=g).cuda()
        x1 = torch.randn(B, H - 1, W - 1, C1, generator=g).cuda() if C1 else None
        w = torch.randn(Cout, C0 + C1, 3, 3, generator=g) / np.sqrt(9 * (C0 + C1))
        sc, sh = (torch.rand(Cout, generator=g) + 0.5).cuda(), (torch.randn(Cout, generator=g) * 0.1).cuda()
        wk = K.pack_conv3x3(w).cuda()
        w3, wf = K.split_bf16x3(wk), (2, K.split_bf16x3_frag(wk, 2))
        ref, ref_p, _ = K.conv3x3_fused(x0, w3, sc, sh, x1=x1, precision=1, pool=pool, wf=wf)
        # (1) split sources
        a, a_p, _ = K.conv3x3_fused(_to_split(x0), w3, sc, sh, x1=x1, precision=1, pool=pool, wf=wf, x0_split=True)
        assert torch.equal(a, ref) and (not pool or torch.equal(a_p, ref_p)), (B, H, W, C0, C1, Cout)
        if C1:
            b_, _, _ = K.conv3x3_fused(x0, w3, sc, sh, x1=_to_split(x1), precision=1, pool=pool, wf=wf, x1_split=True)
            c_, _, _ = K.conv3x3_fused(_to_split(x0), w3, sc, sh, x1=_to_split(x1), precision=1, pool=pool, wf=wf, x0_split=True, x1_split=True)
            assert torch.equal(b_, ref) and torch.equal(c_, ref)
        # (2) split outputs
        s_, s_p, _ = K.conv3x3_fused(x0, w3, sc, sh, x1=x1, precision=1, pool=pool, wf=wf, y_split=True, pool_split=pool)
        assert torch.equal(s_.view(torch.int32), _to_split(ref).view(torch.int32)), (B, H, W, C0, C1, Cout)
        if pool:
            assert torch.equal(s_p.view(torch.int32), _to_split(ref_p).view(torch.int32))
    # the fused first layer as a producer
    B, H, W = 3, 40, 70
    w1k = (torch.randn(9, 64, generator=g) / 3.0).cuda()
    s1, b1 = (torch.rand(64, generator=g) + 0.5).cuda(), (torch.randn(64, generator=g) * 0.2).cuda()
    wk = K.pack_conv3x3(torch.randn(64, 64, 3, 3, generator=g) / 24.0).cuda()
    w3, wf = K.split_bf16x3(wk), (2, K.split_bf16x3_frag(wk, 2))
    sc, sh = (torch.rand(64, generator=g) + 0.5).cuda(), (torch.randn(64, generator=g) * 0.1).cuda()
    c1 = dict(x32=torch.rand(B, H, W, generator=g).cuda(), w=w1k, scale=s1, shift=b1)
    ref, ref_p, _ = K.conv3x3_fused(None, w3, sc, sh, precision=1, pool=True, wf=wf, c1=c1)
    s_, s_p, _ = K.conv3x3_fused(None, w3, sc, sh, precision=1, pool=True, wf=wf, c1=c1, y_split=True, pool_split=True)
    assert torch.equal(s_.view(torch.int32), _to_split(ref).view(torch.int32)) and torch.equal(s_p.view(torch.int32), _to_split(ref_p).view(torch.int32))
    # (3) the whole network
    from musicfpaugment_amd.training.unet import UNet
    m = UNet(1, 1, rate=0.05)
    m.load_state_dict(formula_state_dict(0))
    m = m.cuda().eval()
    m.precision = 1
    x = torch.from_numpy(synth.batch(3, seed=77)).cuda()
    from musicfpaugment_amd import ops
    mag, cmax = ops.stft_mag(x, torch.float64)
    with torch.no_grad():
        y_split = m.denoise_spectrogram(mag, cmax, per_clip=True)
        K.SPLIT_EDGES = False
        try:
            y_plain = m.denoise_spectrogram(mag, cmax, per_clip=True)
        finally:
            K.SPLIT_EDGES = True
    assert torch.equal(y_split, y_plain)
    # (4) refused elsewhere: a 512-input-channel layer runs on conv_wd16_kernel
    xs = torch.randn(1, 32, 31, 512, generator=g).cuda()
    wk = K.pack_conv3x3(torch.randn(128, 512, 3, 3, generator=g) / 60.0).cuda()
    with pytest.raises(ValueError):
        K.conv3x3_fused(xs, K.split_bf16x3(wk), torch.ones(128).cuda(), torch.zeros(128).cuda(), precision=1, wf=(2, K.split_bf16x3_frag(wk, 2)), x0_split=True)


def test_plan_split_edges_at_the_headline_shape():
    """unet_plan's split edges at 257 x 251, bf16x3, as the hand-written per-edge conditions of the forward chose them (recorded from
    that code's launches on the MI355X).  With up4 folded its two edges (inc -> up4.0, up4.0 -> up4.3) are plain float32; the three
    encoder edges follow the launches on conv_ws64_kernel."""
    from musicfpaugment_amd import ops_unet as K
    if K.frag_layout() != 2:
        pytest.skip("the library was built without the 16 x 16 x 32 weights-direct kernels")
    d1, d2 = "down1.maxpool_conv.1.double_conv", "down2.maxpool_conv.1.double_conv"
    encoder = {("inc.double_conv.3", "pool_split"), (d1 + ".0", "x0_split"), (d1 + ".0", "y_split"), (d1 + ".3", "x0_split"),
               (d1 + ".3", "pool_split"), (d2 + ".0", "x0_split")}
    up4 = {("inc.double_conv.3", "y_split"), ("up4.conv.double_conv.0", "x0_split"), ("up4.conv.double_conv.0", "y_split"),
           ("up4.conv.double_conv.3", "x0_split")}
    for fold, want in ((True, encoder), (False, encoder | up4)):
        K.FOLD_UP = fold
        try:
            plan = K.unet_plan(257, 251, 1)
        finally:
            K.FOLD_UP = True
        got = {(key, f) for key, st in plan.items() for f in ("x0_split", "y_split", "pool_split") if getattr(st, f)}
        assert got == want, (fold, sorted(got ^ want))
        assert ("up4.conv.double_conv.0" in plan) != fold
