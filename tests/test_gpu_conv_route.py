"""Every instantiation of the UNet convolution family launched once through mfpa_conv_mfma, from the descriptor of its row of the case
table (tests/_conv_route_cases.py), at that row's small shape: the descriptor must route to the instantiation the row names (now with
real pointers), the launch must succeed, and the stored output is compared with a float64 torch reference.  NaN sentinels sit in front of
and behind the output.

Bounds (relative L1 of the whole output, the metric and the figures the existing tests use for the same arithmetic): fp32 products 1e-5
(tests/test_gpu_unet.py, tests/test_gpu_train.py building blocks), bf16x3 1e-4 (tests/test_gpu_unet.py), one bf16 product per term or
a bfloat16-only output 6e-3 (tests/test_gpu_train.py, plain bf16)."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from tests import _conv_route_cases as rc

pytestmark = pytest.mark.gpu
GUARD = 1024
CASES = rc.cases()


@pytest.fixture(scope="module")
def lib():
    from musicfpaugment_amd import _lib
    return _lib


def _guarded(n, dtype):
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n]


@pytest.mark.parametrize("name,fields,want", CASES, ids=[c[0] for c in CASES])
def test_row_launches_the_kernel_it_names_and_computes_the_convolution(lib, name, fields, want):
    from musicfpaugment_amd import ops_unet as K
    from oracle.unet import relative_l1
    f = dict(C0=64, C1=0, B=1, H=8, W=33, Cout=64, mode=0, precision=0, w_layout=0)
    f.update(fields)
    assert f["C1"] == 0
    B, H, W, C0, Cout, mode, prec, lay = (f[k] for k in ("B", "H", "W", "C0", "Cout", "mode", "precision", "w_layout"))
    g = torch.Generator().manual_seed(len(name) * 7919 + C0 + Cout)
    keep = []                                                          # device tensors the descriptor points into
    p = {}

    def dev(t, key):
        t = t.contiguous().cuda()
        keep.append(t)
        p[key] = lib.ptr(t)
        return t

    taps = 9 if mode == 0 else 4
    wk = torch.randn(taps, Cout, C0, generator=g) / math.sqrt(taps * C0)          # kernel layout [tap][Cout][Cin]
    wdev = wk.cuda()
    dev(wdev if prec == 0 else (K.split_bf16x3_frag(wdev, 2) if lay == 2 else K.split_bf16x3(wdev)), "w")
    sh_src = (B, 2 * H, 2 * W, C0) if mode == 2 else (B, H, W, C0)
    if f.get("c1_x32"):                                                 # source 0 = the fused first layer of the 1-channel input
        x1c = torch.rand(B, H, W, generator=g)
        c1w, c1s, c1b = torch.randn(9, 64, generator=g) / 3, torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.1
        dev(x1c, "c1_x32"); dev(c1w, "c1_w"); dev(c1s, "c1_scale"); dev(c1b, "c1_shift")
        src = F.relu(F.conv2d(x1c.double()[:, None], c1w.double().t().reshape(64, 1, 3, 3), padding=1) * c1s.double()[None, :, None, None]
                     + c1b.double()[None, :, None, None])
    else:
        x0 = torch.randn(sh_src, generator=g)
        if f.get("x0_is_bf16"):
            x0 = x0.bfloat16()
        dev(x0, "x0")
        src = x0.double().permute(0, 3, 1, 2)
        if f.get("in_scale0"):
            sc, sh = torch.rand(C0, generator=g) + 0.5, torch.randn(C0, generator=g) * 0.3
            dev(sc, "in_scale0"); dev(sh, "in_shift0")
            src = F.relu(src * sc.double()[None, :, None, None] + sh.double()[None, :, None, None])
    w64 = wk.double()
    if mode == 0:
        ref = F.conv2d(src, w64.view(3, 3, Cout, C0).permute(2, 3, 0, 1), padding=1)
    elif mode == 1:
        ref = F.conv_transpose2d(src, w64.view(2, 2, Cout, C0).permute(3, 2, 0, 1), stride=2)
    else:
        ref = F.conv2d(src, w64.view(2, 2, Cout, C0).permute(2, 3, 0, 1), stride=2)
    oh, ow = ref.shape[2], ref.shape[3]
    n = B * oh * ow * Cout
    bf16_only = not f.get("y", 1)
    buf, out = _guarded(n, torch.bfloat16 if bf16_only else torch.float32)
    p["y_bf16" if bf16_only else "y"] = buf.data_ptr() + GUARD * buf.element_size()
    if f.get("y_bf16") and not bf16_only:
        dev(torch.empty(n, dtype=torch.bfloat16), "y_bf16")
    if f.get("x0_bf16"):
        dev(torch.empty(sh_src, dtype=torch.bfloat16), "x0_bf16")
    if f.get("stats_part"):
        rows = lib.lib().mfpa_conv_stats_rows(B, H, W, C0, Cout)
        assert rows > 0
        dev(torch.empty(rows, 2, Cout), "stats_part")
    if f.get("bwd_z"):
        dev(torch.randn(B, H, W, Cout, generator=g), "bwd_z")
        for k in ("bwd_scale", "bwd_shift", "bwd_mean", "bwd_invstd"):
            dev(torch.rand(Cout, generator=g) + 0.5, k)
    d = rc.desc(lib, **{**f, **p})
    code, got, _ = rc.route(lib, d)
    assert code == 0 and got == want, (name, code, got, want)
    lib.check(lib.lib().mfpa_conv_mfma(ctypes.byref(d), lib.stream()), name)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all()), (name, "wrote outside the output")
    y = out.view(B, oh, ow, Cout).float().cpu()
    assert bool(torch.isfinite(y).all()), (name, "an output element was not stored")
    bound = 1e-5 if prec == 0 else 6e-3 if (prec == 2 or bf16_only or f.get("x0_is_bf16")) else 1e-4
    r = relative_l1(y.permute(0, 3, 1, 2), ref)
    print(f"CONV-ROUTE {name}: relative L1 {r:.3g} (bound {bound:g})")
    assert r < bound, (name, r, bound)
