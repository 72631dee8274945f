"""mfpa_upconv_fused (csrc/unet_up.hip) computes, bit for bit, what it computed before its fragment reads were shared: the products and the
order of every accumulator's additions are part of the kernel's contract, so a change of its read or staging schedule must leave every
output byte alone.  tests/golden/upconv_bits.json holds the sha256 of the output bytes (and the first 16 floats, for a readable failure) of
tools/record_upconv_bits.py's cases, recorded with the library of the commit BEFORE that change; a difference here is a bug, not a tolerance
question.  Cl = 32 and 96 (one low-resolution chunk, three) are also compared with the float64 reference formulation, with the helpers and
bounds of tests/test_gpu_upconv.py."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_tool():
    spec = importlib.util.spec_from_file_location("record_upconv_bits", os.path.join(ROOT, "tools", "record_upconv_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _load_tool()
with open(os.path.join(ROOT, "tests", "golden", "upconv_bits.json")) as _fh:
    GOLDEN_BITS = json.load(_fh)


def test_the_golden_file_covers_exactly_the_recorded_cases():
    assert sorted(GOLDEN_BITS) == sorted(REC.case_id(c, p) for c in REC.CASES for p in REC.PRECISIONS)
    assert {c[6] for c in REC.CASES} == {32, 64, 96, 128} and {c[5] for c in REC.CASES} == {64, 96} and {c[7] for c in REC.CASES} == {64, 128}
    assert {c[:5] for c in REC.CASES} == {(1, 8, 32, 4, 16), (1, 9, 35, 4, 17), (20, 26, 98, 13, 49)}


@pytest.mark.parametrize("precision", REC.PRECISIONS)
@pytest.mark.parametrize("case", REC.CASES, ids=lambda c: "-".join(map(str, c)))
def test_upconv_fused_output_bits_are_those_of_the_recorded_commit(case, precision):
    y = REC.run(case, precision)
    got, want = REC.digest(y), GOLDEN_BITS[REC.case_id(case, precision)]
    if got["sha256"] != want["sha256"]:
        print(f"[upconv bits {case} precision {precision}] first 16 floats now {got['first16']}, recorded {want['first16']}")
    assert got["sha256"] == want["sha256"], (case, precision)


def _level(g, B, H, W, Hl, Wl, Cs, Cu, Cl, Cout):
    skip = torch.randn(B, Cs, H, W, generator=g)
    low = torch.randn(B, Cl, Hl, Wl, generator=g)
    wt = torch.randn(Cl, Cu, 2, 2, generator=g) / np.sqrt(Cl)
    bt = torch.randn(Cu, generator=g) * 0.5
    w3 = torch.randn(Cout, Cs + Cu, 3, 3, generator=g) / np.sqrt(9 * (Cs + Cu))
    sc, sh = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.1
    return skip, low, wt, bt, w3, sc, sh


def _reference(skip, low, wt, bt, w3, sc, sh):
    dd = torch.float64
    up = F.conv_transpose2d(low.to(dd), wt.to(dd), bt.to(dd), stride=2)
    dY, dX = skip.shape[2] - up.shape[2], skip.shape[3] - up.shape[3]
    up = F.pad(up, [dX // 2, dX - dX // 2, dY // 2, dY - dY // 2])                     # unet.py:60-63
    z = F.conv2d(torch.cat([skip.to(dd), up], dim=1), w3.to(dd), padding=1)
    return F.relu(z * sc.to(dd)[None, :, None, None] + sh.to(dd)[None, :, None, None])


def _fused(skip, low, wt, bt, w3, sc, sh, precision):
    from musicfpaugment_amd import ops_unet as K
    pw = {"L.conv.double_conv.0.w": K.pack_conv3x3(w3).cuda(), "L.up.w": K.pack_convT2x2(wt).cuda(), "L.up.b": bt.cuda(),
          "L.conv.double_conv.0.scale": sc.cuda(), "L.conv.double_conv.0.shift": sh.cuda()}
    pk = K.pack_upconv(pw, "L", precision)
    return K.upconv_fused(skip.permute(0, 2, 3, 1).contiguous().cuda(), low.permute(0, 2, 3, 1).contiguous().cuda(), pk["L.upc.wsk"], pk["L.upc.wup"],
                          sh.cuda(), pk["L.upc.bias"], w3.shape[0], precision=precision)


@pytest.mark.parametrize("shape", [
    (2, 9, 35, 4, 17, 64, 32, 32, 64),        # Cl = 32: the low half is one chunk; padding row and column, four edge tiles
    (2, 26, 98, 13, 49, 96, 48, 96, 128),     # Cl = 96: three low chunks; interior tiles, three skip chunks, two channel groups
    (1, 8, 32, 4, 16, 64, 32, 96, 64),        # Cl = 96 on one tile without interior
])
def test_upconv_fused_with_one_and_three_low_chunks_matches_the_reference_formulation(shape):
    from musicfpaugment_amd._lib import lib
    from oracle.unet import relative_l1
    B, H, W, Hl, Wl, Cs, Cu, Cl, Cout = shape
    assert lib().mfpa_upconv_serves(H, W, Hl, Wl, Cs, Cl, Cout) == 1
    args = _level(torch.Generator().manual_seed(sum(shape)), *shape)
    want = _reference(*args)
    for precision, bound in ((1, 1e-5), (0, 2e-6)):
        got = _fused(*args, precision=precision).cpu().permute(0, 3, 1, 2).double()
        rl1 = relative_l1(got, want)
        print(f"[upconv {shape} precision {precision}] relative L1 {rl1:.2e} (bound {bound:.0e})")
        assert rl1 <= bound, (shape, precision, rl1)
        for sl in (np.s_[:, :, 0], np.s_[:, :, -1], np.s_[:, :, :, 0], np.s_[:, :, :, -1]):         # the border lines: bias classes, zero padding
            assert relative_l1(got[sl], want[sl]) <= 3 * bound, (shape, precision, sl)
