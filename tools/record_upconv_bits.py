#!/usr/bin/env python3
"""Record what mfpa_upconv_fused (csrc/unet_up.hip) computes, bit for bit: for every case of CASES, both precisions, the sha256 of the
output's bytes and its first 16 floats -> tests/golden/upconv_bits.json.  tests/test_gpu_upconv_bits.py recomputes the hashes with the
library in the tree and requires equality, so the file is recorded with the library of the commit whose results are to be kept:

    record_upconv_bits.py [--lib <libmfpa.so of that commit>] [--out <json>]

Operands are seeded numpy arrays.  The weight images are made on the CPU (ops_unet.weight_image) from seeded weights, the composite
weights and the bias table are seeded arrays too (mfpa_upconv_pack is not involved): nothing but the one launch runs on the device.

Cases -- the smallest shapes at which the kernel's paths differ: Cl / 32 = 1 .. 4 low-resolution chunks (one, a pair, a pair and a
single, two pairs), Cs / 32 = 2, 3 skip chunks, one and two channel groups, and three geometries: one tile without interior; a padding
row and column with four edge tiles; interior tiles with 320 tiles on at most 256 workgroups, so that workgroups cross a tile boundary."""
import argparse
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GEOMETRIES = [(1, 8, 32, 4, 16), (1, 9, 35, 4, 17), (20, 26, 98, 13, 49)]          # (B, H, W, Hl, Wl)
CASES = [(B, H, W, Hl, Wl, Cs, Cl, Cout) for (B, H, W, Hl, Wl) in GEOMETRIES for Cl in (32, 64, 96, 128) for Cs in (64, 96) for Cout in (64, 128)]
PRECISIONS = (1, 0)
DEFAULT_OUT = os.path.join(ROOT, "tests", "golden", "upconv_bits.json")


def case_id(case, precision):
    return "B%d_%dx%d_low%dx%d_Cs%d_Cl%d_Cout%d_p%d" % (case + (precision,))


def operands(case):
    """Seeded numpy operands of one case: skip, low (NHWC), w_skip [9][Cout][Cs], w_up [16][Cout][Cl], shift, bias table [4][4][Cout]."""
    B, H, W, Hl, Wl, Cs, Cl, Cout = case
    rng = np.random.default_rng([2107] + list(case))
    f = lambda *shape: rng.standard_normal(shape, dtype=np.float32)
    return {"skip": f(B, H, W, Cs), "low": f(B, Hl, Wl, Cl),
            "w_skip": f(9, Cout, Cs) / np.float32(np.sqrt(9 * Cs)), "w_up": f(16, Cout, Cl) / np.float32(np.sqrt(4 * Cl)),
            "shift": f(Cout) * np.float32(0.1), "bias": f(4, 4, Cout) * np.float32(0.1)}


def run(case, precision):
    """One mfpa_upconv_fused launch on the case's operands through the C ABI -> the output (B, H, W, Cout) as a numpy array."""
    import torch
    from musicfpaugment_amd import ops_unet as K
    from musicfpaugment_amd._lib import UpconvDesc, check, lib, ptr, stream
    B, H, W, Hl, Wl, Cs, Cl, Cout = case
    if lib().mfpa_upconv_serves(H, W, Hl, Wl, Cs, Cl, Cout) != 1:
        raise ValueError(f"mfpa_upconv_fused does not serve {case}")
    op = operands(case)
    dev = {k: torch.from_numpy(v).cuda() for k, v in op.items() if not k.startswith("w_")}
    wsk = K.weight_image(torch.from_numpy(op["w_skip"]), precision, 2).t.cuda()
    wup = K.weight_image(torch.from_numpy(op["w_up"]), precision, 2).t.cuda()
    y = torch.full((B, H, W, Cout), float("nan"), dtype=torch.float32, device="cuda")
    d = UpconvDesc(skip=ptr(dev["skip"]), low=ptr(dev["low"]), w_skip=ptr(wsk), w_up=ptr(wup), shift=ptr(dev["shift"]), bias_tab=ptr(dev["bias"]),
                   y=ptr(y), B=B, H=H, W=W, Cs=Cs, Hl=Hl, Wl=Wl, Cl=Cl, Cout=Cout, relu=1, precision=precision)
    check(lib().mfpa_upconv_fused(ctypes.byref(d), stream()), "mfpa_upconv_fused")
    torch.cuda.synchronize()
    return y.cpu().numpy()


def digest(y):
    return {"sha256": hashlib.sha256(np.ascontiguousarray(y).tobytes()).hexdigest(), "first16": [float(v) for v in y.reshape(-1)[:16]]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", default=None, help="another build of libmfpa.so (default: the one in the tree)")
    ap.add_argument("--out", default=DEFAULT_OUT)
    args = ap.parse_args()
    if args.lib:
        from musicfpaugment_amd import _lib
        _lib.set_library_path(args.lib)
    rec = {}
    for case in CASES:
        for precision in PRECISIONS:
            y = run(case, precision)
            assert np.isfinite(y).all(), (case, precision)
            rec[case_id(case, precision)] = digest(y)
            print(case_id(case, precision), rec[case_id(case, precision)]["sha256"][:16], flush=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(rec, indent=1, sort_keys=True) + "\n")
    print(f"{len(rec)} cases -> {args.out}")


if __name__ == "__main__":
    main()
