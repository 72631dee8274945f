#!/usr/bin/env python3
"""Record what conv_ws64_kernel (csrc/unet_ws.hip) computes, bit for bit: for every case of CASES the sha256 of the bytes of every output
the launch writes (full-resolution, pooled, OutConv -- in that order) and the first 16 floats of the first of them ->
tests/golden/ws64_bits.json.  tests/test_gpu_ws64_bits.py recomputes the hashes with the library in the tree and requires equality, so
the file is recorded with the library of the commit whose results are to be kept:

    record_ws64_bits.py [--lib <libmfpa.so of that commit>] [--out <json>]

Operands are seeded numpy arrays; the weight images are made on the CPU (ops_unet.split_bf16x3_frag): nothing but the one launch runs on
the device, through ops_unet.conv3x3_fused, and every case is required to route to conv_ws64_kernel (ops_unet.conv_route).

Cases -- the smallest shapes at which the kernel's paths differ.  Geometries (B, H, W): one tile without interior; a padding row and
column with four edge tiles; interior tiles with a ragged right edge and two clips; and the last one with 20 clips (320 tiles on at most
256 workgroups: workgroups cross a tile boundary) for a few forms.  Channels (C0, C1, Cout): every combination of C0 in {64, 96, 128},
a second source of 32 channels (two pixels smaller each way and three narrower: offset (1, 1)) and Cout in {64, 128} that the routing
gives to this kernel -- 64 outputs need a multiple of 64 input channels, 128 outputs at most 128 of them.  Forms: plain; fused max-pool;
fused OutConv without the 64-channel store (64 outputs); sources and outputs in the split layout; the scale folded into the weights.
And the fused first layer <C1SRC> from both source forms (float64 spectrogram + per-clip denominator, float32), pooled, split, folded."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GEOMETRIES = [(1, 8, 32), (1, 9, 35), (2, 26, 98)]                                   # (B, H, W)
WALK = (20, 26, 98)                                                                  # more tiles than workgroups
CHANNELS = [(C0, C1, Cout) for C0 in (64, 96, 128) for C1 in (0, 32) for Cout in (64, 128)
            if ((C0 + C1) % 64 == 0 if Cout == 64 else C0 + C1 <= 128)]
FORMS = ("plain", "pool", "out1x1", "split", "folded")
C1_FORMS = ("pool", "split", "folded")
# a case: (B, H, W, C0, C1, Cout, form, c1 source: "" | "spec64" | "x32")
CASES = [(B, H, W, C0, C1, Cout, form, "") for (B, H, W) in GEOMETRIES for (C0, C1, Cout) in CHANNELS for form in FORMS
         if form != "out1x1" or Cout == 64]
CASES += [(B, H, W, 64, 0, 64, form, src) for (B, H, W) in GEOMETRIES for src in ("spec64", "x32") for form in C1_FORMS]
CASES += [WALK + (64, 0, 64, "pool", ""), WALK + (96, 32, 64, "plain", ""), WALK + (64, 32, 128, "split", ""), WALK + (64, 0, 64, "out1x1", ""),
          WALK + (64, 0, 64, "pool", "x32")]
DEFAULT_OUT = os.path.join(ROOT, "tests", "golden", "ws64_bits.json")


def case_id(case):
    B, H, W, C0, C1, Cout, form, src = case
    return "B%d_%dx%d_C%d+%d_Cout%d_%s%s" % (B, H, W, C0, C1, Cout, form, "_c1" + src if src else "")


def operands(case):
    """Seeded numpy operands of one case."""
    B, H, W, C0, C1, Cout, form, src = case
    rng = np.random.default_rng([2108, B, H, W, C0, C1, Cout, FORMS.index(form), ("", "spec64", "x32").index(src)])
    f = lambda *shape: rng.standard_normal(shape, dtype=np.float32)
    u = lambda *shape: rng.random(shape, dtype=np.float32)
    op = {"w": f(9, Cout, C0 + C1) / np.float32(np.sqrt(9 * (C0 + C1))), "scale": u(Cout) + np.float32(0.5), "shift": f(Cout) * np.float32(0.1)}
    if src:
        op.update(c1_w=f(9, 64) / np.float32(3.0), c1_scale=u(64) + np.float32(0.5), c1_shift=f(64) * np.float32(0.2), x=u(B, H, W))
        if src == "spec64":
            op["denom"] = (u(B) + np.float32(0.5)).astype(np.float64)
    else:
        op["x0"] = f(B, H, W, C0)
        if C1:
            op["x1"] = f(B, H - 2, W - 3, C1)
    if form == "out1x1":
        op["w1x1"] = f(64)
    return op


def to_split(x):
    """float32 NHWC (C % 32 == 0) -> the split layout of include/mfpa.h: per pixel and 32-channel chunk [32 bf16 hi | 32 bf16 lo], same bytes."""
    import torch
    B, H, W, C = x.shape
    x4 = x.reshape(B, H, W, C // 32, 32)
    hi = x4.to(torch.bfloat16)
    lo = (x4 - hi.float()).to(torch.bfloat16)
    return torch.cat([hi, lo], dim=-1).contiguous().view(torch.float32).reshape(B, H, W, C)


def run(case):
    """One conv_ws64_kernel launch on the case's operands -> the outputs it wrote (numpy arrays; full-resolution, pooled, OutConv order)."""
    import torch
    from musicfpaugment_amd import ops_unet as K
    B, H, W, C0, C1, Cout, form, src = case
    if not K.conv_route(H, W, C0 + C1, Cout, 2, c1=bool(src), out1x1=form == "out1x1")[2]:
        raise ValueError(f"conv_ws64_kernel does not serve {case}")
    op = {k: torch.from_numpy(v) for k, v in operands(case).items()}
    wk = op["w"]
    sc, sh = op["scale"].cuda(), op["shift"].cuda()
    w3 = K.split_bf16x3(wk).cuda()
    wf = (2, K.split_bf16x3_frag(wk, 2).cuda())
    kw = dict(precision=1, wf=wf)
    if form == "folded":
        kw.update(wff=(2, K.split_bf16x3_frag(wk * op["scale"][None, :, None], 2).cuda()), pool=True)
    split = form == "split"
    if form in ("pool", "split"):
        kw.update(pool=True)
    if split:
        kw.update(y_split=True, pool_split=True)
    if form == "out1x1":
        kw.update(out1x1=(op["w1x1"].cuda(), 0.25), store=False)
    if src:
        c1 = dict(w=op["c1_w"].cuda(), scale=op["c1_scale"].cuda(), shift=op["c1_shift"].cuda())
        if src == "spec64":
            c1.update(spec64=(op["x"].double() * op["denom"][:, None, None]).cuda(), denom=op["denom"].cuda())
        else:
            c1.update(x32=op["x"].cuda())
        outs = K.conv3x3_fused(None, w3, sc, sh, c1=c1, **kw)
    else:
        x0 = op["x0"].cuda()
        x1 = op["x1"].cuda() if C1 else None
        if split:
            x0, kw["x0_split"] = to_split(x0), True
            if C1:
                x1, kw["x1_split"] = to_split(x1), True
        outs = K.conv3x3_fused(x0, w3, sc, sh, x1=x1, **kw)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs if o is not None]


def digest(outs):
    h = hashlib.sha256()
    for o in outs:
        h.update(np.ascontiguousarray(o).tobytes())
    return {"sha256": h.hexdigest(), "first16": [float(v) for v in outs[0].reshape(-1)[:16]]}


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
        outs = run(case)
        assert all(np.isfinite(o).all() for o in outs), case
        rec[case_id(case)] = digest(outs)
        print(case_id(case), rec[case_id(case)]["sha256"][:16], flush=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(rec, indent=1, sort_keys=True) + "\n")
    print(f"{len(rec)} cases -> {args.out}")


if __name__ == "__main__":
    main()
