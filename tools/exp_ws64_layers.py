#!/usr/bin/env python3
"""The six launches of the eval chain that conv_ws64_kernel serves at the headline shape (257 x 251, bf16x3, decoder levels folded), each
as ops_unet.unet_forward_eval issues it -- scale-folded fragment image, split-layout edges as unet_plan() chooses them:
inc (first layer in the loaders + pool), up4.3 (+ OutConv, no store), down1.0, down1.3 (+ pool), up3.3, down2.0.
us per launch, `--readings` readings of `--reps` launches each.  usage: exp_ws64_layers.py [--lib PATH] [--clips N] [--reps N] [--readings N]"""
import argparse, importlib.util, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None)
ap.add_argument("--clips", type=int, default=128)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--readings", type=int, default=2)
args = ap.parse_args()
if args.lib:
    from musicfpaugment_amd import _lib
    _lib.set_library_path(args.lib)
from musicfpaugment_amd import ops_unet as K
spec = importlib.util.spec_from_file_location("record_ws64_bits", os.path.join(ROOT, "tools", "record_ws64_bits.py"))
REC = importlib.util.module_from_spec(spec)
spec.loader.exec_module(REC)
B = args.clips
g = torch.Generator(device="cuda").manual_seed(5)
rn = lambda *s: torch.randn(*s, device="cuda", generator=g)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.reps * 1e3


def layer(name, H, W, cin, cout, **kw):
    """One launch: activations relu(randn) (split where the chain hands them over split), weights randn / sqrt(9 cin), scale folded."""
    w = rn(9, cout, cin) / (9 * cin) ** 0.5
    sc, sh = torch.rand(cout, device="cuda", generator=g) + 0.5, rn(cout) * 0.1
    w3, wf, wff = K.split_bf16x3(w), (2, K.split_bf16x3_frag(w, 2)), (2, K.split_bf16x3_frag(w * sc[None, :, None], 2))
    assert K.conv_route(H, W, cin, cout, 2, c1="c1" in kw, out1x1="out1x1" in kw)[2], name
    x = None
    if "c1" not in kw:
        x = torch.relu(rn(B, H, W, cin))
        if kw.get("x0_split"):
            x = REC.to_split(x)
    return name, lambda: K.conv3x3_fused(x, w3, sc, sh, precision=1, wf=wf, wff=wff, **kw)


c1 = dict(spec64=torch.rand(B, 257, 251, device="cuda", dtype=torch.float64, generator=g), denom=torch.ones(B, device="cuda", dtype=torch.float64),
          w=rn(9, 64) / 3.0, scale=torch.rand(64, device="cuda", generator=g) + 0.5, shift=rn(64) * 0.2)
LAYERS = [layer("inc     1(->64)->64 @257x251 c1src + pool", 257, 251, 64, 64, c1=c1, pool=True, pool_split=True),
          layer("up4.3   64-> 64 @257x251 + OutConv, no store", 257, 251, 64, 64, out1x1=(rn(64), 0.1), store=False),
          layer("down1.0 64->128 @128x125 split in, split out", 128, 125, 64, 128, x0_split=True, y_split=True),
          layer("down1.3 128->128 @128x125 split in, + pool", 128, 125, 128, 128, x0_split=True, pool=True, pool_split=True),
          layer("up3.3   128->128 @128x125", 128, 125, 128, 128),
          layer("down2.0 128->256 @64x62 split in", 64, 62, 128, 256, x0_split=True)]
print(f"# {B} clips, {args.readings} readings of {args.reps} launches each; us per launch")
tot = [0.0] * args.readings
for name, fn in LAYERS:
    for _ in range(args.reps): fn()                                  # an untimed reading first: caches, clocks
    torch.cuda.synchronize()
    r = [timed(fn) for _ in range(args.readings)]
    tot = [a + b for a, b in zip(tot, r)]
    print(f"{name:48s} " + "  ".join(f"{v:8.1f}" for v in r))
print(f"{'sum':48s} " + "  ".join(f"{v:8.1f}" for v in tot))
