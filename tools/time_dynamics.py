#!/usr/bin/env python3
"""Timing of the dynamic range compressor (ops.compressor, ops.envelope_follow; csrc/dynamics.hip) on one MI355X.

Batches: --clips (64 and 256) clips of --samples (64000) float32 samples already on the device: a gated tone with noise, so that the
detector attacks and releases.  Every case is warmed up and then timed in --reps (7) windows of --inner (5) back-to-back calls
between device events; the median per call is reported with every window beside it (the method of tools/time_iir.py).
  ms              device time of one call
  one_pass_bytes  every sample read once and written once (4 bytes each way)
  gbs             one_pass_bytes / ms: ACHIEVED rate against that byte count, not a traffic measurement
Cases per batch, in one process on the same tensor:
  launch full / level-in      mfpa_dynamics alone, parameters already on the device, one set for the batch and one per row
  ops.compressor / envelope   the whole op: parameters checked on the host and uploaded, output allocated, then the launch
  ops.sosfilt S=2             the neighbour: csrc/iir.hip, one wavefront per row, two second-order sections, comparable serial work
Then the Compressor transform (p = 1: host draws, B parameter rows, one launch) on the first batch.  Prints one JSON line.

Usage:  python tools/time_dynamics.py [--clips 64 256] [--samples 64000] [--reps 7] [--inner 5]
"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from musicfpaugment_amd import ops  # noqa: E402
from musicfpaugment_amd._lib import check, lib, ptr, stream  # noqa: E402
from musicfpaugment_amd.functional import biquad_coefficients, compressor_params  # noqa: E402


def timed(fn, reps, inner):
    for _ in range(2):
        y = fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            y = fn()
        e1.record()
        torch.cuda.synchronize()
        runs.append(e0.elapsed_time(e1) / inner)
    return float(np.median(runs)), [round(r, 4) for r in runs], y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--samples", type=int, default=64000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_dynamics.py measures on the MI355X: no GPU, no number")
    dev = torch.device("cuda:0")
    T = args.samples
    out = {"samples": T, "reps": args.reps, "inner": args.inner, "cases": []}

    def add(B, name, fn, nbytes):
        ms, runs, y = timed(fn, args.reps, args.inner)
        out["cases"].append({"clips": B, "case": name, "ms": round(ms, 4), "runs_ms": runs, "one_pass_bytes": nbytes,
                             "gbs": round(nbytes / (ms * 1e-3) / 1e9, 1), "checksum": float(y.double().abs().mean())})

    gen = torch.Generator(device=dev)
    gen.manual_seed(T)
    t = torch.arange(T, device=dev, dtype=torch.float64) / 8000.0
    for B in args.clips:
        tone = torch.sin(2 * np.pi * 220.0 * t) * (torch.sin(2 * np.pi * 3.0 * t + 0.4) >= 0)
        x = (0.8 * tone[None, :] + 0.05 * torch.randn((B, T), generator=gen, device=dev, dtype=torch.float64)).float().contiguous()
        nbytes = 2 * B * T * 4
        shared = compressor_params(8000, -20.0, 4.0, 5.0, 100.0, 6.0, 3.0)
        per_row = compressor_params(8000, np.linspace(-30.0, -10.0, B), np.linspace(2.0, 10.0, B), np.linspace(1.0, 20.0, B),
                                    np.linspace(50.0, 300.0, B), 6.0, 0.0)
        level = ops.compressor(x, shared, return_gain_reduction=True)[1].contiguous()
        y = torch.empty_like(x)
        for tag, q in (("shared", shared), ("per-row", per_row)):
            q_d = torch.from_numpy(q).to(dev)

            def launch(src, level_in, q_d=q_d, rows=int(q.ndim == 2)):
                check(lib().mfpa_dynamics(ptr(src), 0, B, T, ptr(q_d), rows, 0, 0, 0, level_in, ptr(y), 0, stream()), "mfpa_dynamics")
                return y

            add(B, f"launch full {tag}", lambda: launch(x, 0), nbytes)
            add(B, f"launch level-in {tag}", lambda: launch(level, 1), nbytes)
            add(B, f"ops.compressor {tag}", lambda q=q: ops.compressor(x, q), nbytes)
            add(B, f"ops.envelope_follow {tag}", lambda q=q: ops.envelope_follow(level, q[..., 3], q[..., 4]), nbytes)
        sos = ops.sos_normalized(np.stack([biquad_coefficients("lowshelf", 8000, 200.0, 0.707, 4.0),
                                           biquad_coefficients("peaking", 8000, 1000.0, 1.0, -3.0)]))
        add(B, "ops.sosfilt S=2 shared (csrc/iir.hip: one wavefront per row)", lambda: ops.sosfilt(x, sos), nbytes)

    from musicfpaugment_amd.augmentation.transformations.dynamics import Compressor
    comp = Compressor(p=1.0, sample_rate=8000)
    wav = x[:args.clips[0], None, :].contiguous()
    B = wav.shape[0]

    def transform():
        random.seed(0)
        torch.manual_seed(0)
        return comp(wav).samples

    add(B, "Compressor p=1", transform, 2 * B * T * 4)
    out["gpu"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
