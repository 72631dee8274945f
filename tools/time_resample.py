#!/usr/bin/env python3
"""Timing of the device resampler (ops.resample, csrc/resample.hip) on one MI355X.

Cases: --tracks (256) clips of --seconds (30) at 44.1 kHz -> 8 kHz and the same batch at 16 kHz -> 8 kHz, random float32 samples
already on the device.  Each case is warmed up (the tap bank is built and uploaded there) and then timed --reps times with device
events around --inner back-to-back calls; the median per call is reported with every run beside it.
  ms            device time of one ops.resample call (output allocation included, no host synchronise inside)
  tracks_per_s  tracks / ms
  one_pass_bytes (B * T + B * Tout) * 4: every input sample read once, every output sample written once
  gbs           one_pass_bytes / ms: ACHIEVED rate against that byte count, not a traffic measurement
  gflops        2 * B * Tout * taps-per-phase / ms (the multiply-adds of the filter, zeros at the clip edges included)
Prints one JSON line.

Usage:  python tools/time_resample.py [--tracks 256] [--seconds 30] [--reps 7] [--inner 5]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from musicfpaugment_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_resample.py measures on the MI355X: no GPU, no number")
    dev = torch.device("cuda:0")
    out = {"tracks": args.tracks, "seconds": args.seconds, "reps": args.reps, "inner": args.inner, "cases": []}
    for orig, new in ((44100, 8000), (16000, 8000)):
        B, T = args.tracks, int(round(args.seconds * orig))
        gen = torch.Generator(device=dev)
        gen.manual_seed(orig)
        x = torch.rand((B, T), generator=gen, device=dev) * 2 - 1
        o, n, width, ntaps, Tout = ops.resample_geometry(orig, new, T)
        for _ in range(2):
            y = ops.resample(x, orig, new)
        torch.cuda.synchronize()
        runs = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.inner):
                y = ops.resample(x, orig, new)
            e1.record()
            torch.cuda.synchronize()
            runs.append(e0.elapsed_time(e1) / args.inner)
        ms = float(np.median(runs))
        nbytes = (B * T + B * Tout) * 4
        out["cases"].append({"orig_freq": orig, "new_freq": new, "B": B, "T": T, "Tout": Tout, "o": o, "n": n, "taps_per_phase": ntaps,
                             "tile_frames": ops.resample_tile(orig, new), "ms": round(ms, 4), "runs_ms": [round(r, 4) for r in runs],
                             "tracks_per_s": round(B / (ms * 1e-3), 1), "one_pass_bytes": nbytes,
                             "gbs": round(nbytes / (ms * 1e-3) / 1e9, 1), "gflops": round(2.0 * B * Tout * ntaps / (ms * 1e-3) / 1e9, 1),
                             "checksum": float(y.double().abs().mean())})
        del x, y
    out["gpu"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
