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

--sparse adds the sparse-tap kernel (ops.resample(..., any_ratio=True) / kernel="sparse") at --tracks clips of --samples (64000)
input samples, under "sparse_cases":
  8979 -> 8000 and 8000 -> 8979, pairs only the sparse kernel takes (ms, gbs as above; taps_per_output is the support S);
  ops.pitch_shift by 8979/8000 (two semitones at 8 kHz, any_ratio=True) beside ops.pitch_shift by 10/9 through the dense kernel;
  44100 -> 8000 and 16000 -> 8000 with the sparse kernel FORCED beside the dense kernel: the two alternate window by window in the
  same process, and "equal" says that their outputs are the same under torch.equal.

Usage:  python tools/time_resample.py [--tracks 256] [--seconds 30] [--reps 7] [--inner 5] [--sparse [--samples 64000]]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from fractions import Fraction

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from musicfpaugment_amd import ops  # noqa: E402


def _windows(fns, reps, inner):
    """Median ms per call of each fn, the fns alternating window by window; -> ([ms], [[runs]], [last result])."""
    last = [None] * len(fns)
    for i, fn in enumerate(fns):
        for _ in range(2):
            last[i] = fn()
    torch.cuda.synchronize()
    runs = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                last[i] = fn()
            e1.record()
            torch.cuda.synchronize()
            runs[i].append(e0.elapsed_time(e1) / inner)
    return [float(np.median(r)) for r in runs], [[round(v, 4) for v in r] for r in runs], last


def _sparse_cases(args, dev):
    B, T = args.tracks, args.samples
    gen = torch.Generator(device=dev)
    gen.manual_seed(T)
    x = torch.rand((B, T), generator=gen, device=dev) * 2 - 1
    cases = []

    def rate(nbytes, ms):
        return round(nbytes / (ms * 1e-3) / 1e9, 1)

    for orig, new in ((8979, 8000), (8000, 8979)):
        o, n, width, S, Tout = ops.resample_sparse_geometry(orig, new, T)
        (ms,), (runs,), (y,) = _windows([lambda: ops.resample(x, orig, new, any_ratio=True)], args.reps, args.inner)
        nbytes = (B * T + B * Tout) * 4
        cases.append({"case": f"sparse {orig} -> {new}", "B": B, "T": T, "Tout": Tout, "o": o, "n": n, "taps_per_output": S,
                      "table_bytes": n * S * 4 + n * 4, "tile_outputs": ops.resample_sparse_tile(orig, new), "ms": round(ms, 4), "runs_ms": runs,
                      "one_pass_bytes": nbytes, "gbs": rate(nbytes, ms), "checksum": float(y.double().abs().mean())})
    fns = [lambda: ops.pitch_shift(x, Fraction(8979, 8000), any_ratio=True), lambda: ops.pitch_shift(x, Fraction(10, 9))]
    ms, runs, ys = _windows(fns, args.reps, args.inner)
    for name, m, r, y in zip(("pitch_shift ratio 8979/8000 (any_ratio)", "pitch_shift ratio 10/9 (dense)"), ms, runs, ys):
        cases.append({"case": name, "B": B, "T": T, "ms": round(m, 4), "runs_ms": r, "one_pass_bytes": 2 * B * T * 4,
                      "gbs": rate(2 * B * T * 4, m), "checksum": float(y.double().abs().mean())})
    for orig, new in ((44100, 8000), (16000, 8000)):
        o, n, width, ntaps, Tout = ops.resample_geometry(orig, new, T)
        S = ops.resample_sparse_geometry(orig, new)[3]
        fns = [lambda: ops.resample(x, orig, new), lambda: ops.resample(x, orig, new, kernel="sparse")]
        ms, runs, ys = _windows(fns, args.reps, args.inner)
        nbytes = (B * T + B * Tout) * 4
        cases.append({"case": f"{orig} -> {new}: dense beside sparse forced", "B": B, "T": T, "Tout": Tout, "taps_per_phase": ntaps,
                      "taps_per_output": S, "dense_ms": round(ms[0], 4), "sparse_ms": round(ms[1], 4), "dense_runs_ms": runs[0],
                      "sparse_runs_ms": runs[1], "one_pass_bytes": nbytes, "dense_gbs": rate(nbytes, ms[0]), "sparse_gbs": rate(nbytes, ms[1]),
                      "equal": bool(torch.equal(ys[0], ys[1]))})
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--sparse", action="store_true")
    ap.add_argument("--samples", type=int, default=64000)
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
    if args.sparse:
        out["samples"] = args.samples
        out["sparse_cases"] = _sparse_cases(args, dev)
    out["gpu"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
