#!/usr/bin/env python3
"""Timing of the loudness meter (ops.loudness*, csrc/loudness.hip) on one MI355X.

Shapes: --clips (64 and 256) mono clips of --samples (64000) random float32 samples at 8 kHz, and --tracks (64) mono tracks of
--track-samples (1 920 000).  Every case is warmed up and then timed --reps times with device events around --inner back-to-back
calls; the median per call is reported with every run beside it (the method of tools/time_iir.py).
Cases per shape:
  segments launch        mfpa_loudness_segments alone (the setup launch of the powers and the meter launch), sections on the device
  gate launch            mfpa_loudness_gate alone on those segment sums
  ops.loudness           the whole op: design, upload, segments, gate, log10
  ops.loudness_normalize the meter, the gain and the multiply
and the yardsticks, what the library offered before for the same figures, in the same process:
  sosfilt launch S=2     mfpa_sosfilt with the same two sections: the same serial chain, plus the store of the filtered signal
  ops.sosfilt + torch    ops.sosfilt, then torch's square and segment sums
Prints one JSON line.

Usage:  python tools/time_loudness.py [--clips 64 256] [--samples 64000] [--tracks 64] [--track-samples 1920000] [--reps 7] [--inner 10]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from musicfpaugment_amd import ops  # noqa: E402
from musicfpaugment_amd._lib import check, lib, ptr, stream  # noqa: E402
from musicfpaugment_amd.functional import k_weighting_sos  # noqa: E402


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
    ap.add_argument("--tracks", type=int, default=64)
    ap.add_argument("--track-samples", type=int, default=1920000)
    ap.add_argument("--rate", type=int, default=8000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_loudness.py measures on the MI355X: no GPU, no number")
    dev = torch.device("cuda:0")
    fs, hop = args.rate, ops.loudness_hop(args.rate)
    sos = k_weighting_sos(fs)
    sos_d = torch.from_numpy(sos).to(dev)
    out = {"rate": fs, "hop": hop, "reps": args.reps, "inner": args.inner, "cases": []}
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    shapes = [(B, args.samples) for B in args.clips] + ([(args.tracks, args.track_samples)] if args.tracks else [])
    for B, T in shapes:
        x = (torch.rand((B, T), generator=gen, device=dev) * 2 - 1) * 0.3
        nseg = T // hop

        def add(name, fn):
            ms, runs, y = timed(fn, args.reps, args.inner)
            out["cases"].append({"rows": B, "samples": T, "case": name, "ms": round(ms, 4), "runs_ms": runs,
                                 "checksum": float(y.double().abs().mean())})

        work = torch.empty((512,), dtype=torch.float64, device=dev)
        seg = torch.empty((B, nseg), dtype=torch.float64, device=dev)
        y = torch.empty_like(x)
        need = ctypes.c_longlong(0)
        check(lib().mfpa_sosfilt_work(B, 2, 0, ctypes.addressof(need)), "mfpa_sosfilt_work")

        def segments():
            check(lib().mfpa_loudness_segments(ptr(x), 0, B, T, ptr(sos_d), 2, hop, ptr(work), 512, ptr(seg), 0, stream()), "mfpa_loudness_segments")
            return seg

        def sosfilt():
            check(lib().mfpa_sosfilt(ptr(x), 0, B, T, ptr(sos_d), 2, 0, 0, 0, 0, 0, ptr(work), need.value, ptr(y), stream()), "mfpa_sosfilt")
            return y

        def before():
            f = ops.sosfilt(x, sos).double()
            return (f * f)[:, :nseg * hop].reshape(B, nseg, hop).sum(dim=2)

        power = torch.zeros((B, 2), dtype=torch.float64, device=dev)
        counts = torch.zeros((B, 2), dtype=torch.int32, device=dev)

        def gate():
            check(lib().mfpa_loudness_gate(ptr(seg), B, 1, nseg, hop, 4, 0, ops.loudness_power(-70.0), 0.1, ptr(power), ptr(counts), 0, 0, stream()),
                  "mfpa_loudness_gate")
            return power

        add("sosfilt launch S=2 (yardstick)", sosfilt)
        add("segments launch", segments)
        add("gate launch", gate)
        add("ops.sosfilt + torch square and segment sums (yardstick)", before)
        add("ops.loudness", lambda: ops.loudness(x, fs))
        add("ops.loudness_normalize", lambda: ops.loudness_normalize(x, fs, -23.0))
        if B == shapes[0][0] and T == shapes[0][1]:
            add("ops.loudness_range", lambda: ops.loudness_range(x, fs))
    out["gpu"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
