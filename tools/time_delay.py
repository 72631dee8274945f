#!/usr/bin/env python3
"""Timing of the delay lines (ops.variable_delay, ops.comb; csrc/delay.hip) on one MI355X.

Batches: --clips (64 and 256) clips of --samples (64000) float32 samples already on the device, uniform noise.  Every case is
warmed up and then timed in --reps (7) windows of --inner (5) back-to-back calls between device events; the median per call is
reported with every window beside it (the method of tools/time_iir.py).
  ms              device time of one call
  one_pass_bytes  every sample read once and written once (4 bytes each way); for a (B, V, T) delay tensor its 8 bytes per voice
                  and sample are counted too
  gbs             one_pass_bytes / ms: ACHIEVED rate against that byte count, not a traffic measurement
  gtaps           for ops.variable_delay: B T V (filter_len + 1) taps per call over ms, in 1e9 taps per second
Cases per batch, in one process on the same tensor:
  ops.variable_delay   V = 1 and 3, filter_len 33 and 81, on a smooth LFO delay already on the device (every tile staged in LDS),
                       on uniformly random delays in [-T, T] (every tile reads global memory), and V = 3 constant voices (B, V):
                       an echo, no delay tensor
  ops.comb             D = 1, 64 and 2000 (1, 64 and 2000 lanes per row); at D = 1 and 2000 also with no row selected, which is the
                       copy of an unselected row on the grid that D sizes (256 and 2048 lanes per row)
  band-pass            for scale: ops.bandpass_taps + one mfpa_fir, 161 taps
  ops.sosfilt S=1      for scale: csrc/iir.hip, one wavefront per row
Then the Echo, Echo(feedback=True), WowFlutter and Chorus transforms (p = 1: host draws, the delay tensor built on the device, one
launch) on the first batch.  Prints one JSON line.

Usage:  python tools/time_delay.py [--clips 64 256] [--samples 64000] [--reps 7] [--inner 5]
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
from musicfpaugment_amd.functional import biquad_coefficients  # noqa: E402


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
        raise SystemExit("time_delay.py measures on the MI355X: no GPU, no number")
    dev = torch.device("cuda:0")
    T = args.samples
    out = {"samples": T, "reps": args.reps, "inner": args.inner, "cases": []}

    def add(B, name, fn, nbytes, taps=None):
        ms, runs, y = timed(fn, args.reps, args.inner)
        case = {"clips": B, "case": name, "ms": round(ms, 4), "runs_ms": runs, "one_pass_bytes": nbytes,
                "gbs": round(nbytes / (ms * 1e-3) / 1e9, 1), "checksum": float(y.double().abs().mean())}
        if taps is not None:
            case["gtaps"] = round(taps / (ms * 1e-3) / 1e9, 1)
        out["cases"].append(case)

    gen = torch.Generator(device=dev)
    gen.manual_seed(T)
    for B in args.clips:
        x = torch.rand((B, T), generator=gen, device=dev) * 2 - 1
        nbytes = 2 * B * T * 4
        on = torch.ones(B, dtype=torch.uint8, device=dev)
        for V in (1, 3):
            smooth = torch.stack([ops.lfo_delay(B, T, 8000, base_ms=20.0, depth_ms=2.0, rate_hz=0.8, phase=2.0 * np.pi * v / V) for v in range(V)], 1)
            rand = (torch.rand((B, V, T), generator=gen, device=dev, dtype=torch.float64) * 2 - 1) * T
            for taps in (33, 81):
                work = B * T * V * (taps + 1)
                add(B, f"ops.variable_delay V={V} taps={taps} LFO (staged)", lambda d=smooth, n=taps: ops.variable_delay(x, d, 1.0 / V, dry=0.5, filter_len=n),
                    nbytes + B * V * T * 8, work)
                add(B, f"ops.variable_delay V={V} taps={taps} random (direct)", lambda d=rand, n=taps: ops.variable_delay(x, d, 1.0 / V, dry=0.5, filter_len=n),
                    nbytes + B * V * T * 8, work)
            del smooth, rand
        echo = torch.tensor([400.0, 800.5, 1600.25], dtype=torch.float64, device=dev).expand(B, 3)
        add(B, "ops.variable_delay V=3 taps=81 constant voices (B, V)", lambda: ops.variable_delay(x, echo, [0.5, 0.25, 0.125], dry=1.0), nbytes,
            B * T * 3 * 82)
        for D in (1, 64, 2000):
            add(B, f"ops.comb D={D}", lambda D=D: ops.comb(x, D, 1.0, 0.0, 0.5), nbytes)
        off = torch.zeros(B, dtype=torch.uint8, device=dev)
        for D in (1, 2000):                               # no row selected: the copy runs on the grid that D sizes
            add(B, f"ops.comb D={D}, no row selected (copy)", lambda D=D: ops.comb(x, D, 1.0, 0.0, 0.5, apply=off), nbytes)

        def band():
            taps, off_d, ntaps_d, half_d = ops.bandpass_taps([0.05] * B, [0.2] * B, dev)
            y = torch.empty_like(x)
            check(lib().mfpa_fir(ptr(x), B, T, T, ptr(taps), ptr(off_d), ptr(ntaps_d), ptr(half_d), ptr(on), 0, 0, ptr(y), 0, stream()), "mfpa_fir")
            return y

        add(B, "band-pass: bandpass_taps + mfpa_fir, 161 taps", band, nbytes)
        sos = ops.sos_normalized(np.stack([biquad_coefficients("peaking", 8000, 1000.0, 1.0, -3.0)]))
        add(B, "ops.sosfilt S=1 shared (csrc/iir.hip: one wavefront per row)", lambda: ops.sosfilt(x, sos), nbytes)

    from musicfpaugment_amd.augmentation.transformations.delay_effects import Chorus, Echo, WowFlutter
    wav = x[:args.clips[0], None, :].contiguous()
    B = wav.shape[0]
    for name, t in (("Echo p=1", Echo(p=1.0, sample_rate=8000)), ("Echo feedback p=1", Echo(feedback=True, p=1.0, sample_rate=8000)),
                    ("WowFlutter p=1", WowFlutter(p=1.0, sample_rate=8000)), ("Chorus p=1", Chorus(p=1.0, sample_rate=8000))):
        def transform(t=t):
            random.seed(0)
            torch.manual_seed(0)
            return t(wav).samples

        add(B, name, transform, 2 * B * T * 4)
    out["gpu"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
