#!/usr/bin/env python3
"""Timing of the phase vocoder (ops.phase_vocoder; csrc/vocoder.hip) and of ops.time_stretch / ops.pitch_shift beside the two
transforms they stand between (ops.stft_complex, ops.istft) on one MI355X.

Batch: --clips (256) clips of --samples (64000) random float32 samples already on the device, at the rates --rates (0.9 and 1.1).
Every case is warmed up and then timed --reps times with device events around --inner back-to-back calls; the median per call is
reported with every run beside it (the method of tools/time_istft.py).
  ms              device time of one call (output allocation included, no host synchronise inside)
  one_pass_bytes  every operand read once and every result written once (spectrum 16 bytes per bin in and out, samples 4)
  gbs             one_pass_bytes / ms: ACHIEVED rate against that byte count, not a traffic measurement
Cases: stft_complex and istft (for scale), then per rate: phase_vocoder with the rates already on the device (the kernel alone),
time_stretch (stft_complex + phase_vocoder + istft + the crop) and pitch_shift by the ratio 1 / rate (time_stretch + resample).
time_stretch and pitch_shift draw their lengths on the host first: their times include the gaps that leaves on the device.
Prints one JSON line.

Usage:  python tools/time_vocoder.py [--clips 256] [--samples 64000] [--rates 0.9 1.1] [--reps 7] [--inner 50]
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
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--samples", type=int, default=64000)
    ap.add_argument("--rates", type=float, nargs="+", default=[0.9, 1.1])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_vocoder.py measures on the MI355X: no GPU, no number")
    dev = torch.device("cuda:0")
    B, T = args.clips, args.samples
    nF = ops.stft_frames(T)
    gen = torch.Generator(device=dev)
    gen.manual_seed(T)
    x = torch.rand((B, T), generator=gen, device=dev) * 2 - 1
    spec = ops.stft_complex(x)
    bins = B * ops.N_BINS * nF
    wav_bytes, spec_bytes = B * T * 4, bins * 16
    cases = [("stft_complex", lambda: ops.stft_complex(x), wav_bytes + spec_bytes),
             ("istft", lambda: ops.istft(spec, T), spec_bytes + wav_bytes)]
    for rate in args.rates:
        n_out = ops.vocoder_frames(nF, rate)
        out_bytes = B * ops.N_BINS * n_out * 16
        L = int(round(T / rate))
        rates_d = torch.full((B,), rate, dtype=torch.float64, device=dev)
        ratio = Fraction(1 / rate).limit_denominator(16)
        cases += [
            (f"phase_vocoder rate {rate}", lambda r=rates_d, n=n_out: ops.phase_vocoder(spec, r, ld_out=n)[0], spec_bytes + out_bytes),
            (f"time_stretch rate {rate}", lambda r=rate: ops.time_stretch(x, r)[0], wav_bytes + B * L * 4),
            (f"pitch_shift ratio {ratio}", lambda f=ratio: ops.pitch_shift(x, f), 2 * wav_bytes),
        ]
    out = {"clips": B, "samples": T, "frames": nF, "reps": args.reps, "inner": args.inner, "cases": []}
    for name, fn, nbytes in cases:
        ms, runs, y = timed(fn, args.reps, args.inner)
        out["cases"].append({"case": name, "ms": round(ms, 4), "runs_ms": runs, "one_pass_bytes": nbytes,
                             "gbs": round(nbytes / (ms * 1e-3) / 1e9, 1), "checksum": float(torch.view_as_real(y).double().abs().mean())
                             if y.is_complex() else float(y.double().abs().mean())})
    out["gpu"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
