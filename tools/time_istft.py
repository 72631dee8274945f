#!/usr/bin/env python3
"""Timing of the complex STFT and the inverse STFT (ops.stft_complex, ops.istft; csrc/stft.hip, csrc/istft.hip) and of
UNet.denoise_waveform beside UNet.denoise_spectrogram on one MI355X.

Batch: --clips (256) clips of --samples (64000) random float32 samples already on the device.  Every case is warmed up and then
timed --reps times with device events around --inner back-to-back calls (200: some 30 ms per window; --unet-inner, 5, for the two
UNet cases: some 100 ms); the median per call is reported with every run beside it.
  ms              device time of one call (output allocation included, no host synchronise inside)
  one_pass_bytes  every operand read once and every result written once (spectrum 16 bytes per bin, magnitudes 4 or 8, samples 4)
  gbs             one_pass_bytes / ms: ACHIEVED rate against that byte count, not a traffic measurement
Cases: stft_mag (the existing magnitude transform, for scale), stft_complex, stft_complex with magnitudes, istft without and with
float32 / float64 magnitudes; then, with --unet, the formula-weight UNet: stft_mag + denoise_spectrogram (the existing spectrogram path)
and denoise_waveform on the same batch, --unet-clips (32) clips at a time.
Prints one JSON line.

Usage:  python tools/time_istft.py [--clips 256] [--samples 64000] [--reps 7] [--inner 200] [--unet] [--unet-clips 32] [--unet-inner 5]
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--unet", action="store_true")
    ap.add_argument("--unet-clips", type=int, default=32)
    ap.add_argument("--unet-inner", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_istft.py measures on the MI355X: no GPU, no number")
    dev = torch.device("cuda:0")
    B, T = args.clips, args.samples
    nF = ops.stft_frames(T)
    gen = torch.Generator(device=dev)
    gen.manual_seed(T)
    x = torch.rand((B, T), generator=gen, device=dev) * 2 - 1
    spec, mag64, cmax = ops.stft_complex(x, want_mag=True)
    mag32 = mag64.float()
    bins = B * ops.N_BINS * nF
    wav_bytes, spec_bytes = B * T * 4, bins * 16
    cases = [
        ("stft_mag float64", lambda: ops.stft_mag(x)[0], wav_bytes + bins * 8),
        ("stft_complex", lambda: ops.stft_complex(x), wav_bytes + spec_bytes),
        ("stft_complex + float64 magnitudes", lambda: ops.stft_complex(x, want_mag=True)[0], wav_bytes + spec_bytes + bins * 8),
        ("istft", lambda: ops.istft(spec, T), spec_bytes + wav_bytes),
        ("istft, float32 magnitudes", lambda: ops.istft(spec, T, mag=mag32, denom=cmax, clamp=True), spec_bytes + bins * 4 + wav_bytes),
        ("istft, float64 magnitudes", lambda: ops.istft(spec, T, mag=mag64), spec_bytes + bins * 8 + wav_bytes),
    ]
    out = {"clips": B, "samples": T, "frames": nF, "reps": args.reps, "inner": args.inner, "unet_inner": args.unet_inner, "cases": []}
    for name, fn, nbytes in cases:
        ms, runs, y = timed(fn, args.reps, args.inner)
        out["cases"].append({"case": name, "ms": round(ms, 4), "runs_ms": runs, "one_pass_bytes": nbytes,
                             "gbs": round(nbytes / (ms * 1e-3) / 1e9, 1), "checksum": float(torch.view_as_real(y).double().abs().mean())
                             if y.is_complex() else float(y.double().abs().mean())})
    if args.unet:
        from musicfpaugment_amd.training.unet import UNet
        from musicfpaugment_amd.training.weights import formula_state_dict
        net = UNet(1, 1, rate=0.05)
        net.load_state_dict(formula_state_dict(0))
        net = net.to(dev).eval()
        xs = x[:args.unet_clips].contiguous()

        def spectrogram_path():
            m, c = ops.stft_mag(xs)
            return net.denoise_spectrogram(m, c, False)

        for name, fn in (("stft_mag + denoise_spectrogram", spectrogram_path), ("denoise_waveform", lambda: net.denoise_waveform(xs))):
            ms, runs, y = timed(fn, args.reps, args.unet_inner)
            out["cases"].append({"case": name, "clips": args.unet_clips, "ms": round(ms, 4), "runs_ms": runs,
                                 "checksum": float(y.double().abs().mean())})
    out["gpu"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
