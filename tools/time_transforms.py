#!/usr/bin/env python3
"""Timing of the composable device transforms (csrc/transforms.hip, augmentation.transformations, augmentation.composition) on one
MI355X.  B = --batch (64) clips of --samples (64000), everything already on the device.

  colored_noise    ops.colored_noise (one mfpa_colored_noise launch) for N = 8000 and 16000; beside it, FOR INFORMATION, the same
                   noise made with torch.fft on the same device (rfft, mask, irfft, RMS, tile) -- several launches and a library FFT
  band_filter      ops.bandpass_taps + one mfpa_fir (band-pass of every clip, cut-offs 0.05 / 0.2 of the sample rate: 161 taps)
  compose          the Compose of the eight AugmentFP stages beside AugmentFP.batch_augment itself, same banks, same seeds (the two
                   make the same draws and launches; the difference is the Python around them)
Each case is warmed up and then timed --reps times with device events around --inner back-to-back calls; the median per call is
reported with every run beside it.  Prints one JSON line.

Usage:  python tools/time_transforms.py [--batch 64] [--samples 64000] [--reps 7] [--inner 5]
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


def timed(fn, reps, inner):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        runs.append(e0.elapsed_time(e1) / inner)
    return {"ms": round(float(np.median(runs)), 4), "runs_ms": [round(r, 4) for r in runs]}


def torch_fft_noise(white, f_decay, T):
    N = white.shape[1]
    mask = 1 / (torch.linspace(1, (N / 2) ** 0.5, N // 2 + 1, device=white.device)[None, :] ** f_decay[:, None])
    x = torch.fft.irfft(torch.fft.rfft(white) * mask, n=N)
    x = x / (x.square().mean(dim=1, keepdim=True).sqrt() + 1e-8)
    return x.repeat(1, -(-T // N))[:, :T]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--samples", type=int, default=64000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_transforms.py measures on the MI355X: no GPU, no number")
    dev = torch.device("cuda:0")
    B, T = args.batch, args.samples
    out = {"B": B, "T": T, "reps": args.reps, "inner": args.inner, "colored_noise": []}
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    for N in (8000, 16000):
        white = torch.randn((B, N), generator=gen, device=dev)
        fd = torch.linspace(-2, 2, B, device=dev)
        ours = timed(lambda: ops.colored_noise(white, fd, T), args.reps, args.inner)
        theirs = timed(lambda: torch_fft_noise(white, fd, T), args.reps, args.inner)
        diff = float((ops.colored_noise(white, fd, T) - torch_fft_noise(white, fd, T)).abs().max())
        out["colored_noise"].append({"N": N, "radices": list(ops.rfft_plan(N)[0]), "mfpa_colored_noise": ours, "torch_fft_for_information": theirs,
                                     "max_abs_difference": diff})
    x = torch.rand((B, T), generator=gen, device=dev) * 2 - 1
    on = torch.ones(B, dtype=torch.uint8, device=dev)

    def band():
        taps, off_d, ntaps_d, half_d = ops.bandpass_taps([0.05] * B, [0.2] * B, dev)
        y = torch.empty_like(x)
        check(lib().mfpa_fir(ptr(x), B, T, T, ptr(taps), ptr(off_d), ptr(ntaps_d), ptr(half_d), ptr(on), 0, 0, ptr(y), 0, stream()), "mfpa_fir")
        return y

    out["band_filter"] = dict(taps=2 * int(8 / 0.05 / 2) + 1, **timed(band, args.reps, args.inner))

    from musicfpaugment_amd.augmentation import AugmentFP, synthetic_banks
    from musicfpaugment_amd.augmentation.composition import Compose
    from musicfpaugment_amd.augmentation.constants import DEFAULT_PARAMETERS as P
    from musicfpaugment_amd.augmentation.transformations.background_noise import AddBackgroundNoise
    from musicfpaugment_amd.augmentation.transformations.clipping import Clipping
    from musicfpaugment_amd.augmentation.transformations.gain import Gain
    from musicfpaugment_amd.augmentation.transformations.impulse_response import ApplyImpulseResponse
    from musicfpaugment_amd.augmentation.transformations.pass_filters import HighPassFilter, LowPassFilter
    from musicfpaugment_amd.augmentation.transformations.peak_normalization import PeakNormalization
    irs, noises = synthetic_banks(0)
    af = AugmentFP(None, 8000, ir_bank=irs, noise_bank=noises, device=dev)
    chain = Compose([
        HighPassFilter(P["min_cutoff_freq1"], P["max_cutoff_freq1"], p=P["proba_cutoff_freq1"], sample_rate=8000),
        ApplyImpulseResponse(None, 8000, p=P["proba_ir_response"], ir_bank=irs, device=dev),
        AddBackgroundNoise(None, P["min_snr_in_db"], P["max_snr_in_db"], p=P["proba_snr_in_db"], sample_rate=8000, noise_bank=noises, device=dev),
        Gain(P["min_gain_in_db"], P["max_gain_in_db"], p=P["proba_gain_in_db"]),
        Clipping(0.0, P["max_percentile_threshold"], p=P["proba_percentile_threshold"]),
        LowPassFilter(P["min_cutoff_freq2"], P["max_cutoff_freq2"], p=P["proba_cutoff_freq2"], sample_rate=8000),
        HighPassFilter(P["min_cutoff_freq3"], P["max_cutoff_freq3"], p=P["proba_cutoff_freq3"], sample_rate=8000),
        PeakNormalization(p=1.0)])
    wav = x[:, None, :]

    def seeded(fn):
        def run():
            random.seed(0)
            torch.manual_seed(0)
            return fn()
        return run

    a = seeded(lambda: af.batch_augment(wav))()
    b = seeded(lambda: chain(wav, 8000).samples)()
    out["compose"] = {"bit_identical": bool(torch.equal(a, b)),
                      "AugmentFP.batch_augment": timed(seeded(lambda: af.batch_augment(wav)), args.reps, args.inner),
                      "Compose": timed(seeded(lambda: chain(wav, 8000)), args.reps, args.inner)}
    out["gpu"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
