#!/usr/bin/env python3
"""Timing of the lossy-coding kernels (ops.transform_codec, ops.mu_law; csrc/codec.hip) on one MI355X.

Batches: --clips (64 and 256) clips of --samples (64000) float32 samples already on the device, uniform noise.  Every case is
warmed up and then timed in --reps (7) windows of --inner (5) back-to-back calls between device events; the median per call is
reported with every window beside it (the method of tools/time_iir.py).
  ms              device time of one call
  one_pass_bytes  every sample read once and written once (4 bytes each way; the int32 codes of the encoder likewise)
  gbs             one_pass_bytes / ms: ACHIEVED rate against that byte count, not a traffic measurement
Cases per batch, in one process on the same tensor:
  ops.transform_codec            at 8 and 64 kbit/s and lossless (math.inf: no allocation, no quantiser), and at 8 kbit/s with the
                                 water lines and counts returned
  ops.stft_complex + ops.istft   for scale: the same amount of transform work (512-sample frames at hop 256, there and back)
                                 without the allocation, through a complex128 spectrum in memory
  ops.mu_law                     the round trip in one pass; ops.mu_law_encode and ops.mu_law_decode on their own
Then the LossyCodec and TelephoneChannel transforms (p = 1: host draws, one launch; the telephone's band-pass taps and filter
before the compander) beside the Compose of the eight AugmentFP stages, on the first batch.  Prints one JSON line.

Usage:  python tools/time_codec.py [--clips 64 256] [--samples 64000] [--reps 7] [--inner 5]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import random
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
    ap.add_argument("--clips", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--samples", type=int, default=64000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_codec.py measures on the MI355X: no GPU, no number")
    dev = torch.device("cuda:0")
    T = args.samples
    out = {"samples": T, "reps": args.reps, "inner": args.inner, "cases": []}

    def add(B, name, fn, nbytes):
        ms, runs, y = timed(fn, args.reps, args.inner)
        out["cases"].append({"clips": B, "case": name, "ms": round(ms, 4), "runs_ms": runs, "one_pass_bytes": nbytes,
                             "gbs": round(nbytes / (ms * 1e-3) / 1e9, 1), "checksum": float(y.double().abs().mean())})

    gen = torch.Generator(device=dev)
    gen.manual_seed(T)
    for B in args.clips:
        x = torch.rand((B, T), generator=gen, device=dev) * 2 - 1
        nbytes = 2 * B * T * 4
        for kbps in (8.0, 64.0, math.inf):
            add(B, f"ops.transform_codec {kbps:g} kbit/s", lambda k=kbps: ops.transform_codec(x, k), nbytes)
        add(B, "ops.transform_codec 8 kbit/s, return_stats", lambda: ops.transform_codec(x, 8.0, return_stats=True)[0], nbytes)
        add(B, "ops.stft_complex", lambda: torch.view_as_real(ops.stft_complex(x)), nbytes // 2)
        spec = ops.stft_complex(x)
        add(B, "ops.istft", lambda: ops.istft(spec, T), nbytes // 2)
        add(B, "ops.stft_complex + ops.istft", lambda: ops.istft(ops.stft_complex(x), T), nbytes)
        del spec
        add(B, "ops.mu_law 256 (round trip)", lambda: ops.mu_law(x, 256), nbytes)
        add(B, "ops.mu_law_encode 256", lambda: ops.mu_law_encode(x, 256), nbytes)
        codes = ops.mu_law_encode(x, 256)
        add(B, "ops.mu_law_decode 256", lambda: ops.mu_law_decode(codes, 256), nbytes)
        del codes

    from musicfpaugment_amd.augmentation import synthetic_banks
    from musicfpaugment_amd.augmentation.composition import Compose
    from musicfpaugment_amd.augmentation.constants import DEFAULT_PARAMETERS as P
    from musicfpaugment_amd.augmentation.transformations.background_noise import AddBackgroundNoise
    from musicfpaugment_amd.augmentation.transformations.clipping import Clipping
    from musicfpaugment_amd.augmentation.transformations.codec import LossyCodec, TelephoneChannel
    from musicfpaugment_amd.augmentation.transformations.gain import Gain
    from musicfpaugment_amd.augmentation.transformations.impulse_response import ApplyImpulseResponse
    from musicfpaugment_amd.augmentation.transformations.pass_filters import HighPassFilter, LowPassFilter
    from musicfpaugment_amd.augmentation.transformations.peak_normalization import PeakNormalization
    irs, noises = synthetic_banks(0)
    chain = Compose([
        HighPassFilter(P["min_cutoff_freq1"], P["max_cutoff_freq1"], p=P["proba_cutoff_freq1"], sample_rate=8000),
        ApplyImpulseResponse(None, 8000, p=P["proba_ir_response"], ir_bank=irs, device=dev),
        AddBackgroundNoise(None, P["min_snr_in_db"], P["max_snr_in_db"], p=P["proba_snr_in_db"], sample_rate=8000, noise_bank=noises, device=dev),
        Gain(P["min_gain_in_db"], P["max_gain_in_db"], p=P["proba_gain_in_db"]),
        Clipping(0.0, P["max_percentile_threshold"], p=P["proba_percentile_threshold"]),
        LowPassFilter(P["min_cutoff_freq2"], P["max_cutoff_freq2"], p=P["proba_cutoff_freq2"], sample_rate=8000),
        HighPassFilter(P["min_cutoff_freq3"], P["max_cutoff_freq3"], p=P["proba_cutoff_freq3"], sample_rate=8000),
        PeakNormalization(p=1.0)])
    B = args.clips[0]
    wav = (torch.rand((B, T), generator=gen, device=dev) * 2 - 1)[:, None, :]

    def seeded(fn):
        def run():
            random.seed(0)
            torch.manual_seed(0)
            return fn()
        return run

    codec, phone = LossyCodec(p=1.0, sample_rate=8000), TelephoneChannel(p=1.0, sample_rate=8000)
    add(B, "LossyCodec p=1", seeded(lambda: codec(wav).samples), 2 * B * T * 4)
    add(B, "TelephoneChannel p=1", seeded(lambda: phone(wav).samples), 2 * B * T * 4)
    add(B, "Compose of the eight AugmentFP stages", seeded(lambda: chain(wav, 8000).samples), 2 * B * T * 4)
    out["gpu"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
