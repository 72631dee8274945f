#!/usr/bin/env python3
"""Timing of the recursive filters (ops.sosfilt; csrc/iir.hip) and of the ParametricEQ transform on one MI355X.

Batches: --clips (64 and 256) clips of --samples (64000) random float32 samples already on the device.  Every case is warmed up and
then timed --reps times with device events around --inner back-to-back calls; the median per call is reported with every run beside
it (the method of tools/time_vocoder.py).
  ms              device time of one call
  one_pass_bytes  every sample read once and written once (4 bytes each way)
  gbs             one_pass_bytes / ms: ACHIEVED rate against that byte count, not a traffic measurement
Cases per batch, for S = 1 and S = 7 sections, with one filter for the batch and with one per row:
  launch          mfpa_sosfilt alone (the setup launch of the powers and the filter launch), sections and work already on the device
  ops.sosfilt     the whole op: the sections normalised on the host and uploaded, output and work allocated, then the launch
and, for scale, the band-pass of every clip by ops.bandpass_taps + one mfpa_fir (cut-offs 0.05 / 0.2 of the sample rate: 161 taps).
Then ParametricEQ (p = 1, seven bands: host draws, 7 B cookbook designs, one launch) beside the Compose of the eight AugmentFP
stages on the 64-clip batch.  Prints one JSON line.

Usage:  python tools/time_iir.py [--clips 64 256] [--samples 64000] [--reps 7] [--inner 20]
"""
from __future__ import annotations

import argparse
import ctypes
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


def sections(S: int, rows: int) -> np.ndarray:
    """(rows, S, 6): a low shelf, peaking bands and a high shelf like ParametricEQ's, the gains varying with the row."""
    centers = np.geomspace(60.0, 3200.0, max(S, 2))
    out = np.empty((rows, S, 6))
    for b in range(rows):
        for s in range(S):
            kind = "peaking" if S == 1 else "lowshelf" if s == 0 else "highshelf" if s == S - 1 else "peaking"
            out[b, s] = biquad_coefficients(kind, 8000, centers[s], 0.707 if kind != "peaking" else 1.0, 6.0 * np.cos(b + 2.0 * s))
    return ops.sos_normalized(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--samples", type=int, default=64000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_iir.py measures on the MI355X: no GPU, no number")
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
        on = torch.ones(B, dtype=torch.uint8, device=dev)

        def band():
            taps, off_d, ntaps_d, half_d = ops.bandpass_taps([0.05] * B, [0.2] * B, dev)
            y = torch.empty_like(x)
            check(lib().mfpa_fir(ptr(x), B, T, T, ptr(taps), ptr(off_d), ptr(ntaps_d), ptr(half_d), ptr(on), 0, 0, ptr(y), 0, stream()), "mfpa_fir")
            return y

        add(B, "band-pass: bandpass_taps + mfpa_fir, 161 taps", band, nbytes)
        for S in (1, 7):
            for per_row in (0, 1):
                sos = sections(S, B if per_row else 1)
                sos = sos if per_row else sos[0]
                sos_d = torch.from_numpy(sos).to(dev)
                need = ctypes.c_longlong(0)
                check(lib().mfpa_sosfilt_work(B, S, per_row, ctypes.addressof(need)), "mfpa_sosfilt_work")
                work = torch.empty((need.value,), dtype=torch.float64, device=dev)
                y = torch.empty_like(x)

                def launch(sos_d=sos_d, work=work, y=y, S=S, per_row=per_row, n=need.value):
                    check(lib().mfpa_sosfilt(ptr(x), 0, B, T, ptr(sos_d), S, per_row, 0, 0, 0, 0, ptr(work), n, ptr(y), stream()), "mfpa_sosfilt")
                    return y

                tag = f"S={S} {'per-row' if per_row else 'shared'}"
                add(B, f"launch {tag}", launch, nbytes)
                add(B, f"ops.sosfilt {tag}", lambda sos=sos: ops.sosfilt(x, sos), nbytes)

    from musicfpaugment_amd.augmentation import synthetic_banks
    from musicfpaugment_amd.augmentation.composition import Compose
    from musicfpaugment_amd.augmentation.constants import DEFAULT_PARAMETERS as P
    from musicfpaugment_amd.augmentation.transformations.background_noise import AddBackgroundNoise
    from musicfpaugment_amd.augmentation.transformations.clipping import Clipping
    from musicfpaugment_amd.augmentation.transformations.equalizer import ParametricEQ
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
    eq = ParametricEQ(p=1.0, sample_rate=8000)
    B = args.clips[0]
    wav = (torch.rand((B, T), generator=gen, device=dev) * 2 - 1)[:, None, :]

    def seeded(fn):
        def run():
            random.seed(0)
            torch.manual_seed(0)
            return fn()
        return run

    add(B, "ParametricEQ p=1, 7 bands", seeded(lambda: eq(wav).samples), 2 * B * T * 4)
    add(B, "Compose of the eight AugmentFP stages", seeded(lambda: chain(wav, 8000).samples), 2 * B * T * 4)
    out["gpu"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
