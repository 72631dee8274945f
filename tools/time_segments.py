#!/usr/bin/env python3
"""Timing of the segment stage (csrc/segments.hip) and of the AugmentationDataset built on it, on one MI355X.

Input: --tracks (256) tracks of --minutes (4) at 8 kHz, random float32 samples with one gain per 3-s piece (so that the silence
rule drops some), back to back in one device buffer.
  kernels   mfpa_segment_stats (S == L and S == L / 2), mfpa_segment_select, mfpa_segment_gather (n_keep 1 and 8), each warmed up
            and timed --reps times with device events around --inner back-to-back calls (output allocation included, no host
            synchronise inside); the median per call, with every run beside it, against the ONE-PASS byte count of the call:
              stats    the bank once (S == L reads it once; S != L reads it 1 + L / S times, the rate is still quoted on one pass)
              select   the sums, keys and per-row outputs
              gather   rows * L * 4 read + written
            gbs = one_pass_bytes / ms is an ACHIEVED rate against that count, not a traffic measurement.
  dataset   AugmentationDataset(tracks=..., n_segments=1, 3-s chunks).batches(64) with AugmentFP on synthetic banks: wall-clock
            milliseconds per batch over --batches batches, a device synchronise after each (ingest, host draws and the
            augmentation chain included), with the tracks already on the device and with the tracks in host memory (one upload of
            64 tracks per group); and Trainer.train_step (UNet, bf16x3) on such a batch, the consumer it has to keep fed.
Prints one JSON line.

Usage:  python tools/time_segments.py [--tracks 256] [--minutes 4] [--reps 7] [--inner 5] [--batches 12]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from musicfpaugment_amd import ops  # noqa: E402

SR, L = 8000, 24000


def timed(fn, reps, inner):
    for _ in range(2):
        out = fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            out = fn()
        e1.record()
        torch.cuda.synchronize()
        runs.append(e0.elapsed_time(e1) / inner)
    return float(np.median(runs)), [round(r, 4) for r in runs], out


def case(name, ms, runs, nbytes, **extra):
    d = {"name": name, "ms": round(ms, 4), "runs_ms": runs, "one_pass_bytes": int(nbytes), "gbs": round(nbytes / (ms * 1e-3) / 1e9, 1)}
    d.update(extra)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=256)
    ap.add_argument("--minutes", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--batches", type=int, default=12)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_segments.py measures on the MI355X: no GPU, no number")
    dev = torch.device("cuda:0")
    n, N = args.tracks, int(round(args.minutes * 60 * SR))
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    bank = torch.rand((n, N), generator=gen, device=dev) * 2 - 1
    pieces = -(-N // L)
    gains = torch.tensor([1.0, 0.05, 0.0], device=dev)[torch.multinomial(torch.tensor([0.55, 0.3, 0.15], device=dev), n * pieces, True,
                                                                          generator=gen)].reshape(n, pieces)
    bank = (bank * gains.repeat_interleave(L, dim=1)[:, :N]).reshape(-1).contiguous()
    lens = np.full(n, N, dtype=np.int64)
    off = np.arange(n, dtype=np.int64) * N
    off_d, len_d = torch.from_numpy(off).to(dev), torch.from_numpy(lens).to(dev)
    out = {"tracks": n, "minutes": args.minutes, "samples_per_track": N, "L": L, "reps": args.reps, "inner": args.inner, "kernels": []}
    bank_bytes = bank.numel() * 4
    stats = None
    for S in (L, L // 2):
        seg_off = ops.segment_geometry(lens, L, S)
        ns = int(seg_off[-1])
        seg_off_d = torch.from_numpy(seg_off).to(dev)
        ms, runs, res = timed(lambda: ops.segment_stats(bank, off_d, len_d, seg_off_d, ns, L, S), args.reps, args.inner)
        out["kernels"].append(case(f"segment_stats S={S}", ms, runs, bank_bytes, segments=ns, checksum=float(res[1].sum())))
        if S == L:
            stats, seg_off_1, ns_1 = res, seg_off_d, ns
    keys = torch.from_numpy(np.random.default_rng(2).integers(0, 1 << 32, size=ns_1, dtype=np.uint32).view(np.int32)).to(dev)
    for n_keep in (1, 8):
        ms, runs, res = timed(lambda: ops.segment_select(*stats, off_d, len_d, seg_off_1, L, L, keys, -7.5, n_keep), args.reps, args.inner)
        sel, src, div, kept = res
        out["kernels"].append(case(f"segment_select n_keep={n_keep}", ms, runs, ns_1 * 12 + n * 20 + n * n_keep * 16,
                                   kept_mean=float(kept.float().mean()), segments=ns_1))
        rows = int((src >= 0).sum())
        ms, runs, res = timed(lambda: ops.segment_gather(bank, src, div, L), args.reps, args.inner)
        out["kernels"].append(case(f"segment_gather n_keep={n_keep}", ms, runs, rows * L * 8, rows=rows,
                                   note="the zero fill of a fresh output (rows * L * 4 more bytes written) is inside the time"))
        pool = torch.empty((n * n_keep, L), device=dev)
        ms, runs, res = timed(lambda: ops.segment_gather(bank, src, div, L, out=pool), args.reps, args.inner)
        out["kernels"].append(case(f"segment_gather n_keep={n_keep} into a given buffer", ms, runs, rows * L * 8, rows=rows))
        del pool

    # ------------------------------------------------------------------ the dataset against its consumer
    from musicfpaugment_amd.augmentation import AugmentFP, synthetic_banks
    from musicfpaugment_amd.training.dataset import AugmentationDataset
    from musicfpaugment_amd.training.train import Trainer
    from musicfpaugment_amd.training.unet import UNet
    from musicfpaugment_amd.training.weights import formula_state_dict
    irs, noises = synthetic_banks(3)
    af = AugmentFP(ir_bank=irs, noise_bank=noises)
    B = 64
    views = [bank[i * N:(i + 1) * N] for i in range(n)]
    feeds = {}
    for where, trk in (("device", views), ("host", [v.cpu() for v in views])):
        gen_b = AugmentationDataset(None, SR, tracks=trk, augment=af, n_segments=1, model_duration_seconds=3.0).batches(B)
        for _ in range(2):
            batch = next(gen_b)
        torch.cuda.synchronize()
        per = []
        for _ in range(args.batches):
            t0 = time.perf_counter()
            batch = next(gen_b)
            torch.cuda.synchronize()
            per.append((time.perf_counter() - t0) * 1e3)
        feeds[where] = {"ms_per_batch_median": round(float(np.median(per)), 3), "ms_per_batch": [round(p, 3) for p in per],
                        "clips_per_s": round(B / (float(np.median(per)) * 1e-3), 1)}
    out["dataset"] = {"batch": B, "chunk_samples": L, "tracks_per_group": 64, "n_segments": 1, "feeds": feeds}
    net = UNet(1, 1, rate=0.0)
    net.load_state_dict(formula_state_dict(3))
    tr = Trainer(net, None, None, precision=1)
    clean, aug = batch
    for _ in range(2):
        tr.train_step(clean, aug)
    torch.cuda.synchronize()
    per = []
    for _ in range(5):
        t0 = time.perf_counter()
        tr.train_step(clean, aug)
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) * 1e3)
    out["dataset"]["train_step_bf16x3_ms"] = round(float(np.median(per)), 3)
    out["dataset"]["train_step_runs_ms"] = [round(p, 3) for p in per]
    out["gpu"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
