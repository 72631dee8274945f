#!/usr/bin/env python3
"""Timing of the room simulator (ops.simulate_rir; csrc/rir.hip) and of the RoomReverb transform on one MI355X.

Rooms: --rooms (1 and 64) rooms of 3.0 x 2.5 x 2.2 m, the sources and microphones varying with the row, at 8 kHz, for the orders and
lengths a decay target of 0.1 s (order 16, 800 samples) and of 0.3 s (order 47, 2400 samples) ask for, each order with each length.
Every case is warmed up and then timed --reps times with device events around --inner back-to-back calls; the median per call is
reported with every run beside it (the method of tools/time_iir.py).
  ms              device time of one call
  images          rooms x mfpa_rir_image_count(order): every image is visited, whether or not its window meets the response
  images_per_s    images / ms
Cases per batch:
  launch            mfpa_rir_shoebox alone, the geometry already on the device
  ops.simulate_rir  the whole op: the geometry checked on the host and uploaded, the output allocated, then the launch
Then RoomReverb (p = 1, defaults: host draws, one simulator launch, mfpa_fir and the peak division) on 64 x --samples (64000)
samples beside ApplyImpulseResponse with a bank of responses of the same length.  Prints one JSON line.

Usage:  python tools/time_rir.py [--rooms 1 64] [--samples 64000] [--reps 7] [--inner 5]
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
from musicfpaugment_amd.functional import eyring_absorption  # noqa: E402

ROOM, FS = (3.0, 2.5, 2.2), 8000


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


def rooms(B: int, rt60: float):
    """B rooms of ROOM with the source and the microphone moving with the row, the walls at Eyring's coefficient for rt60."""
    b = np.arange(B)[:, None]
    source = 0.5 + np.array(ROOM) * 0.3 * (0.5 + 0.5 * np.cos(b + np.arange(3)[None]))
    mic = np.array(ROOM) - 0.5 - np.array(ROOM) * 0.3 * (0.5 + 0.5 * np.sin(2.0 * b + np.arange(3)[None]))
    return np.tile(ROOM, (B, 1)), source, mic, eyring_absorption(ROOM, rt60)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rooms", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--samples", type=int, default=64000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_rir.py measures on the MI355X: no GPU, no number")
    dev = torch.device("cuda:0")
    out = {"sample_rate": FS, "room": ROOM, "reps": args.reps, "inner": args.inner, "cases": []}

    def add(B, name, fn, images=None):
        ms, runs, y = timed(fn, args.reps, args.inner)
        case = {"rooms": B, "case": name, "ms": round(ms, 4), "runs_ms": runs, "checksum": float(y.double().abs().mean())}
        if images:
            case.update(images=images, images_per_s=round(images / (ms * 1e-3), 1))
        out["cases"].append(case)

    for B in args.rooms:
        for order, rt60 in ((16, 0.1), (47, 0.3)):
            room, source, mic, alpha = rooms(B, rt60)
            geom_d = torch.from_numpy(ops.rir_geometry(room, source, mic, alpha)).to(dev)
            for length in (800, 2400):
                h = torch.empty((B, length), dtype=torch.float32, device=dev)

                def launch(geom_d=geom_d, h=h, order=order, length=length):
                    check(lib().mfpa_rir_shoebox(ptr(geom_d), B, order, length, float(FS), 343.0, 81, 0, 0, ptr(h), length, stream()),
                          "mfpa_rir_shoebox")
                    return h

                images = B * ops.rir_image_count(order)
                add(B, f"launch order={order} length={length}", launch, images)
                add(B, f"ops.simulate_rir order={order} length={length}",
                    lambda a=(room, source, mic, alpha, order, length): ops.simulate_rir(*a, FS), images)

    from musicfpaugment_amd.augmentation.transformations.impulse_response import ApplyImpulseResponse
    from musicfpaugment_amd.augmentation.transformations.room_reverb import RoomReverb
    B, T = 64, args.samples
    gen = torch.Generator(device=dev)
    gen.manual_seed(T)
    wav = (torch.rand((B, T), generator=gen, device=dev) * 2 - 1)[:, None, :]
    reverb = RoomReverb(p=1.0, sample_rate=FS)

    def seeded(fn):
        def run():
            random.seed(0)
            torch.manual_seed(0)
            return fn()
        return run

    add(B, "RoomReverb p=1, defaults", seeded(lambda: reverb(wav).samples))
    ir = reverb.transform_parameters["ir"]
    out["room_reverb"] = {"order": reverb.transform_parameters["max_order"], "ir_length": int(ir.shape[1]),
                          "images": B * ops.rir_image_count(reverb.transform_parameters["max_order"])}
    air = ApplyImpulseResponse(None, FS, p=1.0, ir_bank=[row.cpu() for row in ir], device=dev)
    add(B, f"ApplyImpulseResponse p=1, bank of {ir.shape[0]} x {ir.shape[1]} taps", seeded(lambda: air(wav).samples))
    out["gpu"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
