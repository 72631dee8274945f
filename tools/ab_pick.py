#!/usr/bin/env python3
"""Audfprint picker and landmark timing of one library in one process.  usage: ab_pick.py [--lib PATH] [--clips 256] [--reps 30]

Clips (the shape of benchmark config 2: --clips x 64000 samples): stft_mag, audfprint_prune, audfprint_pick, audfprint_landmarks, and
the hashes_batch chain (STFT -> pick -> landmarks -> unique rows).  Tracks (16 x 8000 frames, about four minutes each):
audfprint_pick_track, audfprint_landmarks_track.  Every figure is the MEDIAN of --reps single calls, each between two HIP events.
To compare two builds, run this once per library in alternation (A B A B A B), a fresh process each."""
import argparse, os, statistics, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser(); ap.add_argument("--lib", default=None); ap.add_argument("--clips", type=int, default=256)
ap.add_argument("--reps", type=int, default=30)
args = ap.parse_args()
if args.lib:
    from musicfpaugment_amd import _lib
    _lib.set_library_path(args.lib)
from musicfpaugment_amd import ops, synth
from musicfpaugment_amd.afp.audfprint.peak_extractor import Audfprint_peaks
B = args.clips
base = synth.batch(32, seed=59)
wav = torch.from_numpy(np.concatenate([base] * (B // 32)).copy()).cuda()
mag, cmax = ops.stft_mag(wav, torch.float64)
def t(fn, reps=args.reps):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(us)
tag = args.lib or "product"
def line(name, us, note=""):
    print(f"{tag:40s} {name:26s} {us:9.1f} us  {note}", flush=True)
line("stft_mag", t(lambda: ops.stft_mag(wav, torch.float64)), f"B={B}")
filtered = ops.audfprint_prepare(mag, cmax, mean_order=1, denom_is_clip_max=True)
line("audfprint_prune", t(lambda: ops.audfprint_prune(filtered)))
del filtered
line("audfprint_pick", t(lambda: ops.audfprint_pick(mag, cmax)))
mask, npeaks = ops.audfprint_pick(mag, cmax)
line("audfprint_landmarks", t(lambda: ops.audfprint_landmarks(mask, 4096)),
     f"npeaks per clip {float(npeaks.float().mean()):.1f}, landmarks {float(ops.audfprint_landmarks(mask, 4096)[3][:, 0].float().mean()):.1f}")
an = Audfprint_peaks(None, device="cuda")
line("hashes_batch chain", t(lambda: an.hashes_batch(wav)), f"rows per clip {float(an.hashes_batch(wav)[1].float().mean()):.1f}")
# floor of the scan: a constant spectrogram has (almost) no candidate frames -- what the frame loops cost with every frame quiet
flat = torch.ones_like(mag); fmax = torch.ones_like(cmax)
line("audfprint_pick, constant", t(lambda: ops.audfprint_pick(flat, fmax)), f"npeaks {int(ops.audfprint_pick(flat, fmax)[1].sum())}")
del flat, mag, mask
# whole tracks: 16 tracks of 8000 frames, each the 32 clips strung together from another starting clip
FR, NT = 8000, 16
tracks = np.stack([np.roll(base, -2 * k, axis=0).reshape(-1)[:(FR - 1) * 256] for k in range(NT)])
tmag, tmax = ops.stft_mag(torch.from_numpy(tracks).cuda(), torch.float64)
assert tmag.shape[2] == FR
line("audfprint_pick_track", t(lambda: ops.audfprint_pick_track(tmag, tmax), max(5, args.reps // 3)), f"{NT} x {FR} frames")
tmask, tn = ops.audfprint_pick_track(tmag, tmax)
cap = 3 * int(tn.max())
line("audfprint_landmarks_track", t(lambda: ops.audfprint_landmarks_track(tmask, cap), max(5, args.reps // 3)),
     f"npeaks per track {float(tn.float().mean()):.0f}, rows {float(ops.audfprint_landmarks_track(tmask, cap)[3][:, 1].float().mean()):.0f}")
