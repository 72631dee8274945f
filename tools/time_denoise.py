#!/usr/bin/env python3
"""Timing of the spectral noise suppressor (ops.spectral_suppress; csrc/denoise.hip) on one MI355X, and the table for the question it
exists to make answerable: what does a classical suppressor do to the waveform SNR and to Audfprint's peaks?

Timing.  Batches of float64 magnitudes (B, 257, nF) already on the device, |N(0,1)|: 64 and 256 clips of 251 frames, 1 and 64
clips of 1500 frames, each at the default window (48, 48) and at the largest (63, 64).  Every case is warmed up and then timed in
--reps (7) windows of --inner (5) back-to-back calls between device events; the median per call is reported with every window
beside it (the method of tools/time_codec.py).
  ms              device time of one call
  one_pass_bytes  every magnitude read once and written once (8 bytes each way)
  gbs             one_pass_bytes / ms: ACHIEVED rate against that byte count, not a traffic measurement
Beside each batch: ops.stft_mag on waveforms of the same frame count; the suppressor with a noise PSD given (no tracker) and with
g and n returned.  For 32 clips of 64000 samples: SpectralDenoiser.denoise_waveform (STFT, suppressor, inverse STFT).

Table.  Noise-free tonal clips (decaying harmonic notes, tests/_denoise_oracle.tonal) plus white and pink noise at 0, 10 and 20 dB:
waveform SNR in and out of denoise_waveform, and the F1 of Audfprint's peak mask against the clean clip's mask without and with
the suppressor in the UNet's slot (ops.peak_metrics_counts: precision and recall with the experiment's tolerance).  Prints one JSON
line.

Usage:  python tools/time_denoise.py [--reps 7] [--inner 5] [--seeds 4]
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
from musicfpaugment_amd.afp.audfprint.peak_extractor import Audfprint_peaks  # noqa: E402
from musicfpaugment_amd.denoisers import SpectralDenoiser  # noqa: E402
from tests import _denoise_oracle as o  # noqa: E402


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


def f1(counts: np.ndarray) -> float:
    hp, n_pred, hr, n_gt = (float(v) for v in counts)
    p, r = hp / max(n_pred, 1.0), hr / max(n_gt, 1.0)
    return 2.0 * p * r / (p + r) if p + r > 0.0 else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--seeds", type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_denoise.py measures on the MI355X: no GPU, no number")
    dev = torch.device("cuda:0")
    out = {"reps": args.reps, "inner": args.inner, "cases": [], "table": []}

    def add(B, nF, name, fn, nbytes):
        ms, runs, y = timed(fn, args.reps, args.inner)
        out["cases"].append({"clips": B, "frames": nF, "case": name, "ms": round(ms, 4), "runs_ms": runs, "one_pass_bytes": nbytes,
                             "gbs": round(nbytes / (ms * 1e-3) / 1e9, 1), "checksum": float(y.double().abs().mean())})

    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    for B, nF in ((64, 251), (256, 251), (1, 1500), (64, 1500)):
        mag = torch.randn((B, 257, nF), generator=gen, device=dev, dtype=torch.float64).abs()
        wav = torch.rand((B, 256 * (nF - 1)), generator=gen, device=dev) * 2 - 1
        noise = torch.full((B, 257), 0.5, device=dev, dtype=torch.float64)
        nbytes = 2 * mag.numel() * 8
        for back, ahead in ((48, 48), (63, 64)):
            add(B, nF, f"ops.spectral_suppress window ({back}, {ahead})", lambda b=back, a=ahead: ops.spectral_suppress(mag, back=b, ahead=a), nbytes)
        add(B, nF, "ops.spectral_suppress window (0, 0)", lambda: ops.spectral_suppress(mag, back=0, ahead=0), nbytes)
        add(B, nF, "ops.spectral_suppress noise_psd given", lambda: ops.spectral_suppress(mag, noise_psd=noise), nbytes)
        add(B, nF, "ops.spectral_suppress return_gain, return_noise", lambda: ops.spectral_suppress(mag, return_gain=True, return_noise=True)[0],
            2 * nbytes)
        add(B, nF, "ops.spectral_suppress float32 in and out", lambda m32=mag.float(): ops.spectral_suppress(m32), nbytes // 2)
        add(B, nF, "ops.stft_mag", lambda: ops.stft_mag(wav, torch.float64)[0], wav.numel() * 4 + mag.numel() * 8)
        del mag, wav

    net = SpectralDenoiser().to(dev).eval()
    wav = torch.rand((32, 64000), generator=gen, device=dev) * 2 - 1
    add(32, 251, "SpectralDenoiser.denoise_waveform", lambda: net.denoise_waveform(wav), 2 * wav.numel() * 4)
    add(32, 251, "ops.stft_complex + ops.istft", lambda: ops.istft(ops.stft_complex(wav), 64000), 2 * wav.numel() * 4)

    plain = Audfprint_peaks(None, device=dev)
    denoised = Audfprint_peaks(None, denoising=True, denoising_model="unet", unet=SpectralDenoiser(), device=dev)
    cleans = [o.tonal(seed=s) for s in range(args.seeds)]
    clean_d = torch.from_numpy(np.stack(cleans)).float().to(dev)
    clean_mask = plain.find_peaks_batch(clean_d)[0].transpose(1, 2).contiguous()
    for kind in ("white", "pink"):
        for snr_in in (0.0, 10.0, 20.0):
            noisy = np.stack([o.noisy(c, kind, snr_in, seed=100 + s) for s, c in enumerate(cleans)])
            x = torch.from_numpy(noisy).float().to(dev)
            y = net.denoise_waveform(x).double().cpu().numpy()
            row = {"noise": kind, "snr_in_db": snr_in,
                   "snr_out_db": round(float(np.mean([o.snr_db(c, y[s]) for s, c in enumerate(cleans)])), 2)}
            for name, ext in (("f1_plain", plain), ("f1_suppressed", denoised)):
                mask = ext.find_peaks_batch(x)[0].transpose(1, 2).contiguous()
                counts = ops.peak_metrics_counts(mask, clean_mask).cpu().numpy()
                row[name] = round(float(np.mean([f1(c) for c in counts])), 4)
            out["table"].append(row)
    out["gpu"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
