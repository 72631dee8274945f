"""Dejavu peak-metrics experiment on MI355X -- mirror of compute_peaks_metrics in the reference's
testing/dejavu_exps.py:82-167 (harness row SURVEY.md §8f-4), batched and sharded like testing/audfprint_exps.py.

The reference walks the augmented query files, calls Dejavu.generate_fingerprints(get_masks=True) three times per query
(clean, augmented, augmented through the denoising Dejavu instance -- afp/dejavu/dejavu.py:255-289), transposes the
(257, 249) peak masks (:118-120) and averages per-query Precision / Recall / F1 and the PSNR of the normalised
spectrograms.  `DejavuPeaks` carries the two attributes of the Dejavu class this path reads -- `denoising`,
`denoising_model` -- plus the networks, which the reference loads at import time.  Queries are tensors (or files through `compute_peaks_metrics_files`); with torch.distributed initialised
they are split over the ranks and the per-query rows gathered, so the means equal a single-GPU run's.

The reference's result dictionary is kept key for key, including its "psnr_*_wav" entries, which it fills from the
spectrogram PSNR (:139-140,158).

The identification-rate half (dejavu_exps.py:16-79) runs on the device store and matcher (afp/dejavu/database.py,
DESIGN.md §3.9): `create_fp_database` / `compute_accuracy` with the reference's signatures over files, and the tensor forms
`create_fp_database_batch` / `compute_accuracy_batch`, which shard the queries over ranks like testing/audfprint_exps.py.
"""
from __future__ import annotations

import os
from typing import Dict, Optional

import torch

from .. import ops
from ..afp.dejavu.fingerprint import fingerprint_peaks_batch
from ..constants import afp_settings
from ..pipeline import shard_range
from .audfprint_exps import _prf, _psnr


class DejavuPeaks:
    """The peak-extraction face of afp/dejavu/dejavu.py's Dejavu (constructor :121-134, generate_fingerprints :255-289)."""

    def __init__(self, settings: Optional[dict] = None, denoising: bool = False, denoising_model: Optional[str] = None,
                 unet=None, demucs=None, device="cuda") -> None:
        self.settings = dict(settings or afp_settings["dejavu"])
        self.denoising = denoising
        self.denoising_model = denoising_model
        if self.denoising is True:
            assert self.denoising_model in ["unet", "demucs"]
            if (unet if denoising_model == "unet" else demucs) is None:
                raise ValueError(f"denoising_model={denoising_model!r} needs the {denoising_model} module")
        self.unet, self.demucs = unet, demucs
        self.device = torch.device(device)

    @torch.no_grad()
    def generate_fingerprints_batch(self, wav: torch.Tensor):
        """(B, T) float32 waveforms in [-1, 1] -> (peak_mask (B, 257, nF) uint8, specgram (B, 257, nF)), the get_masks=True
        return of generate_fingerprints for every clip (read() scales by 32767, dejavu.py:106)."""
        wav = wav.to(self.device, torch.float32).contiguous()
        mask, _, spec = fingerprint_peaks_batch(wav, amp_min=self.settings["amp_min"], scale_in=32767.0,
                                                denoising=bool(self.denoising), denoising_model=self.denoising_model or "unet",
                                                unet=self.unet, demucs=self.demucs)
        return mask, spec


KEYS = ["precision_no_den", "recall_no_den", "f1_score_no_den", "psnr_no_den_spec", "psnr_no_den_wav", "prec_den", "rec_den",
        "f1_den", "psnr_den_spec", "psnr_den_wav"]


@torch.no_grad()
def compute_peaks_metrics(clean_wav: torch.Tensor, augmented_wav: torch.Tensor, djv_no_den: DejavuPeaks, djv_den: DejavuPeaks,
                          batch: int = 256) -> Dict[str, float]:
    """clean_wav, augmented_wav: (N, T) float32 (any device).  Returns the reference's result dictionary."""
    import torch.distributed as dist
    N = clean_wav.shape[0]
    ddp = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    rank, world = (dist.get_rank(), dist.get_world_size()) if ddp else (0, 1)
    lo, hi = shard_range(N, rank, world)
    dev = djv_no_den.device
    rows = []
    for s in range(lo, hi, batch):
        e = min(hi, s + batch)
        m_clean, sg_clean = djv_no_den.generate_fingerprints_batch(clean_wav[s:e])
        m_aug, sg_aug = djv_no_den.generate_fingerprints_batch(augmented_wav[s:e])
        m_den, sg_den = djv_den.generate_fingerprints_batch(augmented_wav[s:e])
        tr = lambda m: m.transpose(1, 2).contiguous()               # (B, nF, 257): dejavu_exps.py:118-120
        p, r, f1 = _prf(ops.peak_metrics_counts(tr(m_aug), tr(m_clean)))
        pd, rd, f1d = _prf(ops.peak_metrics_counts(tr(m_den), tr(m_clean)))
        ps, psd = _psnr(sg_aug, sg_clean), _psnr(sg_den, sg_clean)
        rows.append(torch.stack([p, r, f1, ps, ps, pd, rd, f1d, psd, psd], dim=1))
    local = torch.cat(rows) if rows else torch.zeros((0, len(KEYS)), dtype=torch.float64, device=dev)
    if ddp:
        sizes = [shard_range(N, r, world)[1] - shard_range(N, r, world)[0] for r in range(world)]
        pad = torch.zeros((max(sizes), len(KEYS)), dtype=torch.float64, device=dev)
        pad[: local.shape[0]] = local
        gathered = [torch.empty_like(pad) for _ in range(world)]
        dist.all_gather(gathered, pad)
        local = torch.cat([g[:n] for g, n in zip(gathered, sizes)])
    mean = (local.sum(dim=0) / max(N, 1)).cpu().tolist()             # sums in query order: identical on every rank
    return dict(zip(KEYS, mean))


def compute_peaks_metrics_files(queries_augmented, clean_dir: str, djv_no_den: DejavuPeaks, djv_den: DejavuPeaks,
                                batch: int = 256) -> Dict[str, float]:
    """The reference's signature (dejavu_exps.py:82-86): augmented query files (.pkl / .wav) whose clean counterparts carry the
    same file name under `clean_dir` (queries_paths["cleans"], :104-105).  Files are read on the host and handed to the
    batched device path; queries must share one length."""
    from ..afp.audfprint.peak_extractor import Audfprint_peaks
    sr = djv_no_den.settings["samplerate"]
    aug = [Audfprint_peaks._read_waveform(q, sr) for q in queries_augmented]
    clean = [Audfprint_peaks._read_waveform(os.path.join(clean_dir, os.path.basename(q)), sr) for q in queries_augmented]
    if len({len(a) for a in aug} | {len(c) for c in clean}) > 1:
        raise ValueError("queries of different lengths: group them by length before calling the batched harness")
    return compute_peaks_metrics(torch.stack(clean), torch.stack(aug), djv_no_den, djv_den, batch=batch)


# ----------------------------------------------------------------------------- identification rate (dejavu_exps.py:16-79)
MAX_PEAKS = 16384        # the hash kernel's peak list per clip (mfpa_dejavu_hashes)


def _hash_caps(n_samples: int, fan_value: int):
    """fingerprint()'s buffer sizes for a clip: at most one peak per ~64 cells of the (257, frames) spectrogram."""
    n_frames = (n_samples - 256) // 256
    peaks = max(16, 257 * max(n_frames, 1) // 64)
    return max(16, min(peaks, MAX_PEAKS) * max(int(fan_value) - 1, 1)), min(peaks, MAX_PEAKS)


@torch.no_grad()
def _clip_hashes(djv, wav: torch.Tensor, what: str):
    """(B, T) waveforms in [-1, 1] -> (digests, t1, counts) exactly as FileRecognizer sees them: read() runs Demucs on the
    waveform and scales by 32767 (dejavu.py:95-106), fingerprint() runs the UNet on the spectrogram (fingerprint.py:68-75)."""
    from ..afp.dejavu.fingerprint import fingerprint_batch
    settings = djv.settings if djv is not None else afp_settings["dejavu"]
    denoising = djv is not None and djv.denoising is True
    if denoising and djv.denoising_model == "demucs":
        wav = djv.demucs(wav)[:, 0]
    cap, peak_cap = _hash_caps(wav.shape[1], settings["fan_value"])
    net = djv.unet if denoising and djv.denoising_model == "unet" else None
    dig, t1, counts, _, _ = fingerprint_batch((wav * 32767).contiguous(), amp_min=settings["amp_min"],
                                              fan_value=settings["fan_value"], cap=cap, scale_in=1.0, peak_cap=peak_cap,
                                              denoising=net is not None, denoising_model="unet", unet=net)
    bad = (counts < 0).nonzero().flatten().tolist()
    if bad:
        raise ValueError(f"{what}: clip(s) {bad} have more than {peak_cap} spectral peaks or {cap} hashes, the hash kernel's "
                         f"limit for {wav.shape[1]} samples (at most {MAX_PEAKS} peaks per clip): split longer tracks")
    return dig, t1, counts


def create_fp_database(files, db=None):
    """dejavu_exps.py:16-18: a Dejavu instance in state "set" fingerprints every file (one song per file, named by its base
    name).  Returns the database."""
    from ..afp.dejavu.dejavu import Dejavu
    djv = Dejavu({"database": db} if db is not None else {}, afp_settings["dejavu"], "set")
    djv.fingerprint_directory(files)
    return djv.db


def compute_accuracy(audio_paths, djv, djv2) -> Dict[str, float]:
    """dejavu_exps.py:21-79: one query file at a time through FileRecognizer; the ground truth is the parent directory's
    name (:30), compared with the matched song's name."""
    from ..afp.dejavu.file_recognizer import FileRecognizer
    rec1, rec2 = FileRecognizer(djv), FileRecognizer(djv2)
    tp1 = tp2 = tpmix = 0
    for path in audio_paths:
        gt = path.split("/")[-2]
        r1, r2 = rec1.recognize_file(path), rec2.recognize_file(path)
        name1, n1 = (r1["results"][0]["song_name"].decode("utf-8"), r1["results"][0]["nb_matches_with_offset"]) if r1["match"] else ("", 0)
        name2, n2 = (r2["results"][0]["song_name"].decode("utf-8"), r2["results"][0]["nb_matches_with_offset"]) if r2["match"] else ("", 0)
        tp1 += bool(r1["match"] and name1 == gt)
        tp2 += bool(r2["match"] and name2 == gt)
        pred, hit = (name1, r1["match"]) if n1 >= n2 else (name2, r2["match"])
        tpmix += bool(hit and pred == gt)
    N = len(audio_paths)
    return {"No Denoising": tp1 / N, "With Denoising": tp2 / N, "Mix Pipeline": tpmix / N}


@torch.no_grad()
def create_fp_database_batch(tracks, names, db=None, batch: int = 16, device=None):
    """The database of `tracks` (a (N, T) tensor or a sequence of 1-D waveforms in [-1, 1] of any lengths) under `names`:
    tracks are fingerprinted in batches of equal length on the device, without denoising as create_fp_database does, and
    inserted with song ids in the given order.  Each song's file_sha1 is the SHA-1 of its float32 samples and its
    total_hashes the size of its set of (hash, offset) pairs.  Returns the database."""
    import hashlib

    import numpy as np

    from ..afp.dejavu.database import DeviceDatabase
    device = torch.device(device if device is not None else (db.device if db is not None else "cuda"))
    db = db if db is not None else DeviceDatabase(device=device)
    tracks = [torch.as_tensor(t, dtype=torch.float32).reshape(-1) for t in tracks]
    if len(tracks) != len(names):
        raise ValueError("one name per track")
    sids = [db.insert_song(name, hashlib.sha1(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest().upper(), 0)
            for name, t in zip(names, tracks)]
    by_len = {}
    for i, t in enumerate(tracks):
        by_len.setdefault(int(t.shape[0]), []).append(i)
    for _, idx in sorted(by_len.items()):
        for s in range(0, len(idx), batch):
            chunk = idx[s:s + batch]
            wav = torch.stack([tracks[i] for i in chunk]).to(device)
            dig, t1, counts = _clip_hashes(None, wav, "tracks " + ", ".join(str(names[i]) for i in chunk))
            db.insert_batch([sids[i] for i in chunk], dig, t1, counts)
    for sid, n in zip(sids, db.count_fingerprints(sids)):
        db.set_total_hashes(sid, n)
        db.set_song_fingerprinted(sid)
    return db


@torch.no_grad()
def compute_accuracy_batch(queries: torch.Tensor, gt_ids, db, djv_no_den, djv_den, batch: int = 256, per_query: bool = False):
    """compute_accuracy for query waveforms in memory: queries (N, T) float32 in [-1, 1], gt_ids (N,) the song id of each
    query's track.  Each query is fingerprinted by both Dejavu instances and matched on the device (match_batch, top
    row).  Returns the reference's dictionary; with per_query=True also the (N, 4) int64 tensor [sid1, count1, sid2, count2]
    behind it (sid -1 and count 0 when nb_matches_with_offset <= MIN_HASHES).  With torch.distributed initialised the
    queries are split over ranks and the rows gathered: identical to one GPU when every rank builds the same database."""
    import torch.distributed as dist

    from ..afp.dejavu.dejavu import MIN_HASHES
    from .audfprint_exps import accuracy_from_rows
    N = queries.shape[0]
    gt = torch.as_tensor(gt_ids, dtype=torch.int64).reshape(-1)
    if gt.numel() != N:
        raise ValueError("one ground-truth id per query")
    ddp = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    rank, world = (dist.get_rank(), dist.get_world_size()) if ddp else (0, 1)
    lo, hi = shard_range(N, rank, world)
    dev = db.device
    rows = []
    for s in range(lo, hi, batch):
        e = min(hi, s + batch)
        wav = queries[s:e].to(dev, torch.float32).contiguous()
        cols = []
        for djv in (djv_no_den, djv_den):
            dig, t1, n = _clip_hashes(djv, wav, f"queries {s}..{e - 1}")
            top, info = db.match_batch(dig, t1, n, k=1)
            hit = (info[:, 2] > 0) & (top[:, 0, 2] > MIN_HASHES)
            cols.append(torch.where(hit, top[:, 0, 0], -1).to(torch.int64))
            cols.append(torch.where(hit, top[:, 0, 2], 0).to(torch.int64))
        rows.append(torch.stack(cols, dim=1))
    local = torch.cat(rows) if rows else torch.zeros((0, 4), dtype=torch.int64, device=dev)
    if ddp:
        sizes = [shard_range(N, r, world)[1] - shard_range(N, r, world)[0] for r in range(world)]
        pad = torch.zeros((max(sizes), 4), dtype=torch.int64, device=dev)
        pad[: local.shape[0]] = local
        gathered = [torch.empty_like(pad) for _ in range(world)]
        dist.all_gather(gathered, pad)
        local = torch.cat([g[:n] for g, n in zip(gathered, sizes)])
    res = accuracy_from_rows(local.cpu(), gt)
    return (res, local) if per_query else res
