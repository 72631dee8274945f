"""Peak-metrics experiment on MI355X -- mirror of compute_peaks_metrics in the reference's
testing/audfprint_exps.py:86-157 (the harness row SURVEY.md §8f-4), batched and sharded.

The reference loops over 10 000 query FILES, runs find_peaks three times per query (clean, augmented,
augmented + denoiser), and averages per-query Precision / Recall / F1 (masks transposed to (1, 251, 256),
:119-121) and spectrogram PSNR.  File I/O is out of scope, so this version takes the clean and
augmented waveforms as tensors; everything else -- three peak extractions, per-query metrics, means -- runs as
batched device kernels.  With torch.distributed initialised the queries are split over ranks
(pipeline.shard_range) and the per-query results are gathered: the means are identical to a single-GPU run.
"""
from __future__ import annotations

import math
from typing import Dict

import torch

from .. import ops
from ..afp.audfprint.peak_extractor import Audfprint_peaks
from ..pipeline import shard_range


def _prf(counts: torch.Tensor):
    """(B, 4) int64 [hits_p, n_p, hits_r, n_r] -> per-query precision, recall, F1 as the reference computes them
    (testing/metrics.py: 0.0 for an empty mask; F1 = 0 when P + R is ~0)."""
    c = counts.to(torch.float64)
    p = torch.where(c[:, 1] > 0, c[:, 0] / c[:, 1].clamp_min(1), torch.zeros_like(c[:, 0]))
    r = torch.where(c[:, 3] > 0, c[:, 2] / c[:, 3].clamp_min(1), torch.zeros_like(c[:, 0]))
    s = p + r
    f1 = torch.where(s.abs() <= 1e-9, torch.zeros_like(s), 2.0 * p * r / s.clamp_min(1e-300))   # math.isclose(p + r, 0.0)
    return p, r, f1


def _psnr(pred: torch.Tensor, target64: torch.Tensor) -> torch.Tensor:
    st = ops.psnr_stats(pred, target64)
    n = pred[0].numel()
    rng = st[:, 2] - st[:, 1]
    return 10.0 * torch.log10(rng * rng / (st[:, 0] / n))


@torch.no_grad()
def compute_peaks_metrics(clean_wav: torch.Tensor, augmented_wav: torch.Tensor, analyzer_no_den: Audfprint_peaks,
                          analyzer_den: Audfprint_peaks, batch: int = 256, per_query: bool = False):
    """clean_wav, augmented_wav: (N, T) float32 (any device).  Returns the reference's result dictionary; with
    `per_query=True` also the (N, 8) float64 tensor of per-query values behind the means (columns in the dictionary's key order)."""
    import torch.distributed as dist
    N = clean_wav.shape[0]
    ddp = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    rank, world = (dist.get_rank(), dist.get_world_size()) if ddp else (0, 1)
    lo, hi = shard_range(N, rank, world)
    dev = analyzer_no_den.device
    rows = []
    for s in range(lo, hi, batch):
        e = min(hi, s + batch)
        clean = clean_wav[s:e].to(dev, torch.float32).contiguous()
        aug = augmented_wav[s:e].to(dev, torch.float32).contiguous()
        m_clean, _, sg_clean = analyzer_no_den.wav2peaks_batch(clean)
        m_aug, _, sg_aug = analyzer_no_den.wav2peaks_batch(aug)
        m_den, _, sg_den = analyzer_den.wav2peaks_batch(aug)          # UNet inside find_peaks, Demucs on the waveform
        tr = lambda m: m.transpose(1, 2).contiguous()               # (B, 251, 256): audfprint_exps.py:119-121
        c_aug = ops.peak_metrics_counts(tr(m_aug), tr(m_clean))
        c_den = ops.peak_metrics_counts(tr(m_den), tr(m_clean))
        p, r, f1 = _prf(c_aug)
        pd, rd, f1d = _prf(c_den)
        rows.append(torch.stack([p, r, f1, _psnr(sg_aug, sg_clean), pd, rd, f1d, _psnr(sg_den, sg_clean)], dim=1))
    local = torch.cat(rows) if rows else torch.zeros((0, 8), dtype=torch.float64, device=dev)
    if ddp:
        sizes = [shard_range(N, r, world)[1] - shard_range(N, r, world)[0] for r in range(world)]
        pad = torch.zeros((max(sizes), 8), dtype=torch.float64, device=dev)
        pad[: local.shape[0]] = local
        gathered = [torch.empty_like(pad) for _ in range(world)]
        dist.all_gather(gathered, pad)
        local = torch.cat([g[:n] for g, n in zip(gathered, sizes)])
    mean = (local.sum(dim=0) / max(N, 1)).cpu().tolist()             # sums in query order: identical on every rank
    keys = ["precision_no_den", "recall_no_den", "f1_score_no_den", "psnr_no_den_spec", "prec_den", "rec_den", "f1_den",
            "psnr_den_spec"]
    return (dict(zip(keys, mean)), local) if per_query else dict(zip(keys, mean))


def compute_peaks_metrics_files(queries_augmented, clean_dir: str, analyzer_no_den: Audfprint_peaks, analyzer_den: Audfprint_peaks,
                                batch: int = 256) -> Dict[str, float]:
    """The reference's signature (audfprint_exps.py:86-157): a list of augmented query files (.pkl / .wav) whose clean
    counterparts carry the same file name under `clean_dir` (queries_paths["cleans"], :106-107).  Files are read on the host
    and handed to the batched device path; queries must share one length."""
    import os
    aug = [Audfprint_peaks._read_waveform(q, analyzer_no_den.target_sr) for q in queries_augmented]
    clean = [Audfprint_peaks._read_waveform(os.path.join(clean_dir, os.path.basename(q)), analyzer_no_den.target_sr)
             for q in queries_augmented]
    if len({len(a) for a in aug} | {len(c) for c in clean}) > 1:
        raise ValueError("queries of different lengths: group them by length before calling the batched harness")
    return compute_peaks_metrics(torch.stack(clean), torch.stack(aug), analyzer_no_den, analyzer_den, batch=batch)


# ----------------------------------------------------------------------------- identification rate (audfprint_exps.py:17-84)
MAX_TRACK_FRAMES = 1500          # the pruner's frame limit (ops.audfprint_prune): 1 + n_samples // 256 <= 1500, ~48 s at 8 kHz
WHOLE_TRACK_FRAMES = ops.TRACK_MAX_FRAMES     # with whole_tracks=True: 16384 frames, ~8.7 min (the 14 time bits of the hash table)
TRACK_BATCH_FRAMES = 131072      # frames of one device batch of whole tracks: float64 spectrogram + its log copy stay near 0.5 GB


def _check_track_length(n_samples: int, what: str, whole_tracks: bool = False) -> None:
    frames = 1 + n_samples // 256
    if whole_tracks:
        if frames > WHOLE_TRACK_FRAMES:
            raise ValueError(f"{what}: {n_samples} samples = {frames} STFT frames; whole tracks take at most {WHOLE_TRACK_FRAMES} "
                             f"frames ({WHOLE_TRACK_FRAMES * 256 / 8000:.0f} s at 8 kHz): the hash table keeps 14 time bits")
        return
    if frames > MAX_TRACK_FRAMES:
        raise ValueError(f"{what}: {n_samples} samples = {frames} STFT frames; the device peak picker takes at most "
                         f"{MAX_TRACK_FRAMES} frames ({MAX_TRACK_FRAMES * 256 / 8000:.0f} s at 8 kHz) per clip, and the landmark "
                         "kernel at most 8192 landmarks: split longer tracks")


def _database_analyzer(device, whole_tracks: bool = False):
    from ..constants import afp_settings
    a = Audfprint_peaks(afp_settings["audfprint"], device=device, whole_tracks=whole_tracks)
    a.shifts = 1                                                     # audfprint_exps.py:20-21
    return a


@torch.no_grad()
def create_fp_database_batch(tracks, names, ht=None, analyzer: Audfprint_peaks = None, batch: int = 64, device=None,
                             whole_tracks: bool = False):
    """Fingerprint database of `tracks` (a (N, T) tensor or a sequence of 1-D waveforms of any lengths up to the limit
    above), stored under `names` in the given order.  Tracks are fingerprinted in batches of equal length on the device
    (hashes_batch with shifts = 1, as create_fp_database) and stored in file order with HashTable.store_batch.  Returns the
    HashTable.  `whole_tracks`: tracks of up to 16384 frames (~8.7 min) are taken whole (Audfprint_peaks(whole_tracks=True)),
    at most max(1, 131072 // frames) of them in one device batch."""
    from ..afp.audfprint.hash_table import HashTable
    device = torch.device(device if device is not None else (analyzer.device if analyzer is not None else "cuda"))
    analyzer = analyzer or _database_analyzer(device, whole_tracks)
    if whole_tracks and not analyzer.whole_tracks:
        raise ValueError("whole_tracks=True needs an analyzer built with whole_tracks=True")
    ht = ht if ht is not None else HashTable(device=device)
    tracks = list(tracks)
    if len(tracks) != len(names):
        raise ValueError("one name per track")
    for i, t in enumerate(tracks):
        _check_track_length(int(torch.as_tensor(t).shape[-1]), f"track {i} ({names[i]})", whole_tracks)
    by_len = {}
    for i, t in enumerate(tracks):
        by_len.setdefault(int(torch.as_tensor(t).shape[-1]), []).append(i)
    per_track = [None] * len(tracks)
    for n_samples, idx in sorted(by_len.items()):
        step = min(batch, max(1, TRACK_BATCH_FRAMES // (1 + n_samples // 256))) if whole_tracks else batch
        for s in range(0, len(idx), step):
            chunk = idx[s:s + step]
            wav = torch.stack([torch.as_tensor(tracks[i], dtype=torch.float32).reshape(-1) for i in chunk]).to(device)
            uq, n = analyzer.hashes_batch(wav.contiguous(), shifts=1)
            for j, i in enumerate(chunk):
                per_track[i] = (uq[j], n[j])
    cap = max([u.shape[0] for u, _ in per_track], default=1)
    for s in range(0, len(tracks), batch):                           # file order
        part = per_track[s:s + batch]
        uq = torch.zeros((len(part), cap, 2), dtype=torch.int32, device=device)
        for j, (u, _) in enumerate(part):
            uq[j, : u.shape[0]] = u
        ht.store_batch(names[s:s + batch], uq, torch.stack([n for _, n in part]))
    return ht


def _query_hashes(analyzer: Audfprint_peaks, wav: torch.Tensor):
    if analyzer.demucs is not None:                                  # wavfile2peaks: Demucs acts on the waveform (:369-376)
        wav = analyzer.demucs(wav)[:, 0].contiguous()
    return analyzer.hashes_batch(wav)


@torch.no_grad()
def compute_accuracy_batch(queries: torch.Tensor, gt_ids, ht, analyzer1: Audfprint_peaks, analyzer2: Audfprint_peaks,
                           batch: int = 256, per_query: bool = False, matcher=None):
    """compute_accuracy (audfprint_exps.py:24-84) for query waveforms already in memory: queries (N, T) float32, gt_ids (N,)
    the database id of each query's track.  Each query is fingerprinted by both analyzers (their `shifts`, 4 in the
    experiment) and matched on the device (Matcher.match_batch, top row).  Returns the reference's dictionary; with
    per_query=True also the (N, 4) int64 tensor [id1, count1, id2, count2] behind it (id -1: NOMATCH, count 0).  With
    torch.distributed initialised the queries are split over ranks and the rows gathered: identical to one GPU, because
    every rank builds the same table (the store is deterministic)."""
    import torch.distributed as dist
    from ..afp.audfprint.audfprint_match import Matcher
    matcher = matcher or Matcher()
    N = queries.shape[0]
    _check_track_length(int(queries.shape[1]), "queries")
    gt = torch.as_tensor(gt_ids, dtype=torch.int64).reshape(-1)
    if gt.numel() != N:
        raise ValueError("one ground-truth id per query")
    ddp = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    rank, world = (dist.get_rank(), dist.get_world_size()) if ddp else (0, 1)
    lo, hi = shard_range(N, rank, world)
    dev = ht.table.device
    rows = []
    for s in range(lo, hi, batch):
        e = min(hi, s + batch)
        wav = queries[s:e].to(dev, torch.float32).contiguous()
        cols = []
        for an in (analyzer1, analyzer2):
            uq, n = _query_hashes(an, wav)
            top, info = matcher.match_batch(ht, uq, n, k=1)
            hit = info[:, 1] > 0
            cols.append(torch.where(hit, top[:, 0, 0], -1).to(torch.int64))
            cols.append(torch.where(hit, top[:, 0, 1], 0).to(torch.int64))
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


def accuracy_from_rows(rows: torch.Tensor, gt: torch.Tensor):
    """[id1, count1, id2, count2] per query -> the reference's accuracies; "mix" takes analyzer 1's answer when its filtered
    count is >= analyzer 2's (audfprint_exps.py:58-73)."""
    rows = rows.to(torch.int64)
    gt = torch.as_tensor(gt, dtype=torch.int64).reshape(-1)
    N = max(rows.shape[0], 1)
    ok1 = (rows[:, 0] >= 0) & (rows[:, 0] == gt)
    ok2 = (rows[:, 2] >= 0) & (rows[:, 2] == gt)
    mix = torch.where(rows[:, 1] >= rows[:, 3], ok1, ok2)
    return {"No Denoising": int(ok1.sum()) / N, "With Denoising": int(ok2.sum()) / N, "Mix Pipeline": int(mix.sum()) / N}


def create_fp_database(files, dbpath: str, device=None, whole_tracks: bool = False) -> None:
    """audfprint_exps.py:17-27: ingest every file (unreadable ones are reported and skipped), save to dbpath.  `whole_tracks`: files of
    up to 16384 frames are fingerprinted whole, as by the reference."""
    from ..afp.audfprint.hash_table import HashTable
    hash_tab = HashTable(device=device)
    analyzer = _database_analyzer(hash_tab.device, whole_tracks)
    for filename in files:
        try:
            analyzer.ingest(hash_tab, filename)
        except Exception:
            print("error with ", filename)
    hash_tab.save(dbpath)


def compute_accuracy(files, dbpath: str, analyzer1: Audfprint_peaks, analyzer2: Audfprint_peaks) -> Dict[str, float]:
    """audfprint_exps.py:30-84, one query file at a time through Matcher.file_match_to_msgs."""
    from ..afp.audfprint.audfprint_match import Matcher
    from ..afp.audfprint.hash_table import HashTable
    hash_tab = HashTable(dbpath, device=analyzer1.device)
    matcher = Matcher()
    acc_no_den = acc_den = acc_mix = 0
    for filename in files:
        gt = filename.split("/")[-1].split(".")[0]
        msgs1 = matcher.file_match_to_msgs(analyzer1, hash_tab, filename)
        msgs2 = matcher.file_match_to_msgs(analyzer2, hash_tab, filename)
        pred1 = msgs1[1].split("/")[-1].split(".")[0]
        if msgs1[0] == "MATCH" and str(gt) == str(pred1):
            acc_no_den += 1
        pred2 = msgs2[1].split("/")[-1].split(".")[0]
        if msgs2[0] == "MATCH" and str(gt) == str(pred2):
            acc_den += 1
        if msgs1[2] >= msgs2[2]:
            pred_mix, message = pred1, msgs1[0]
        else:
            pred_mix, message = pred2, msgs2[0]
        if message == "MATCH" and str(gt) == str(pred_mix):
            acc_mix += 1
    return {"No Denoising": acc_no_den / len(files), "With Denoising": acc_den / len(files), "Mix Pipeline": acc_mix / len(files)}
