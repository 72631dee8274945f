"""Training segments: geometry, statistics, selection, gather (csrc/segments.hip)."""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np
import torch

from .._lib import check, lib, ptr, require_gpu, stream


SEGMENT_MAX_PER_TRACK = 8192           # MFPA_SEGMENT_MAX_PER_TRACK
SEGMENT_DBS_THRESHOLD = -7.5           # training/dataset.py:89


def segment_geometry(lengths, L: int, S: int) -> np.ndarray:
    """Exclusive prefix (n_tracks + 1 int32, on the HOST) of the segments per track, 1 + (N - L) // S or 0 when N < L
    (tf.signal.frame without end padding, training/dataset.py:78-82).  mfpa_segment_geometry: host integers only."""
    lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64).reshape(-1))
    seg_off = np.empty(lens.size + 1, dtype=np.int32)
    check(lib().mfpa_segment_geometry(lens.ctypes.data_as(ctypes.c_void_p), int(lens.size), int(L), int(S),
                                      seg_off.ctypes.data_as(ctypes.c_void_p)), "mfpa_segment_geometry")
    return seg_off


def segment_threshold(dbs_threshold: float = SEGMENT_DBS_THRESHOLD) -> float:
    """thr of mfpa_segment_select: 10 * ln(rms_seg / rms_ref) > dbs  <=>  meansq_seg > exp(dbs / 5) * meansq_ref."""
    return float(np.exp(np.float64(dbs_threshold) / 5.0))


def _segment_meta(off: torch.Tensor, lens: torch.Tensor, seg_off: torch.Tensor) -> int:
    for t, dt, name in ((off, torch.int64, "off"), (lens, torch.int64, "lens"), (seg_off, torch.int32, "seg_off")):
        require_gpu(t, name)
        if t.dtype != dt or t.dim() != 1:
            raise ValueError(f"{name} must be a 1-D {dt} tensor")
    if off.numel() != lens.numel() or seg_off.numel() != lens.numel() + 1:
        raise ValueError("off and lens hold one entry per track, seg_off one more")
    return int(lens.numel())


def segment_stats(bank: torch.Tensor, off: torch.Tensor, lens: torch.Tensor, seg_off: torch.Tensor, n_seg: int, L: int,
                  S: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(seg_sumsq (n_seg,) float64, trk_sumsq (n_tracks,) float64, trk_peak (n_tracks,) float32) of the tracks
    bank[off[i] : off[i] + lens[i]]; off / lens (int64) and seg_off (int32, segment_geometry's, uploaded) are device tensors and
    n_seg = seg_off[-1] is the host's copy of it.  Each value is bit for bit a function of its own samples."""
    require_gpu(bank, "bank")
    if bank.dtype != torch.float32 or bank.dim() != 1:
        raise ValueError("bank must be a 1-D float32 tensor")
    n = _segment_meta(off, lens, seg_off)
    seg_sumsq = torch.empty((int(n_seg),), dtype=torch.float64, device=bank.device)
    trk_sumsq = torch.empty((n,), dtype=torch.float64, device=bank.device)
    trk_peak = torch.empty((n,), dtype=torch.float32, device=bank.device)
    # an empty bank has no address: hand the kernel a valid one it never reads (every track is then empty)
    check(lib().mfpa_segment_stats(ptr(bank) if bank.numel() else ptr(trk_peak), ptr(off), ptr(lens), ptr(seg_off), n, int(L), int(S),
                                   ptr(seg_sumsq) if n_seg else ptr(trk_sumsq), ptr(trk_sumsq), ptr(trk_peak), stream()),
          "mfpa_segment_stats")
    return seg_sumsq, trk_sumsq, trk_peak


def segment_select(seg_sumsq: torch.Tensor, trk_sumsq: torch.Tensor, trk_peak: torch.Tensor, off: torch.Tensor, lens: torch.Tensor,
                   seg_off: torch.Tensor, L: int, S: int, keys: torch.Tensor, dbs_threshold: float = SEGMENT_DBS_THRESHOLD,
                   n_keep: int = 1, do_norm: bool = True, with_mask: bool = False):
    """The reference's select_no_silence_frames + shuffle(...)[:n_keep] per track (training/dataset.py:86-122): returns
    (sel (n_tracks * n_keep,) int32, src (...) int64, div (...) float32, kept (n_tracks,) int32[, mask (n_seg,) uint8]).
    `keys`: one uint32 per segment (an int32 tensor holding the bit patterns is taken as such), drawn before the mask is known;
    the winners of a track are its kept segments in ascending (key, index) order."""
    n = _segment_meta(off, lens, seg_off)
    require_gpu(keys, "keys")
    if keys.dim() != 1 or keys.element_size() != 4 or keys.numel() != seg_sumsq.numel():
        raise ValueError("keys must hold one 32-bit integer per segment")
    if int(n_keep) < 1:
        raise ValueError("n_keep must be at least 1")
    dev = seg_sumsq.device
    rows = n * int(n_keep)
    sel = torch.empty((rows,), dtype=torch.int32, device=dev)
    src = torch.empty((rows,), dtype=torch.int64, device=dev)
    div = torch.empty((rows,), dtype=torch.float32, device=dev)
    kept = torch.empty((n,), dtype=torch.int32, device=dev)
    mask = torch.empty((seg_sumsq.numel(),), dtype=torch.uint8, device=dev) if with_mask else None
    ns = seg_sumsq.numel()
    check(lib().mfpa_segment_select(ptr(seg_sumsq) if ns else ptr(trk_sumsq), ptr(trk_sumsq), ptr(trk_peak), ptr(off), ptr(lens),
                                    ptr(seg_off), n, int(L), int(S), ptr(keys) if ns else ptr(trk_peak),
                                    segment_threshold(dbs_threshold), int(n_keep), 1 if do_norm else 0, ptr(sel), ptr(src), ptr(div),
                                    ptr(kept), ptr(mask) if ns else 0, stream()), "mfpa_segment_select")
    return (sel, src, div, kept, mask) if with_mask else (sel, src, div, kept)


def segment_gather(bank: torch.Tensor, src: torch.Tensor, div: Optional[torch.Tensor], L: int,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[r] = bank[src[r] : src[r] + L] / div[r] (float32 division; a copy without `div`); rows with src[r] < 0 keep what `out`
    held (a fresh `out` is zero there).  The caller guarantees src[r] + L <= len(bank): nothing here reads the device to check."""
    require_gpu(bank, "bank")
    require_gpu(src, "src")
    if bank.dtype != torch.float32 or bank.dim() != 1 or src.dtype != torch.int64 or src.dim() != 1:
        raise ValueError("bank must be 1-D float32 and src 1-D int64")
    if div is not None and (div.dtype != torch.float32 or div.shape != src.shape):
        raise ValueError("div must be float32, one per row")
    rows, L = int(src.numel()), int(L)
    if out is None:
        out = torch.zeros((rows, L), dtype=torch.float32, device=bank.device)
    elif (out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != rows or out.shape[1] < L or out.stride(1) != 1
          or (rows > 1 and out.stride(0) < L)):
        raise ValueError("out must be (rows, >= L) float32 with unit stride along a row and a row pitch of at least L")
    if rows == 0 or bank.numel() == 0:
        return out
    first = out.as_strided((1,), (1,))                                   # `out` may be the first L columns of a wider buffer
    check(lib().mfpa_segment_gather(ptr(bank), ptr(src), ptr(div), rows, L, ptr(first), int(out.stride(0)) if rows > 1 else L,
                                    stream()), "mfpa_segment_gather")
    return out
