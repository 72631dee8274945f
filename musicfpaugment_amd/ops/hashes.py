"""Landmarks and hashes from peak masks (csrc/hashes.hip)."""
from __future__ import annotations

import torch

from .._lib import check, lib, ptr, require_gpu, stream
from .peaks import TRACK_MAX_FRAMES


def audfprint_landmarks(mask: torch.Tensor, cap: int = 4096, mindt: int = 2, targetdt: int = 63, targetdf: int = 31,
                        maxpairs: int = 3):
    """Peak masks (B, R, T) uint8 -> (landmarks (B,cap,4), hashes (B,cap,2), unique sorted hashes (B,cap,2),
    counts (B,2) = [n_landmarks, n_unique]); all int32 on the device.  peak_extractor.py:313-346, :40-58, :443-460."""
    require_gpu(mask, "mask")
    if mask.dim() != 3 or mask.dtype != torch.uint8:
        raise ValueError("mask must be (B, R, T) uint8")
    mask = mask.contiguous()
    B, R, T = mask.shape
    if not (1 <= cap <= 8192) or R > 256:
        raise ValueError("cap must be in [1, 8192] and R <= 256")
    dev = mask.device
    lm = torch.zeros((B, cap, 4), dtype=torch.int32, device=dev)
    hs = torch.zeros((B, cap, 2), dtype=torch.int32, device=dev)
    uq = torch.zeros((B, cap, 2), dtype=torch.int32, device=dev)
    counts = torch.zeros((B, 2), dtype=torch.int32, device=dev)
    check(lib().mfpa_audfprint_landmarks(ptr(mask), B, R, T, cap, mindt, targetdt, targetdf, maxpairs, ptr(lm), ptr(hs),
                                         ptr(uq), ptr(counts), stream()), "mfpa_audfprint_landmarks")
    return lm, hs, uq, counts


def audfprint_landmarks_track(mask: torch.Tensor, cap: int, mindt: int = 2, targetdt: int = 63, targetdf: int = 31, maxpairs: int = 3,
                              want_lists: bool = False):
    """audfprint_landmarks for whole tracks (mfpa_audfprint_landmarks_track): peak masks (B, R, T) uint8 with T <= 16384 and any
    capacity `cap` -> (landmarks (B,cap,4) | None, hashes (B,cap,2) | None, unique sorted hashes (B,cap,2), counts (B,2)); the two
    list-order outputs only with `want_lists`.  counts is [-1, -1] for a clip with more than 8 peaks in a frame or more than `cap`
    landmarks."""
    require_gpu(mask, "mask")
    if mask.dim() != 3 or mask.dtype != torch.uint8:
        raise ValueError("mask must be (B, R, T) uint8")
    mask = mask.contiguous()
    B, R, T = mask.shape
    if cap < 1 or R > 256 or R % 4 or T < 1 or T > TRACK_MAX_FRAMES:
        raise ValueError(f"cap must be >= 1, R <= 256 with R % 4 == 0 and 1 <= T <= {TRACK_MAX_FRAMES}")
    dev = mask.device
    lm = torch.zeros((B, cap, 4), dtype=torch.int32, device=dev) if want_lists else None
    hs = torch.zeros((B, cap, 2), dtype=torch.int32, device=dev) if want_lists else None
    uq = torch.zeros((B, cap, 2), dtype=torch.int32, device=dev)
    counts = torch.zeros((B, 2), dtype=torch.int32, device=dev)
    tiles = torch.empty((B, (T + 255) // 256, 2), dtype=torch.int32, device=dev)
    check(lib().mfpa_audfprint_landmarks_track(ptr(mask), B, R, T, int(cap), mindt, targetdt, targetdf, maxpairs, ptr(tiles), ptr(lm),
                                               ptr(hs), ptr(uq), ptr(counts), stream()), "mfpa_audfprint_landmarks_track")
    return lm, hs, uq, counts


def dejavu_hashes(mask: torch.Tensor, cap: int = 4096, peak_cap: int = 4096, fan_value: int = 3, min_dt: int = 0,
                  max_dt: int = 200):
    """Peak masks (B, F, T) uint8 -> (digests (B,cap,10) uint8 = sha1("f1|f2|dt")[:20 hex], t1 (B,cap) int32,
    counts (B,) int32).  afp/dejavu/fingerprint.py:174-213."""
    require_gpu(mask, "mask")
    if mask.dim() != 3 or mask.dtype != torch.uint8:
        raise ValueError("mask must be (B, F, T) uint8")
    mask = mask.contiguous()
    B, F, T = mask.shape
    dev = mask.device
    dig = torch.zeros((B, cap, 10), dtype=torch.uint8, device=dev)
    t1 = torch.zeros((B, cap), dtype=torch.int32, device=dev)
    counts = torch.zeros((B,), dtype=torch.int32, device=dev)
    check(lib().mfpa_dejavu_hashes(ptr(mask), B, F, T, cap, peak_cap, fan_value, min_dt, max_dt, ptr(dig), ptr(t1),
                                   ptr(counts), stream()), "mfpa_dejavu_hashes")
    return dig, t1, counts
