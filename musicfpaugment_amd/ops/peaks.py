"""The Audfprint and Dejavu peak pickers and the metrics on their masks (csrc/audfprint.hip, dejavu.hip, metrics.hip)."""
from __future__ import annotations

import ctypes
from functools import lru_cache
from typing import Optional

import numpy as np
import torch

from .._lib import check, lib, ptr, require_gpu, stream
from ._args import _dtype_code
from .stft import N_HOP


FLOAT32_LOGS = ("rounded", "numpy")


def _float32_log_code(float32_log: str) -> int:
    """The logarithm of the pickers' FLOAT32 (denoised) branch: "rounded" = the float64 log rounded once to float32 (the default),
    "numpy" = numpy's own float32 log bit for bit (csrc/mfpa_nplog.h), what the reference computes at
    afp/audfprint/peak_extractor.py:265-276 and afp/dejavu/fingerprint.py:70-79."""
    if float32_log not in FLOAT32_LOGS:
        raise ValueError(f"float32_log must be 'rounded' or 'numpy', got {float32_log!r}")
    return FLOAT32_LOGS.index(float32_log)


# testing/parameters.py:17-26 (afp_settings["audfprint"])
AUDFPRINT_DENSITY = 20
AUDFPRINT_MAX_PKS = 5
AUDFPRINT_F_SD = 30.0
AUDFPRINT_POLE = 0.98


def audfprint_a_dec(density: float = AUDFPRINT_DENSITY, n_hop: int = N_HOP) -> float:
    """peak_extractor.py:295."""
    return float(1 - 0.01 * (density * np.sqrt(n_hop / 352.8) / 35))


@lru_cache(maxsize=16)
def _gauss_cached(npoints: int, width: float, device_index: int) -> torch.Tensor:
    # peak_extractor.py:163-165 -- computed with numpy on the host so the table is numpy's, bit for bit
    tab = np.exp(-0.5 * ((np.arange(-npoints, npoints + 1) / width) ** 2))
    return torch.from_numpy(tab).to(torch.device("cuda", device_index))


def gauss_table(npoints: int, width: float, device) -> torch.Tensor:
    device = torch.device(device)
    return _gauss_cached(int(npoints), float(width),
                         device.index if device.index is not None else torch.cuda.current_device())


def audfprint_prepare(spec: torch.Tensor, denom: Optional[torch.Tensor] = None, mean_order: int = 0,
                      log_input: bool = False, pole: float = AUDFPRINT_POLE, denom_is_clip_max: bool = False,
                      float32_log: str = "rounded") -> torch.Tensor:
    """(B, F, T) spectrogram -> frame-major filtered log-spectrogram (B, T, F-1) float64.  `denom_is_clip_max`: denom[b] is the
    maximum of the float64 spec[b] itself (what stft_mag returned with it), so the kernel skips its max pass.  `float32_log`
    ("rounded" | "numpy", float32 spectrograms without `log_input` only): which float32 logarithm, see _float32_log_code."""
    nplog = 4 * _float32_log_code(float32_log)
    require_gpu(spec, "spectrogram")
    if spec.dim() != 3:
        raise ValueError("spectrogram must be (B, F, T)")
    spec = spec.contiguous()
    B, F, T = spec.shape
    if F < 2 or F - 1 > 256 or T < 1:
        raise ValueError("need 2 <= F <= 257 bins and T >= 1 frames")
    if denom is not None and (denom.shape != (B,) or denom.dtype != torch.float64):
        raise ValueError("denom must be (B,) float64")
    filtered = torch.empty((B, T, F - 1), dtype=torch.float64, device=spec.device)
    scratch = torch.empty((B, F * T), dtype=torch.float64, device=spec.device)
    check(lib().mfpa_audfprint_prepare(ptr(spec), _dtype_code(spec), B, F, T, ptr(denom), int(mean_order),
                                       int(bool(log_input)) | (2 if (denom_is_clip_max and denom is not None and spec.dtype == torch.float64) else 0) | nplog,
                                       float(pole), ptr(filtered), ptr(scratch), stream()),
          "mfpa_audfprint_prepare")
    return filtered


def audfprint_prune(filtered: torch.Tensor, a_dec: Optional[float] = None, maxpks: int = AUDFPRINT_MAX_PKS,
                    f_sd: float = AUDFPRINT_F_SD):
    """Frame-major filtered (B, T, R) float64 -> (mask (B, R, T) uint8, npeaks (B,) int32)."""
    require_gpu(filtered, "filtered spectrogram")
    if filtered.dim() != 3 or filtered.dtype != torch.float64:
        raise ValueError("filtered must be (B, T, R) float64")
    filtered = filtered.contiguous()
    B, T, R = filtered.shape
    if R % 4 or R < 4 or R > 256 or T < 1 or T > 1500 or not (1 <= maxpks <= 8):
        raise ValueError("unsupported pruner shape (R % 4 == 0, R <= 256, T <= 1500, maxpks <= 8)")
    if a_dec is None:
        a_dec = audfprint_a_dec()
    gauss = gauss_table(R, f_sd, filtered.device)
    mask = torch.empty((B, R, T), dtype=torch.uint8, device=filtered.device)
    npeaks = torch.empty((B,), dtype=torch.int32, device=filtered.device)
    check(lib().mfpa_audfprint_prune(ptr(filtered), B, R, T, ptr(gauss), float(a_dec), int(maxpks), ptr(mask),
                                     ptr(npeaks), stream()), "mfpa_audfprint_prune")
    return mask, npeaks


def audfprint_pick(mag: torch.Tensor, clip_max: torch.Tensor, a_dec: Optional[float] = None, maxpks: int = AUDFPRINT_MAX_PKS,
                   f_sd: float = AUDFPRINT_F_SD, pole: float = AUDFPRINT_POLE):
    """find_peaks without a denoiser, stages 1 + 2 in one call (mfpa_audfprint_pick): raw float64 |STFT| (B, F, T) and its per-clip
    maxima (what stft_mag returned) -> (mask (B, F-1, T) uint8, npeaks (B,) int32).  Same arithmetic as
    audfprint_prepare(mag, clip_max, mean_order=1, denom_is_clip_max=True) + audfprint_prune; the filtered spectrogram is never
    written (the pruner filters the frames as it walks them)."""
    require_gpu(mag, "spectrogram")
    if mag.dim() != 3 or mag.dtype != torch.float64:
        raise ValueError("spectrogram must be (B, F, T) float64")
    mag = mag.contiguous()
    B, F, T = mag.shape
    if clip_max.shape != (B,) or clip_max.dtype != torch.float64:
        raise ValueError("clip_max must be (B,) float64")
    if F < 141 or F > 257 or (F - 1) % 4 or T < 1 or T > 512 or ((F - 1) * T) % 16 or not (1 <= maxpks <= 8):
        raise ValueError("unsupported shape for the fused picker (141 <= F <= 257, (F - 1) % 4 == 0, T <= 512, maxpks <= 8)")
    if a_dec is None:
        a_dec = audfprint_a_dec()
    gauss = gauss_table(F - 1, f_sd, mag.device)
    work = torch.empty(B * F * T + B * 128, dtype=torch.float64, device=mag.device)
    mask = torch.empty((B, F - 1, T), dtype=torch.uint8, device=mag.device)
    npeaks = torch.empty((B,), dtype=torch.int32, device=mag.device)
    check(lib().mfpa_audfprint_pick(ptr(mag), ptr(clip_max), B, F, T, float(pole), ptr(gauss), float(a_dec), int(maxpks), ptr(work),
                                    ptr(mask), ptr(npeaks), stream()), "mfpa_audfprint_pick")
    return mask, npeaks


TRACK_MAX_FRAMES = 16384          # HashTable keeps 14 time bits (hash_table.py:55 of the reference): frame times below 2^14 do not wrap


def audfprint_pick_track(mag: torch.Tensor, clip_max: torch.Tensor, a_dec: Optional[float] = None, maxpks: int = AUDFPRINT_MAX_PKS,
                         f_sd: float = AUDFPRINT_F_SD, pole: float = AUDFPRINT_POLE):
    """audfprint_pick for whole tracks (mfpa_audfprint_pick_track): raw float64 |STFT| (B, F, T) with 1 <= T <= 16384 frames and its
    per-clip maxima -> (mask (B, F-1, T) uint8, npeaks (B,) int32).  The same arithmetic, value for value; the pruner's event list
    lives in a workspace allocated here (T * maxpks * 12 + 4 * (T + 2) bytes per clip) instead of LDS."""
    require_gpu(mag, "spectrogram")
    if mag.dim() != 3 or mag.dtype != torch.float64:
        raise ValueError("spectrogram must be (B, F, T) float64")
    mag = mag.contiguous()
    B, F, T = mag.shape
    if clip_max.shape != (B,) or clip_max.dtype != torch.float64:
        raise ValueError("clip_max must be (B,) float64")
    if F < 141 or F > 257 or (F - 1) % 4 or T < 1 or T > TRACK_MAX_FRAMES or not (1 <= maxpks <= 8):
        raise ValueError(f"unsupported shape for the track picker (141 <= F <= 257, (F - 1) % 4 == 0, 1 <= T <= {TRACK_MAX_FRAMES}, "
                         "maxpks <= 8)")
    if a_dec is None:
        a_dec = audfprint_a_dec()
    dev = mag.device
    gauss = gauss_table(F - 1, f_sd, dev)
    nchunks = (F * T + 8191) // 8192
    logs = torch.empty((B, T, F), dtype=torch.float64, device=dev)
    sums = torch.empty((B, 2 * nchunks), dtype=torch.float64, device=dev)
    events = torch.empty(max(1, (B * (T * maxpks * 12 + 4 * (T + 2)) + 7) // 8), dtype=torch.float64, device=dev)
    mask = torch.empty((B, F - 1, T), dtype=torch.uint8, device=dev)
    npeaks = torch.empty((B,), dtype=torch.int32, device=dev)
    check(lib().mfpa_audfprint_pick_track(ptr(mag), ptr(clip_max), B, F, T, float(pole), ptr(gauss), float(a_dec), int(maxpks),
                                          ptr(logs), ptr(sums), ptr(events), ptr(mask), ptr(npeaks), stream()),
          "mfpa_audfprint_pick_track")
    return mask, npeaks


# ----------------------------------------------------------------------------- Dejavu picker
DEJAVU_RADIUS = 10   # afp/dejavu/variables.py:19 PEAK_NEIGHBORHOOD_SIZE
DEJAVU_AMP_MIN = 50  # testing/parameters.py:32


def dejavu_prepare(psd: torch.Tensor, denom: Optional[torch.Tensor], scale: float = 10.0,
                   mean_order: int = 1) -> torch.Tensor:
    require_gpu(psd, "psd")
    if psd.dim() != 3 or psd.dtype != torch.float64:
        raise ValueError("psd must be (B, F, T) float64")
    psd = psd.contiguous()
    B, F, T = psd.shape
    arr = torch.empty_like(psd)
    check(lib().mfpa_dejavu_prepare(ptr(psd), B, F, T, ptr(denom), float(scale), int(mean_order), ptr(arr), stream()),
          "mfpa_dejavu_prepare")
    return arr


def dejavu_pick(psd: torch.Tensor, clip_max: torch.Tensor, scale: float = 10.0, mean_order: int = 1, radius: int = DEJAVU_RADIUS,
                amp_min: float = DEJAVU_AMP_MIN):
    """The un-denoised Dejavu chain after the spectrogram in one call (mfpa_dejavu_pick): PSD (B, F, T) float64 and its per-clip
    maxima (what specgram_psd returned) -> (mask (B, F, T) uint8, npeaks (B,) int32).  Same arithmetic as
    dejavu_prepare(psd, clip_max, scale, mean_order) + localmax2d; the mean-subtracted array is never written."""
    require_gpu(psd, "psd")
    if psd.dim() != 3 or psd.dtype != torch.float64:
        raise ValueError("psd must be (B, F, T) float64")
    psd = psd.contiguous()
    B, F, T = psd.shape
    if clip_max.shape != (B,) or clip_max.dtype != torch.float64:
        raise ValueError("clip_max must be (B,) float64")
    per = ctypes.c_longlong(0)
    check(lib().mfpa_dejavu_pick_work_doubles(F, T, ctypes.byref(per)), "mfpa_dejavu_pick_work_doubles")
    work = torch.empty(max(B, 1) * per.value, dtype=torch.float64, device=psd.device)
    mask = torch.empty((B, F, T), dtype=torch.uint8, device=psd.device)
    npeaks = torch.empty(B, dtype=torch.int32, device=psd.device)
    check(lib().mfpa_dejavu_pick(ptr(psd), ptr(clip_max), B, F, T, float(scale), int(mean_order), int(radius), float(amp_min),
                                 ptr(work), ptr(mask), ptr(npeaks), stream()), "mfpa_dejavu_pick")
    return mask, npeaks


def dejavu_prepare_f32(x: torch.Tensor, square: bool = True, scale: float = 10.0, mean_order: int = 0,
                       float32_log: str = "rounded") -> torch.Tensor:
    """The denoised branch of Dejavu's pre-processing (fingerprint.py:70-79): float32 (B, F, T) network output -> x**2 ->
    10*log(max(., max/1e6)) - mean in float32, widened to float64 for the picker.  `float32_log` ("rounded" | "numpy"): which
    float32 logarithm, see _float32_log_code."""
    log_mode = _float32_log_code(float32_log)
    require_gpu(x, "x")
    if x.dim() != 3 or x.dtype != torch.float32:
        raise ValueError("x must be (B, F, T) float32")
    x = x.contiguous()
    B, F, T = x.shape
    arr = torch.empty((B, F, T), dtype=torch.float64, device=x.device)
    check(lib().mfpa_dejavu_prepare_f32_ex(ptr(x), B, F, T, int(bool(square)), float(scale), int(mean_order), log_mode, ptr(arr),
                                           stream()), "mfpa_dejavu_prepare_f32_ex")
    return arr


def localmax2d(arr: torch.Tensor, radius: int = DEJAVU_RADIUS, amp_min: float = DEJAVU_AMP_MIN):
    require_gpu(arr, "arr2D")
    if arr.dim() != 3 or arr.dtype != torch.float64:
        raise ValueError("arr must be (B, F, T) float64")
    arr = arr.contiguous()
    B, F, T = arr.shape
    if not (0 <= radius <= 16) or F < 1 or T < 1:
        raise ValueError("radius must be in [0, 16]")
    mask = torch.empty((B, F, T), dtype=torch.uint8, device=arr.device)
    npeaks = torch.empty((B,), dtype=torch.int32, device=arr.device)
    check(lib().mfpa_localmax2d(ptr(arr), B, F, T, int(radius), float(amp_min), ptr(mask), ptr(npeaks), stream()),
          "mfpa_localmax2d")
    return mask, npeaks


def peak_metrics_counts(predicted: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """0/1 uint8 masks (B, N1, N2) -> (B, 4) int64 [hits_p, n_pred, hits_r, n_gt]."""
    require_gpu(predicted, "predicted")
    require_gpu(gt, "gt")
    if predicted.shape != gt.shape or predicted.dim() != 3:
        raise ValueError("masks must both be (B, N1, N2)")
    if predicted.dtype != torch.uint8 or gt.dtype != torch.uint8:
        raise TypeError("masks must be uint8")
    predicted, gt = predicted.contiguous(), gt.contiguous()
    B, N1, N2 = predicted.shape
    if N1 < 2 or N2 < 2:
        raise ValueError("mask axes must have length >= 2")
    counts = torch.empty((B, 4), dtype=torch.int64, device=predicted.device)
    check(lib().mfpa_peak_metrics(ptr(predicted), ptr(gt), B, N1, N2, ptr(counts), stream()), "mfpa_peak_metrics")
    return counts


def psnr_stats(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """(B, ...) pred (float32|float64) vs float64 target -> (B, 3) float64 [sse, min(target), max(target)]."""
    require_gpu(pred, "pred")
    require_gpu(target, "target")
    if pred.shape != target.shape or target.dtype != torch.float64:
        raise ValueError("pred/target must have the same shape, target float64")
    pred, target = pred.contiguous(), target.contiguous()
    B = pred.shape[0]
    n = pred[0].numel() if B else 0
    out = torch.empty((B, 3), dtype=torch.float64, device=pred.device)
    check(lib().mfpa_psnr_stats(ptr(pred), _dtype_code(pred), ptr(target), B, n, ptr(out), stream()), "mfpa_psnr_stats")
    return out
