"""Spectral noise suppression: minimum statistics and the Wiener gain (csrc/denoise.hip)."""
from __future__ import annotations

import math
from typing import Tuple

import numpy as np
import torch

from .._lib import check, lib, ptr, require_gpu, stream
from ._args import _apply_mask, _check_apply, _dtype_code, _is_number, _out_dtype, _row_values, _upload


DENOISE_MAX_WINDOW = 128               # MFPA_DENOISE_MAX_WINDOW: back + ahead + 1 at most
DENOISE_MAX_FRAMES = 16384


def suppress_thresholds(xi_min_db: float = -25.0, floor_db: float = -20.0) -> Tuple[float, float]:
    """(xi_min, g_floor) = (10^(xi_min_db / 10), 10^(floor_db / 20)) as Python floats (host arithmetic, `**`): the a-priori SNR is a
    power ratio, the gain floor an amplitude ratio.  The C entry point takes these two numbers."""
    for name, v in (("xi_min_db", xi_min_db), ("floor_db", floor_db)):
        if not _is_number(v) or not math.isfinite(v):
            raise ValueError(f"{name} must be a finite number, got {v!r}")
    if floor_db > 0:
        raise ValueError(f"floor_db must not be positive (a gain floor above 1), got {floor_db}")
    return 10.0 ** (float(xi_min_db) / 10.0), 10.0 ** (float(floor_db) / 20.0)


def _row_floors(floor_db, B: int):
    """floor_db one value per clip -> (B,) float64 gain floors on the host, each suppress_thresholds's."""
    f = _row_values(floor_db, B, "floor_db", "clip")
    if np.any(f > 0):
        raise ValueError(f"floor_db must not be positive (a gain floor above 1), got {floor_db}")
    return np.array([suppress_thresholds(-25.0, float(v))[1] for v in f], dtype=np.float64)


def spectral_suppress(mag: torch.Tensor, *, alpha: float = 0.7, back: int = 48, ahead: int = 48, bias: float = 3.0, dd: float = 0.9,
                      xi_min_db: float = -25.0, floor_db: float = -20.0, noise_psd=None, denom=None, apply=None, out_dtype=None,
                      return_gain: bool = False, return_noise: bool = False):
    """A model-free noise suppressor on (B, F, nF) float32 or float64 STFT magnitudes with the frames contiguous (the layout of
    stft_mag), in one launch (the definition: include/mfpa.h, mfpa_spectral_suppress): the periodogram smoothed with `alpha`, its
    minimum over the frames [t - back, t + ahead] times `bias` as the noise PSD (minimum statistics, Martin 2001, plain windowed
    form), the decision-directed a-priori SNR with weight `dd` (Ephraim and Malah 1984) floored at `xi_min_db` dB, and the Wiener
    gain xi / (1 + xi) floored at `floor_db` dB, a number or one value per clip (suppress_thresholds turns the two dB values into numbers).  At the pipeline's hop
    of 256 samples at 8 kHz the default window is 3.1 s; dd = 0.9, not the usual 0.98, because a frame is 32 ms here.
    `noise_psd` (B, F) float64 replaces the tracker (no bias); `denom` (B,) float64 divides each clip's output; `apply` (B,) of
    booleans: a clip with a false entry has gain 1.  back + ahead + 1 <= DENOISE_MAX_WINDOW, nF <= DENOISE_MAX_FRAMES.  Float64
    arithmetic without contraction: the result equals tests/_denoise_oracle.py bit for bit.  Returns y (B, F, nF) in `out_dtype`
    (the input's dtype without it; float32 is the float64 value rounded once), then g and n as float64 (B, F, nF) when
    return_gain / return_noise ask for them."""
    if not isinstance(mag, torch.Tensor) or mag.dim() != 3 or mag.dtype not in (torch.float32, torch.float64):
        raise ValueError("magnitudes must be a (B, F, nF) float32 or float64 tensor")
    B, F, nF = mag.shape
    out_dtype = _out_dtype(out_dtype, mag.dtype)
    per_row = not _is_number(floor_db)
    floors = _row_floors(floor_db, B) if per_row else None
    xi_min, g_floor = suppress_thresholds(xi_min_db, -20.0 if per_row else floor_db)
    for name, v in (("alpha", alpha), ("dd", dd)):
        if not _is_number(v) or not 0.0 <= v < 1.0:
            raise ValueError(f"{name} must be a number in [0, 1), got {v!r}")
    if not _is_number(bias) or not (bias > 0.0 and math.isfinite(bias)):
        raise ValueError(f"bias must be positive and finite, got {bias!r}")
    for name, v in (("back", back), ("ahead", ahead)):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or v < 0:
            raise ValueError(f"{name} must be an integer that is not negative, got {v!r}")
    if back + ahead + 1 > DENOISE_MAX_WINDOW:
        raise ValueError(f"back + ahead + 1 must not exceed {DENOISE_MAX_WINDOW}, got {back + ahead + 1}")
    if B < 1 or F < 1 or nF < 1 or B > 65535 or F > (1 << 20) or nF > DENOISE_MAX_FRAMES:
        raise ValueError(f"1 <= B <= 65535, 1 <= F <= 2^20, 1 <= nF <= {DENOISE_MAX_FRAMES}, got {tuple(mag.shape)}")
    for name, t, shape in (("noise_psd", noise_psd, (B, F)), ("denom", denom, (B,))):
        if t is not None and (not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != torch.float64):
            raise ValueError(f"{name} must be a {shape} float64 tensor")
    _check_apply(apply, B, "clip")
    require_gpu(mag, "magnitudes")
    dev = mag.device
    for name, t in (("noise_psd", noise_psd), ("denom", denom)):
        if t is not None:
            require_gpu(t, name)
    mag = mag.contiguous()
    noise_psd = noise_psd.contiguous() if noise_psd is not None else None
    denom = denom.contiguous() if denom is not None else None
    y = torch.empty((B, F, nF), dtype=out_dtype, device=dev)
    g = torch.empty((B, F, nF), dtype=torch.float64, device=dev) if return_gain else None
    n = torch.empty((B, F, nF), dtype=torch.float64, device=dev) if return_noise else None
    apply_d = _apply_mask(apply, dev)
    floors_d = _upload(torch.from_numpy(floors), dev) if per_row else None
    check(lib().mfpa_spectral_suppress(ptr(mag), _dtype_code(mag), B, F, nF, float(alpha), int(back), int(ahead), float(bias), float(dd),
                                       xi_min, g_floor, ptr(floors_d), ptr(noise_psd), ptr(denom), ptr(apply_d), ptr(y), _dtype_code(y), ptr(g), ptr(n),
                                       stream()), "mfpa_spectral_suppress")
    out = (y,) + ((g,) if return_gain else ()) + ((n,) if return_noise else ())
    return out if len(out) > 1 else y
