"""Recursive filters: cascades of second-order sections (csrc/iir.hip)."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .._lib import check, lib, ptr, require_gpu, stream
from ._args import _apply_mask, _check_apply, _dtype_code, _host_f64, _rows, _upload


SOS_MAX_SECTIONS = 8                   # MFPA_SOS_MAX_SECTIONS
SOS_MAX_SAMPLES = 1 << 30


def sos_normalized(sos) -> np.ndarray:
    """Second-order sections (S, 6) or (B, S, 6), rows b0 b1 b2 a0 a1 a2, as float64 on the host with every row divided by its a0
    (host arithmetic, no GPU).  ValueError: another shape, more than SOS_MAX_SECTIONS sections, a coefficient that is not finite,
    a0 == 0."""
    s = np.array(_host_f64(sos, "sos"))                                      # a copy: it is divided in place below
    if s.ndim not in (2, 3) or s.shape[-1] != 6:
        raise ValueError(f"sos must be (S, 6) or (B, S, 6), got {s.shape}")
    if not 1 <= s.shape[-2] <= SOS_MAX_SECTIONS:
        raise ValueError(f"1 to {SOS_MAX_SECTIONS} sections per filter, got {s.shape[-2]}")
    if not np.all(np.isfinite(s)):
        raise ValueError("sos holds a coefficient that is not finite")
    if np.any(s[..., 3] == 0.0):
        raise ValueError("a section with a0 == 0")
    s = s / s[..., 3:4]
    s[..., 3] = 1.0
    if not np.all(np.isfinite(s)):
        raise ValueError("sos holds a coefficient that is not finite once divided by a0")
    return np.ascontiguousarray(s)


def sosfilt(wav: torch.Tensor, sos, *, apply=None, zi=None, clamp: bool = False):
    """scipy.signal.sosfilt along the rows of (B, T) float32 or float64 samples on the GPU: a cascade of up to 8 second-order
    sections in transposed direct form II, one filter for the batch (sos (S, 6)) or one per row ((B, S, 6)), in one launch.  State
    and arithmetic are float64; a float32 output is the float64 result rounded once.  `sos` (rows b0 b1 b2 a0 a1 a2) is read on the
    host and divided by a0.  `apply` (B,) of booleans: a row with a false entry comes back bit for bit.  `zi` (B, S, 2): scipy's
    initial state; with it the return value is (y, zf), zf (B, S, 2) float64 on the device.  clamp=True limits the output to
    [-1, 1] (torchaudio.functional.lfilter's default)."""
    s = sos_normalized(sos)
    B, T = _rows(wav, "waveform", SOS_MAX_SAMPLES)
    S = s.shape[-2]
    if s.ndim == 3 and s.shape[0] != B:
        raise ValueError(f"per-row sections must be ({B}, S, 6), got {s.shape}")
    _check_apply(apply, B)
    if zi is not None and (not isinstance(zi, torch.Tensor) or tuple(zi.shape) != (B, S, 2)):
        raise ValueError(f"zi must be a ({B}, {S}, 2) tensor")
    require_gpu(wav, "waveform")
    dev = wav.device
    wav = wav.contiguous()
    y = torch.empty_like(wav)
    zi_d = zf = None
    if zi is not None:
        zi_d = zi.to(device=dev, dtype=torch.float64).contiguous()
        zf = zi_d.clone()
    if B == 0 or T == 0:
        return y if zi is None else (y, zf)
    apply_d = _apply_mask(apply, dev)
    per_row = int(s.ndim == 3)
    need = ctypes.c_longlong(0)
    check(lib().mfpa_sosfilt_work(B, S, per_row, ctypes.addressof(need)), "mfpa_sosfilt_work")
    work = torch.empty((need.value,), dtype=torch.float64, device=dev)
    sos_d = _upload(torch.from_numpy(s), dev)
    check(lib().mfpa_sosfilt(ptr(wav), _dtype_code(wav), B, T, ptr(sos_d), S, per_row, ptr(apply_d), ptr(zi_d), ptr(zf), int(bool(clamp)),
                             ptr(work), need.value, ptr(y), stream()), "mfpa_sosfilt")
    return y if zi is None else (y, zf)
