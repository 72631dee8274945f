"""STFT magnitudes and spectra, the inverse STFT, PSDs and the element-wise conversions (csrc/stft.hip, istft.hip, nplog.hip)."""
from __future__ import annotations

import ctypes
from functools import lru_cache
from typing import Optional, Tuple

import numpy as np
import torch

from .. import _lib
from .._lib import F32, F64, check, lib, ptr, require_gpu, stream
from ._args import _dtype_code, _out_dtype


N_FFT, N_HOP, N_BINS = 512, 256, 257


def audfprint_window() -> np.ndarray:
    """np.hanning(514)[1:-1]  (training/visualisation.py:18, afp/audfprint/peak_extractor.py:257)."""
    return np.hanning(N_FFT + 2)[1:-1]


def dejavu_window() -> np.ndarray:
    """mlab.window_hanning on 512 samples = np.hanning(512)  (afp/dejavu/fingerprint.py:64)."""
    return np.hanning(N_FFT)


@lru_cache(maxsize=16)
def _tables_cached(kind: str, device_index: int) -> torch.Tensor:
    win = audfprint_window() if kind == "audfprint" else dejavu_window()
    return stft_tables(win, torch.device("cuda", device_index))


def stft_tables(window: np.ndarray, device) -> torch.Tensor:
    """Host-side table build (mfpa_stft_tables) + upload: window and FFT twiddles, float64."""
    w = np.ascontiguousarray(window, dtype=np.float64)
    if w.shape != (N_FFT,):
        raise ValueError("window must have 512 points")
    out = np.empty(_lib.STFT_TABLE_LEN, dtype=np.float64)
    check(lib().mfpa_stft_tables(w.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)),
          "mfpa_stft_tables")
    return torch.from_numpy(out).to(device)


def default_tables(device, kind: str = "audfprint") -> torch.Tensor:
    device = torch.device(device)
    return _tables_cached(kind, device.index if device.index is not None else torch.cuda.current_device())


def stft_frames(n_samples: int) -> int:
    return 1 + n_samples // N_HOP


def stft_mag(wav: torch.Tensor, out_dtype=torch.float64, tables: Optional[torch.Tensor] = None,
             want_max: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(B, T_w) float32 -> |STFT| (B, 257, 1 + T_w//256) and per-clip float64 maxima."""
    require_gpu(wav, "waveform")
    if wav.dim() != 2 or wav.dtype != torch.float32:
        raise ValueError("waveform must be (B, T) float32")
    wav = wav.contiguous()
    B, T_w = wav.shape
    if T_w <= N_HOP:
        raise ValueError("reflect padding needs more than 256 samples per clip")
    if tables is None:
        tables = default_tables(wav.device)
    nF = stft_frames(T_w)
    mag = torch.empty((B, N_BINS, nF), dtype=out_dtype, device=wav.device)
    cmax = torch.empty((B,), dtype=torch.float64, device=wav.device) if want_max else None
    check(lib().mfpa_stft_mag(ptr(wav), B, T_w, ptr(tables), ptr(mag), _dtype_code(mag), ptr(cmax), stream()),
          "mfpa_stft_mag")
    return mag, cmax


def stft_complex(wav: torch.Tensor, tables: Optional[torch.Tensor] = None, want_mag: bool = False, mag_dtype=torch.float64):
    """(B, T_w) float32 -> torch.stft(wav.double(), 512, 256, window=w, return_complex=True): (B, 257, 1 + T_w//256) complex128.
    want_mag=True returns (spec, mag, clip_max) from the one transform, mag and clip_max bit for bit stft_mag(wav, mag_dtype)'s."""
    require_gpu(wav, "waveform")
    if wav.dim() != 2 or wav.dtype != torch.float32:
        raise ValueError("waveform must be (B, T) float32")
    if mag_dtype not in (torch.float32, torch.float64):
        raise ValueError("mag_dtype must be torch.float32 or torch.float64")
    wav = wav.contiguous()
    B, T_w = wav.shape
    if T_w <= N_HOP:
        raise ValueError("reflect padding needs more than 256 samples per clip")
    if tables is None:
        tables = default_tables(wav.device)
    nF = stft_frames(T_w)
    spec = torch.empty((B, N_BINS, nF), dtype=torch.complex128, device=wav.device)
    mag = torch.empty((B, N_BINS, nF), dtype=mag_dtype, device=wav.device) if want_mag else None
    cmax = torch.empty((B,), dtype=torch.float64, device=wav.device) if want_mag else None
    check(lib().mfpa_stft_complex(ptr(wav), B, T_w, ptr(tables), ptr(spec), ptr(mag), F32 if mag_dtype == torch.float32 else F64,
                                  ptr(cmax), stream()), "mfpa_stft_complex")
    return (spec, mag, cmax) if want_mag else spec


ISTFT_CLAMP = 1                        # MFPA_ISTFT_CLAMP
ISTFT_ENVELOPE_MIN = 1e-11             # torch.istft refuses a smaller overlap-added squared window


def istft_envelope_min(window: np.ndarray, n_frames: int, length: int) -> float:
    """Minimum of the overlap-added squared window over the samples istft keeps (mfpa_istft_envelope_min: host arithmetic)."""
    w = np.ascontiguousarray(window, dtype=np.float64)
    if w.shape != (N_FFT,):
        raise ValueError("window must have 512 points")
    out = ctypes.c_double(0.0)
    check(lib().mfpa_istft_envelope_min(w.ctypes.data_as(ctypes.c_void_p), int(n_frames), int(length), ctypes.addressof(out)),
          "mfpa_istft_envelope_min")
    return out.value


@lru_cache(maxsize=64)
def _default_envelope_min(n_frames: int, length: int) -> float:
    return istft_envelope_min(audfprint_window(), n_frames, length)


def istft(spec: torch.Tensor, length: Optional[int] = None, mag: Optional[torch.Tensor] = None,
          denom: Optional[torch.Tensor] = None, clamp: bool = False, out_dtype=torch.float32,
          tables: Optional[torch.Tensor] = None) -> torch.Tensor:
    """torch.istft(Z, 512, 256, window=w, center=True, length=length) of a (B, 257, n_frames) complex128 spectrum -> (B, length).
    mag=None: Z = spec.  Otherwise Z = m * spec / |spec| with m = mag * denom[b] (mag (B, 257, n_frames) float32 or float64, denom
    (B,) float64 or None), phase 0 where spec is 0; clamp=True turns a negative m into 0.  length=None is 256 * (n_frames - 1), as in
    torch; any length an STFT with n_frames frames can have come from is taken.  With `tables` given, its window is read back from
    the device for torch's "window overlap add min" check (the default tables need no copy)."""
    require_gpu(spec, "spectrum")
    if spec.dim() != 3 or spec.shape[1] != N_BINS or spec.dtype != torch.complex128:
        raise ValueError("spectrum must be (B, 257, n_frames) complex128")
    _out_dtype(out_dtype)
    B, _, nF = spec.shape
    if nF < 2:
        raise ValueError("istft needs at least 2 frames")
    if length is None:
        length = N_HOP * (nF - 1)
    length = int(length)
    if not N_HOP * (nF - 1) <= length < N_HOP * nF:
        raise ValueError(f"length must be in [{N_HOP * (nF - 1)}, {N_HOP * nF}) for {nF} frames, got {length}")
    if B > 65535:
        raise ValueError("at most 65535 clips per call")
    if mag is not None:
        require_gpu(mag, "magnitude")
        if mag.shape != spec.shape or mag.dtype not in (torch.float32, torch.float64):
            raise ValueError("magnitude must be (B, 257, n_frames) float32 or float64")
        mag = mag.contiguous()
        if denom is not None:
            require_gpu(denom, "denominator")
            if denom.shape != (B,) or denom.dtype != torch.float64:
                raise ValueError("denom must be (B,) float64")
            denom = denom.contiguous()
    elif denom is not None or clamp:
        raise ValueError("denom and clamp belong to mag")
    if tables is None:
        tables = default_tables(spec.device)
        env_min = _default_envelope_min(nF, length)
    else:
        require_gpu(tables, "tables")
        if tables.shape != (_lib.STFT_TABLE_LEN,) or tables.dtype != torch.float64:
            raise ValueError(f"tables must be ({_lib.STFT_TABLE_LEN},) float64 (stft_tables)")
        env_min = istft_envelope_min(tables[:N_FFT].cpu().numpy(), nF, length)
    if not env_min >= ISTFT_ENVELOPE_MIN:
        raise RuntimeError(f"istft: window overlap add min: {env_min}")      # torch's refusal (its message ends "window overlap add min: 1")
    spec = spec.contiguous()
    out = torch.empty((B, length), dtype=out_dtype, device=spec.device)
    check(lib().mfpa_istft(ptr(spec), ptr(mag), _dtype_code(mag) if mag is not None else F32, ptr(denom),
                           ISTFT_CLAMP if clamp else 0, B, nF, length, ptr(tables), ptr(out), _dtype_code(out), stream()),
          "mfpa_istft")
    return out


def specgram_psd(wav: torch.Tensor, scale_in: float = 1.0, tables: Optional[torch.Tensor] = None):
    """(B, T_w) float32 -> mlab.specgram-style PSD (B, 257, (T_w-256)//256) float64 (unscaled) + clip maxima."""
    require_gpu(wav, "waveform")
    if wav.dim() != 2 or wav.dtype != torch.float32:
        raise ValueError("waveform must be (B, T) float32")
    wav = wav.contiguous()
    B, T_w = wav.shape
    if T_w < N_FFT:
        raise ValueError("need at least one full 512-sample frame")
    if tables is None:
        tables = default_tables(wav.device, "dejavu")
    nF = (T_w - 256) // 256
    psd = torch.empty((B, N_BINS, nF), dtype=torch.float64, device=wav.device)
    cmax = torch.empty((B,), dtype=torch.float64, device=wav.device)
    check(lib().mfpa_specgram_psd(ptr(wav), B, T_w, float(scale_in), ptr(tables), ptr(psd), ptr(cmax), stream()),
          "mfpa_specgram_psd")
    return psd, cmax


def normalize_(data: torch.Tensor, clip_max: torch.Tensor, per_clip: bool) -> torch.Tensor:
    """In-place data[b] /= (clip_max[b] if per_clip else max(clip_max))."""
    require_gpu(data, "data")
    B = data.shape[0]
    if clip_max.shape != (B,) or clip_max.dtype != torch.float64:
        raise ValueError("clip_max must be (B,) float64")
    n = data[0].numel() if B else 0
    check(lib().mfpa_normalize(ptr(data), _dtype_code(data), B, n, ptr(clip_max), int(per_clip), stream()),
          "mfpa_normalize")
    return data


def nplog_f32(x: torch.Tensor) -> torch.Tensor:
    """Element-wise numpy float32 log (mfpa_nplog_f32): float32 tensor of any shape -> np.log(x) as numpy's SIMD kernel returns it,
    bit for bit (csrc/mfpa_nplog.h).  For callers that post-process float32 spectrograms themselves."""
    require_gpu(x)
    if x.dtype != torch.float32:
        raise TypeError("float32 expected")
    x = x.contiguous()
    out = torch.empty_like(x)
    check(lib().mfpa_nplog_f32(ptr(x), ptr(out), x.numel(), stream()), "mfpa_nplog_f32")
    return out


def f64_to_f32(x: torch.Tensor) -> torch.Tensor:
    require_gpu(x)
    if x.dtype != torch.float64:
        raise TypeError("float64 expected")
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    check(lib().mfpa_f64_to_f32(ptr(x), ptr(out), x.numel(), stream()), "mfpa_f64_to_f32")
    return out
