"""Windowed-sinc resampling, dense and sparse-tap (csrc/resample.hip)."""
from __future__ import annotations

import ctypes
from functools import lru_cache
from typing import Optional, Tuple

import numpy as np
import torch

from .._lib import check, lib, ptr, require_gpu, stream


RESAMPLE_LOWPASS_FILTER_WIDTH = 6      # torchaudio.transforms.Resample's defaults (sinc_interp_hann); torchaudio is not in the
RESAMPLE_ROLLOFF = 0.99                # reference tree, so parity with it is unpinned
RESAMPLE_TAP_ALIGN = 16                # MFPA_RESAMPLE_TAP_ALIGN


def resample_geometry(orig_freq: int, new_freq: int, T: int = 0) -> Tuple[int, int, int, int, int]:
    """(o, n, width, taps per phase, Tout) of torchaudio.transforms.Resample(orig_freq, new_freq) for T input samples
    (mfpa_resample_geometry: host arithmetic)."""
    o, n, width, ntaps = (ctypes.c_int(0) for _ in range(4))
    tout = ctypes.c_longlong(0)
    check(lib().mfpa_resample_geometry(int(orig_freq), int(new_freq), RESAMPLE_LOWPASS_FILTER_WIDTH, RESAMPLE_ROLLOFF, int(T),
                                       ctypes.addressof(o), ctypes.addressof(n), ctypes.addressof(width), ctypes.addressof(ntaps),
                                       ctypes.addressof(tout)), "mfpa_resample_geometry")
    return o.value, n.value, width.value, ntaps.value, int(tout.value)


def resample_tile(orig_freq: int, new_freq: int) -> int:
    """Frames (groups of n output / o input samples) one workgroup of the resampling kernel owns for this pair of rates."""
    o, n, width, _, _ = resample_geometry(orig_freq, new_freq)
    tile = lib().mfpa_resample_tile(o, n, width)
    check(min(tile, 0), "mfpa_resample_tile")
    return tile


@lru_cache(maxsize=256)                 # augmentation PitchShift's default set alone is 36 ratios (q <= 16 within +-4 semitones)
def _resample_taps_cached(o: int, n: int, device_index: int) -> torch.Tensor:
    _, _, width, ntaps, _ = resample_geometry(o, n)
    taps = np.empty((n, resample_tap_pitch(ntaps)), dtype=np.float32)
    check(lib().mfpa_resample_taps(o, n, width, RESAMPLE_LOWPASS_FILTER_WIDTH, RESAMPLE_ROLLOFF,
                                   taps.ctypes.data_as(ctypes.c_void_p)), "mfpa_resample_taps")
    return torch.from_numpy(taps).to(torch.device("cuda", device_index))


def resample_tap_pitch(ntaps: int) -> int:
    """MFPA_RESAMPLE_TAP_PITCH: floats from the taps of one phase to the next in the bank."""
    return (ntaps + RESAMPLE_TAP_ALIGN - 1) // RESAMPLE_TAP_ALIGN * RESAMPLE_TAP_ALIGN


def resample_taps(orig_freq: int, new_freq: int, device) -> torch.Tensor:
    """The filter bank of the pair of rates, phase-major (n, resample_tap_pitch(taps per phase)) float32 on `device`, zero behind
    the taps of each row (mfpa_resample_taps: built on the host in float64, uploaded once per (o, n, device))."""
    o, n, _, _, _ = resample_geometry(orig_freq, new_freq)
    device = torch.device(device)
    return _resample_taps_cached(o, n, device.index if device.index is not None else torch.cuda.current_device())


RESAMPLE_ANY_RATIO_HINT = ("the dense resampling kernel does not take this pair of rates (at most 1024 phases and 8192 taps per phase after "
                           "reduction by the gcd); pass any_ratio=True for the sparse-tap kernel, which takes every pair below 65536 Hz")


def resample_sparse_geometry(orig_freq: int, new_freq: int, T: int = 0) -> Tuple[int, int, int, int, int]:
    """(o, n, width, support, Tout) of the sparse-tap resampler for T input samples (mfpa_resample_sparse_geometry: host arithmetic).
    support = 2 * width + 1 rounded up to a multiple of 4: the taps it keeps per phase."""
    o, n, width, support = (ctypes.c_int(0) for _ in range(4))
    tout = ctypes.c_longlong(0)
    check(lib().mfpa_resample_sparse_geometry(int(orig_freq), int(new_freq), RESAMPLE_LOWPASS_FILTER_WIDTH, RESAMPLE_ROLLOFF, int(T),
                                              ctypes.addressof(o), ctypes.addressof(n), ctypes.addressof(width), ctypes.addressof(support),
                                              ctypes.addressof(tout)), "mfpa_resample_sparse_geometry")
    return o.value, n.value, width.value, support.value, int(tout.value)


def resample_sparse_tile(orig_freq: int, new_freq: int) -> int:
    """Consecutive output samples one workgroup of the sparse-tap resampling kernel owns for this pair of rates."""
    o, n, width, _, _ = resample_sparse_geometry(orig_freq, new_freq)
    tile = lib().mfpa_resample_sparse_tile(o, n, width)
    check(min(tile, 0), "mfpa_resample_sparse_tile")
    return tile


@lru_cache(maxsize=64)                  # 8979 : 8000 is 512 KB; the largest table (65536 phases of 512 taps) is 128 MB
def _resample_sparse_taps_cached(o: int, n: int, device_index: int) -> Tuple[torch.Tensor, torch.Tensor]:
    _, _, width, support, _ = resample_sparse_geometry(o, n)
    taps = np.empty((n, support), dtype=np.float32)
    first = np.empty((n,), dtype=np.int32)
    check(lib().mfpa_resample_sparse_taps(o, n, width, RESAMPLE_LOWPASS_FILTER_WIDTH, RESAMPLE_ROLLOFF, taps.ctypes.data_as(ctypes.c_void_p),
                                          first.ctypes.data_as(ctypes.c_void_p)), "mfpa_resample_sparse_taps")
    dev = torch.device("cuda", device_index)
    return torch.from_numpy(taps).to(dev), torch.from_numpy(first).to(dev)


def resample_sparse_taps(orig_freq: int, new_freq: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """(taps (n, support) float32, first (n,) int32) on `device`: row i holds taps first[i] .. first[i] + support - 1 of phase i of the
    dense bank, every tap it leaves out being 0.0f (mfpa_resample_sparse_taps proves it; built on the host, uploaded once per
    (o, n, device))."""
    o, n, _, _, _ = resample_sparse_geometry(orig_freq, new_freq)
    device = torch.device(device)
    return _resample_sparse_taps_cached(o, n, device.index if device.index is not None else torch.cuda.current_device())


def resample_kernel_for(orig_freq: int, new_freq: int, any_ratio: bool = False, kernel: Optional[str] = None) -> str:
    """"dense" or "sparse": the kernel a pair of rates takes -- the dense one unless kernel="sparse" forces the sparse one, or
    any_ratio=True and the dense kernel refuses the pair.  A pair that is left without a kernel is a ValueError; without any_ratio
    its text names the flag."""
    if kernel not in (None, "dense", "sparse"):
        raise ValueError(f'kernel must be None, "dense" or "sparse", got {kernel!r}')
    if kernel == "sparse":
        resample_sparse_geometry(orig_freq, new_freq)
        return "sparse"
    try:
        resample_geometry(orig_freq, new_freq)
        return "dense"
    except ValueError:
        if kernel == "dense" or not any_ratio:
            raise ValueError(f"resample({orig_freq}, {new_freq}): {RESAMPLE_ANY_RATIO_HINT}") from None
    resample_sparse_geometry(orig_freq, new_freq)
    return "sparse"


def resample(wav: torch.Tensor, orig_freq: int, new_freq: int, *, any_ratio: bool = False, kernel: Optional[str] = None) -> torch.Tensor:
    """torchaudio.transforms.Resample(orig_freq, new_freq) of (B, T) float32 on the GPU -> (B, ceil(T * new / orig)).  Equal rates
    return `wav` itself, like torchaudio.  any_ratio=True: a pair of rates the dense kernel refuses (more than 1024 phases or 8192
    taps per phase) takes the sparse-tap kernel, which walks only the taps that are not zero; a pair the dense kernel takes still
    takes it.  kernel="sparse" forces the sparse kernel for any pair it accepts (same float32 values as the dense kernel, up to the
    sign of a zero); kernel="dense" and None are the default routing."""
    require_gpu(wav, "waveform")
    if wav.dim() != 2 or wav.dtype != torch.float32:
        raise ValueError("waveform must be (B, T) float32")
    if int(orig_freq) <= 0 or int(new_freq) <= 0:
        raise ValueError("Original frequency and desired frequecy should be positive")       # torchaudio's own message
    if int(orig_freq) == int(new_freq):
        return wav
    wav = wav.contiguous()
    B, T = wav.shape
    if resample_kernel_for(orig_freq, new_freq, any_ratio, kernel) == "sparse":
        o, n, width, support, Tout = resample_sparse_geometry(orig_freq, new_freq, T)
        out = torch.empty((B, Tout), dtype=torch.float32, device=wav.device)
        if B == 0 or Tout == 0:
            return out
        taps, first = resample_sparse_taps(orig_freq, new_freq, wav.device)
        check(lib().mfpa_resample_sparse(ptr(wav), B, T, T, o, n, width, support, ptr(taps), ptr(first), ptr(out), Tout, Tout, stream()),
              "mfpa_resample_sparse")
        return out
    o, n, width, _, Tout = resample_geometry(orig_freq, new_freq, T)
    out = torch.empty((B, Tout), dtype=torch.float32, device=wav.device)
    if B == 0 or Tout == 0:
        return out
    taps = resample_taps(orig_freq, new_freq, wav.device)
    check(lib().mfpa_resample(ptr(wav), B, T, T, o, n, width, ptr(taps), ptr(out), Tout, Tout, stream()), "mfpa_resample")
    return out
