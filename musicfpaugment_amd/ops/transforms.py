"""Composable transforms: FIR band-pass taps, the real FFT, coloured noise (csrc/transforms.hip)."""
from __future__ import annotations

import ctypes
from functools import lru_cache
from typing import Tuple

import numpy as np
import torch

from .._lib import check, lib, ptr, require_gpu, stream
from ._args import _current_gpu, _host_tensor, _upload


RFFT_MAX_N = 16384                     # MFPA_RFFT_MAX_N: N/2 complex points in one 64 KiB LDS buffer
RFFT_MAX_RADICES = 16                  # MFPA_RFFT_MAX_RADICES
FILTER_ZEROS = 8                       # julius' default; half = int(zeros / cutoff / 2)


def bandpass_taps(cut_lo, cut_hi, device=None):
    """Band-pass taps (julius 0.2.7 BandPassFilter restated; parity unpinned) for B pairs of cut-offs, fractions of the sample
    rate with 0 < lo <= hi <= 0.5, given on the host.  Returns the arguments mfpa_fir wants, on the device:
    (taps, tap_off int64 (B,), ntaps int32 (B,), half int32 (B,)); example b owns taps[tap_off[b] : tap_off[b] + ntaps[b]],
    ntaps = 2 * half + 1, half = int(8 / lo / 2) from the cut-off as given (a float32 tensor's values, or Python floats in
    double); the taps themselves are float32 arithmetic on the float32 cut-offs."""
    dev = _current_gpu(device)
    lo, hi = _host_tensor(cut_lo, "cut_lo"), _host_tensor(cut_hi, "cut_hi")
    if lo.shape != hi.shape:
        raise ValueError("cut_lo and cut_hi must have one entry per example")
    half = []
    for l, h in zip(lo.tolist(), hi.tolist()):
        if h > 0.5 or l > 0.5:
            raise ValueError("A cutoff above 0.5 does not make sense.")                  # julius' own message
        if not (0.0 < l <= h):
            raise ValueError(f"band cut-offs must satisfy 0 < low <= high, got ({l}, {h})")
        if FILTER_ZEROS / l / 2 >= 2 ** 30:
            raise ValueError(f"low cut-off {l}: more than 2^31 taps")
        half.append(int(FILTER_ZEROS / l / 2))
    B = len(half)
    ntaps = [2 * h + 1 for h in half]
    off = np.concatenate([[0], np.cumsum(ntaps)]).astype(np.int64)
    taps = torch.empty((int(off[-1]),), dtype=torch.float32, device=dev)
    off_d = _upload(torch.from_numpy(off[:-1].copy()), dev)
    ntaps_d, half_d = _upload(torch.tensor(ntaps, dtype=torch.int32), dev), _upload(torch.tensor(half, dtype=torch.int32), dev)
    lo_d, hi_d = _upload(lo.to(torch.float32), dev), _upload(hi.to(torch.float32), dev)
    if B:
        with torch.cuda.device(dev):
            check(lib().mfpa_bandpass_taps(ptr(lo_d), ptr(hi_d), ptr(half_d), ptr(off_d), B, ptr(taps),
                                           stream()), "mfpa_bandpass_taps")
    return taps, off_d, ntaps_d, half_d


def rfft_plan(N: int) -> Tuple[Tuple[int, ...], int]:
    """(radices of the N/2-point complex passes, LDS bytes of the workgroup) of the device real FFT, or ValueError for an N it
    does not take (mfpa_rfft_plan: host integers only)."""
    radices = (ctypes.c_int * RFFT_MAX_RADICES)()
    n, lds = ctypes.c_int(0), ctypes.c_int(0)
    N = int(N)
    if not -2 ** 31 <= N < 2 ** 31 or lib().mfpa_rfft_plan(N, ctypes.addressof(radices), ctypes.addressof(n),
                                                           ctypes.addressof(lds)) != 0:
        raise ValueError(f"the device FFT takes an even N with 4 <= N <= {RFFT_MAX_N} and N/2 = 2^a 3^b 5^c, not {N}")
    return tuple(radices[:n.value]), lds.value


@lru_cache(maxsize=16)
def _rfft_twiddles_cached(N: int, device_index: int) -> torch.Tensor:
    tw = np.empty(2 * N, dtype=np.float32)
    check(lib().mfpa_rfft_twiddles(N, tw.ctypes.data_as(ctypes.c_void_p)), "mfpa_rfft_twiddles")
    return torch.from_numpy(tw).to(torch.device("cuda", device_index))


def rfft_twiddles(N: int, device) -> torch.Tensor:
    """exp(-2 pi i q / N), q < N, as (2N,) float32 on `device` (mfpa_rfft_twiddles: float64 on the host, rounded once, uploaded
    once per (N, device))."""
    rfft_plan(N)
    return _rfft_twiddles_cached(int(N), _current_gpu(device).index)


def colored_noise(white: torch.Tensor, f_decay: torch.Tensor, num_samples: int) -> torch.Tensor:
    """AddColoredNoise._gen_noise for a batch: white (B, N) float32 normal draws and f_decay (B,) on the GPU -> (B, num_samples)
    unit-RMS noise with a 1/f^f_decay amplitude profile, one period of N samples tiled to num_samples."""
    _current_gpu()
    require_gpu(white, "white noise")
    require_gpu(f_decay, "f_decay")
    if white.dim() != 2 or white.dtype != torch.float32:
        raise ValueError("white must be (B, N) float32")
    B, N = white.shape
    rfft_plan(N)
    if f_decay.shape != (B,) or f_decay.dtype != torch.float32:
        raise ValueError("f_decay must be (B,) float32")
    T = int(num_samples)
    if not 1 <= T < 2 ** 31:
        raise ValueError("num_samples must be at least 1")
    white, f_decay = white.contiguous(), f_decay.contiguous()
    out = torch.empty((B, T), dtype=torch.float32, device=white.device)
    if B == 0:
        return out
    check(lib().mfpa_colored_noise(ptr(white), B, N, ptr(f_decay), T, ptr(rfft_twiddles(N, white.device)), ptr(out), stream()),
          "mfpa_colored_noise")
    return out
