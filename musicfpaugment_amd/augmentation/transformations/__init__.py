"""The reference's augmentation/transformations/ package over the device kernels: one class per module, the reference's import
paths and constructor signatures.  This file holds what the modules share: the host-side uploads and draws AugmentFP uses, the
windowed-sinc filter launch and the resident-bank layout."""
from __future__ import annotations

from typing import List

import numpy as np
import torch

from ..._lib import check, lib, ptr, stream
from .. import ZEROS, _hz, _mels, _up


def u8(mask: torch.Tensor, dev) -> torch.Tensor:
    return _up(mask.to(torch.uint8), dev)


def uniform(lo: float, hi: float, B: int) -> torch.Tensor:
    """Uniform(lo, hi).sample((B,)) with float32 bounds, on the host."""
    return torch.distributions.Uniform(torch.tensor(float(lo)), torch.tensor(float(hi))).sample((B,))


def mel_uniform(lo_hz: float, hi_hz: float, B: int, integer_bounds: bool) -> torch.Tensor:
    """B frequencies uniform in mel space between lo_hz and hi_hz; the pass filters round the mel bounds inwards to integers
    (pass_filters.py:59-82), the band filters do not (band_filters.py:89-112)."""
    lo, hi = _mels(torch.tensor(lo_hz, dtype=torch.float32)), _mels(torch.tensor(hi_hz, dtype=torch.float32))
    if integer_bounds:
        lo, hi = torch.ceil(lo), torch.floor(hi)
    return _hz(torch.distributions.Uniform(low=lo, high=hi, validate_args=True).sample((B,)))


def sinc_filter(x: torch.Tensor, should: torch.Tensor, cut_hz: torch.Tensor, sample_rate: int, highpass: bool) -> torch.Tensor:
    """Low-pass (or x - low-pass) of every selected example of x (B, T) at its own cut-off: mfpa_lowpass_taps + one mfpa_fir, the
    launch sequence of AugmentFP._filter."""
    B, T = x.shape
    frac = (cut_hz / sample_rate).tolist()
    half = []
    for b in range(B):
        if should[b]:
            c = frac[b]
            if not (0.0 < c <= 0.5):
                raise ValueError(f"Buggy cutoff freq. {c}")                # pass_filters.py:103-110
            if ZEROS / c / 2 >= 2 ** 30:
                raise ValueError(f"Buggy cutoff freq. {c}: more than 2^31 taps")
            half.append(int(ZEROS / c / 2))
        else:
            half.append(1)
    dev = x.device
    ntaps = [2 * h + 1 for h in half]
    tap_off = np.concatenate([[0], np.cumsum(ntaps)]).astype(np.int64)
    cutoff_d = _up(torch.tensor([f if s else 0.25 for f, s in zip(frac, should.tolist())], dtype=torch.float32), dev)
    half_d = _up(torch.tensor(half, dtype=torch.int32), dev)
    ntaps_d = _up(torch.tensor(ntaps, dtype=torch.int32), dev)
    off_d = _up(torch.from_numpy(tap_off[:-1].copy()), dev)
    taps = torch.empty((int(tap_off[-1]),), dtype=torch.float32, device=dev)
    check(lib().mfpa_lowpass_taps(ptr(cutoff_d), ptr(half_d), ptr(off_d), B, ptr(taps), stream()), "mfpa_lowpass_taps")
    y = torch.empty_like(x)
    apply_d = u8(should, dev)
    check(lib().mfpa_fir(ptr(x), B, T, T, ptr(taps), ptr(off_d), ptr(ntaps_d), ptr(half_d), ptr(apply_d), 0,
                         1 if highpass else 0, ptr(y), 0, stream()), "mfpa_fir")
    return y


def as_bank(items) -> List[torch.Tensor]:
    return [torch.as_tensor(i, dtype=torch.float32).reshape(-1) for i in items]


def bank_offsets(bank: List[torch.Tensor]) -> np.ndarray:
    """First sample of each item (and the total) when the items lie back to back in one device tensor: AugmentFP's layout."""
    return np.concatenate([[0], np.cumsum([len(i) for i in bank])]).astype(np.int64)
