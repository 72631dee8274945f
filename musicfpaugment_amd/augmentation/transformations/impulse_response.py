"""ApplyImpulseResponse (reference augmentation/transformations/impulse_response.py) on the device: full convolution with a random
impulse response of a bank resident in HBM, divided by the peak of the full result, cut to the input length.

The bank is given in memory (`ir_bank=`) or read ONCE at construction from `ir_paths` (.wav files, or directories searched for
them) -- AugmentFP's resident-bank layout and its `resample_banks=` switch; the reference decodes a file per example."""
from __future__ import annotations

import random
from typing import List, Optional

import torch

from ..._lib import check, lib, ptr, stream
from .. import _find_wavs, _read_wav, _up
from ..transform import BaseWaveformTransform, EmptyPathException, ModeNotSupportedException
from . import as_bank, bank_offsets, u8


class ApplyImpulseResponse(BaseWaveformTransform):
    def __init__(self, ir_paths: Optional[List[str]] = None, sample_rate: Optional[int] = None, convolve_mode: str = "full",
                 compensate_for_propagation_delay: bool = False, p: float = 0.5, *, ir_bank: Optional[List[torch.Tensor]] = None,
                 resample_banks: bool = False, device="cuda") -> None:
        super().__init__(p=p, sample_rate=sample_rate)
        if convolve_mode != "full" or compensate_for_propagation_delay:
            raise ModeNotSupportedException("the device convolution is convolve_mode='full' without delay compensation "
                                            "(what AugmentFP uses)")
        if ir_bank is None:
            if ir_paths is None or sample_rate is None:
                raise ValueError("pass `ir_paths` (.wav files or directories) and `sample_rate`, or an in-memory `ir_bank`")
            ir_bank = [_read_wav(f, int(sample_rate), resample_banks) for f in _find_wavs(list(ir_paths))]
        if len(ir_bank) == 0:
            raise EmptyPathException("There are no supported audio files found.")
        self.convolve_mode = convolve_mode
        self.compensate_for_propagation_delay = compensate_for_propagation_delay
        self.ir_bank = as_bank(ir_bank)
        self._ir_off = bank_offsets(self.ir_bank)
        self._ir_dev = torch.cat([i.flip(0) for i in self.ir_bank]).to(torch.device(device))      # time-reversed: FIR taps

    def randomize_parameters(self, x, sample_rate) -> None:
        self.pick = [random.randrange(len(self.ir_bank)) for _ in range(x.shape[0])]
        self.transform_parameters["ir"] = [self.ir_bank[i] for i in self.pick]

    def apply_transform(self, x, sample_rate):
        B, T = x.shape
        dev, L = x.device, lib()
        nlen = [len(self.ir_bank[i]) for i in self.pick]
        n_d = _up(torch.tensor(nlen, dtype=torch.int32), dev)
        off_d = n_d - 1                                              # y[t] = sum_k ir[n-1-k] x[t + k - (n-1)]
        toff_d = _up(torch.from_numpy(self._ir_off[self.pick]), dev)
        y, peak = torch.empty_like(x), torch.empty((B,), dtype=torch.float32, device=dev)
        on_d = u8(self.transform_parameters["should_apply"], dev)
        check(L.mfpa_fir(ptr(x), B, T, T + max(nlen) - 1, ptr(self._ir_dev), ptr(toff_d), ptr(n_d), ptr(off_d), ptr(on_d), 1, 2,
                         ptr(y), ptr(peak), stream()), "mfpa_fir")
        check(L.mfpa_scale_rows(ptr(y), B, T, ptr(peak), ptr(on_d), 1, ptr(y), stream()), "mfpa_scale_rows")
        return y
