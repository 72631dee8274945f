"""TimeStretch (the tempo change fingerprinting papers test first; the reference has none) on the device: ops.time_stretch -- one
stft_complex, one phase vocoder launch (csrc/vocoder.hip, a rate per example) and one istft for the selected examples.  The output
keeps the input's length: a faster clip is zero-padded at its end, a slower one cropped.  A rate below 1 loses level (torchaudio's
algorithm repeats frame 0: DESIGN.md section 3.14)."""
from __future__ import annotations

from typing import Optional

import torch

from ... import ops
from .. import _up
from ..transform import BaseWaveformTransform
from . import uniform


class TimeStretch(BaseWaveformTransform):
    def __init__(self, min_rate: float = 0.8, max_rate: float = 1.25, p: float = 0.5, sample_rate: Optional[int] = None) -> None:
        super().__init__(p=p, sample_rate=sample_rate)
        if not 0.0 < min_rate <= max_rate:
            raise ValueError("rates must satisfy 0 < min_rate <= max_rate")
        self.min_rate, self.max_rate = min_rate, max_rate

    def randomize_parameters(self, x, sample_rate) -> None:
        B = x.shape[0]
        self.rates = uniform(self.min_rate, self.max_rate, B) if self.min_rate < self.max_rate else torch.full((B,), float(self.min_rate))
        self.transform_parameters["rates"] = self.rates[self.transform_parameters["should_apply"]]

    def apply_transform(self, x, sample_rate):
        B, T = x.shape
        should = self.transform_parameters["should_apply"]
        rows = torch.nonzero(should).flatten()                                # host-known indices: no device-side nonzero
        y = x.clone()
        if rows.numel() == 0:
            return y
        sel = _up(rows, x.device)
        stretched, _ = ops.time_stretch(x.index_select(0, sel), self.rates[should].to(torch.float64))
        W = min(T, stretched.shape[1])
        fitted = torch.zeros((rows.numel(), T), dtype=torch.float32, device=x.device)
        fitted[:, :W] = stretched[:, :W]                                       # rows are zero at and beyond their own length
        y.index_copy_(0, sel, fitted)
        return y
