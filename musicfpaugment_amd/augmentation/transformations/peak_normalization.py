"""PeakNormalization (reference augmentation/transformations/peak_normalization.py) on the device: x / max|x| where the peak is
above zero."""
from __future__ import annotations

from typing import Optional

import torch

from ..._lib import check, lib, ptr, stream
from ..transform import BaseWaveformTransform
from . import u8


class PeakNormalization(BaseWaveformTransform):
    requires_sample_rate = False

    def __init__(self, p: float = 0.5, sample_rate: Optional[int] = None):
        super().__init__(p=p, sample_rate=sample_rate)

    def apply_transform(self, x, sample_rate):
        B, T = x.shape
        should = self.transform_parameters["should_apply"]
        y = torch.empty_like(x)
        on_d = None if bool(should.all()) else u8(should, x.device)       # every example selected: no gate to upload
        check(lib().mfpa_mix_background(ptr(x), B, T, 0, 0, ptr(on_d), ptr(y), stream()), "mfpa_mix_background")
        return y
