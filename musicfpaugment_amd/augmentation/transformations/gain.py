"""Gain (reference augmentation/transformations/gain.py) on the device: x * 10^(gain_db / 20)."""
from __future__ import annotations

from typing import Optional

import torch

from ..._lib import check, lib, ptr, stream
from .. import _up
from ..transform import BaseWaveformTransform
from . import u8, uniform


class Gain(BaseWaveformTransform):
    requires_sample_rate = False

    def __init__(self, min_gain_in_db: float = -18.0, max_gain_in_db: float = 6.0, p: float = 0.5,
                 sample_rate: Optional[int] = None) -> None:
        super().__init__(p=p, sample_rate=sample_rate)
        self.min_gain_in_db = min_gain_in_db
        self.max_gain_in_db = max_gain_in_db
        if self.min_gain_in_db >= self.max_gain_in_db:
            raise ValueError("max_gain_in_db must be higher than min_gain_in_db")

    def randomize_parameters(self, x, sample_rate) -> None:
        self.gain_in_db = uniform(self.min_gain_in_db, self.max_gain_in_db, x.shape[0])
        self.factors = 10 ** (self.gain_in_db / 20)
        self.transform_parameters["gain_factors"] = self.factors[self.transform_parameters["should_apply"]].unsqueeze(1).unsqueeze(1)

    def apply_transform(self, x, sample_rate):
        B, T = x.shape
        y = torch.empty_like(x)
        fac_d, on_d = _up(self.factors, x.device), u8(self.transform_parameters["should_apply"], x.device)
        check(lib().mfpa_scale_rows(ptr(x), B, T, ptr(fac_d), ptr(on_d), 0, ptr(y), stream()), "mfpa_scale_rows")
        return y
