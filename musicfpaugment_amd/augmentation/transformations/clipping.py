"""Clipping (reference augmentation/transformations/clipping.py) on the device: clamp to the p/2 and 1 - p/2 quantiles, found by
a radix select in LDS.  scope="example" takes each example's own quantiles (what the reference computes for one example at a
time); scope="batch" takes them over all selected examples flattened together, which is what the reference's torch.quantile call
without a dim argument does to a batch of more than one (clipping.py:77-93)."""
from __future__ import annotations

from typing import Optional

import torch

from ..._lib import check, lib, ptr, stream
from .. import _up
from ..transform import BaseWaveformTransform
from . import u8, uniform


class Clipping(BaseWaveformTransform):
    requires_sample_rate = False

    def __init__(self, min_percentile_threshold: float = 0.0, max_percentile_threshold: float = 1.0, p: float = 0.5,
                 sample_rate: Optional[int] = None, *, scope: str = "example") -> None:
        super().__init__(p=p, sample_rate=sample_rate)
        if scope not in ("example", "batch"):
            raise ValueError("scope must be 'example' or 'batch'")
        self.scope = scope
        self.min_percentile_threshold = min_percentile_threshold
        self.max_percentile_threshold = max_percentile_threshold
        if self.min_percentile_threshold > self.max_percentile_threshold:
            raise ValueError("max_percentile_threshold must be > min_percentile_threshold")

    def randomize_parameters(self, x, sample_rate) -> None:
        self.percentile = uniform(self.min_percentile_threshold, self.max_percentile_threshold, x.shape[0])
        self.transform_parameters["percentile_threshold"] = self.percentile[self.transform_parameters["should_apply"]].unsqueeze(1)

    def apply_transform(self, x, sample_rate):
        B, T = x.shape
        should = self.transform_parameters["should_apply"]
        y = torch.empty_like(x)
        pct_d, on_d = _up(self.percentile, x.device), u8(should, x.device)
        if self.scope == "batch" and B > 1:
            check(lib().mfpa_clip_quantile_flat(ptr(x), B, T, ptr(pct_d), ptr(on_d), int(should.sum()), ptr(y), stream()),
                  "mfpa_clip_quantile_flat")
        else:
            check(lib().mfpa_clip_quantile(ptr(x), B, T, ptr(pct_d), ptr(on_d), ptr(y), stream()), "mfpa_clip_quantile")
        return y
