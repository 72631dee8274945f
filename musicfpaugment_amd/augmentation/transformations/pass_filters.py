"""LowPassFilter, HighPassFilter (reference augmentation/transformations/pass_filters.py) on the device: windowed-sinc taps
(julius 0.2.7 restated -- julius is not in the reference tree, parity unpinned) and one FIR pass for the batch."""
from __future__ import annotations

from typing import Optional

from ..transform import BaseWaveformTransform
from . import mel_uniform, sinc_filter


class LowPassFilter(BaseWaveformTransform):
    highpass = False

    def __init__(self, min_cutoff_freq: float = 150.0, max_cutoff_freq: float = 7500.0, p: float = 0.5,
                 sample_rate: Optional[int] = None) -> None:
        super().__init__(p=p, sample_rate=sample_rate)
        self.min_cutoff_freq = min_cutoff_freq
        self.max_cutoff_freq = max_cutoff_freq
        if self.min_cutoff_freq > self.max_cutoff_freq:
            raise ValueError("min_cutoff_freq must not be greater than max_cutoff_freq")

    def randomize_parameters(self, x, sample_rate) -> None:
        self.cutoff_freq = mel_uniform(self.min_cutoff_freq, self.max_cutoff_freq, x.shape[0], integer_bounds=True)
        self.transform_parameters["cutoff_freq"] = self.cutoff_freq[self.transform_parameters["should_apply"]]

    def apply_transform(self, x, sample_rate):
        return sinc_filter(x, self.transform_parameters["should_apply"], self.cutoff_freq, sample_rate, self.highpass)


class HighPassFilter(LowPassFilter):
    highpass = True                                  # x - lowpass(x), pass_filters.py:158-171

    def __init__(self, min_cutoff_freq: float = 20.0, max_cutoff_freq: float = 2400.0, p: float = 0.5,
                 sample_rate: Optional[int] = None) -> None:
        super().__init__(min_cutoff_freq, max_cutoff_freq, p=p, sample_rate=sample_rate)
