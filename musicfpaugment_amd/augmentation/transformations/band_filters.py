"""BandPassFilter, BandStopFilter (reference augmentation/transformations/band_filters.py) on the device: mfpa_bandpass_taps
(julius 0.2.7 BandPassFilter restated -- julius is not in the reference tree, parity unpinned) and ONE pass of mfpa_fir, whose
out_mode gives the band-pass (0) or the band-stop x - bandpass (1)."""
from __future__ import annotations

from typing import Optional

import torch

from ... import ops
from ..._lib import check, lib, ptr, stream
from ..transform import BaseWaveformTransform
from . import mel_uniform, u8, uniform


class BandPassFilter(BaseWaveformTransform):
    out_mode = 0

    def __init__(self, min_center_frequency: int = 200, max_center_frequency: int = 4000, min_bandwidth_fraction: float = 0.5,
                 max_bandwidth_fraction: float = 1.99, p: float = 0.5, sample_rate: Optional[int] = None) -> None:
        super().__init__(p=p, sample_rate=sample_rate)
        self.min_center_frequency = min_center_frequency
        self.max_center_frequency = max_center_frequency
        self.min_bandwidth_fraction = min_bandwidth_fraction
        self.max_bandwidth_fraction = max_bandwidth_fraction
        if max_center_frequency < min_center_frequency:
            raise ValueError(f"max_center_frequency ({max_center_frequency}) should be larger than "
                             f"min_center_frequency ({min_center_frequency}).")
        if min_bandwidth_fraction <= 0.0:
            raise ValueError("min_bandwidth_fraction must be a positive number")
        if max_bandwidth_fraction < min_bandwidth_fraction:
            raise ValueError(f"max_bandwidth_fraction ({max_bandwidth_fraction}) should be larger than "
                             f"min_bandwidth_fraction ({min_bandwidth_fraction}).")
        if max_bandwidth_fraction >= 2.0:
            raise ValueError(f"max_bandwidth_fraction ({max_bandwidth_fraction}) should be smaller than 2.0, "
                             "since otherwise low_cut_frequency of the band can be smaller than 0 Hz.")

    def randomize_parameters(self, x, sample_rate) -> None:
        B, should = x.shape[0], self.transform_parameters["should_apply"]
        self.center_freq = mel_uniform(self.min_center_frequency, self.max_center_frequency, B, integer_bounds=False)
        self.bandwidth = uniform(self.min_bandwidth_fraction, self.max_bandwidth_fraction, B)
        self.transform_parameters.update(center_freq=self.center_freq[should], bandwidth=self.bandwidth[should])

    def apply_transform(self, x, sample_rate):
        B, T = x.shape
        should = self.transform_parameters["should_apply"]
        lo = self.center_freq * (1 - 0.5 * self.bandwidth) / sample_rate
        hi = self.center_freq * (1 + 0.5 * self.bandwidth) / sample_rate
        quarter = torch.full_like(lo, 0.25)                          # an example the gate skips gets a short dummy filter
        taps, off_d, ntaps_d, half_d = ops.bandpass_taps(torch.where(should, lo, quarter), torch.where(should, hi, quarter), x.device)
        y, apply_d = torch.empty_like(x), u8(should, x.device)
        check(lib().mfpa_fir(ptr(x), B, T, T, ptr(taps), ptr(off_d), ptr(ntaps_d), ptr(half_d), ptr(apply_d), 0,
                             self.out_mode, ptr(y), 0, stream()), "mfpa_fir")
        return y


class BandStopFilter(BandPassFilter):
    """Also known as notch filter, band reject filter and frequency mask: x - bandpass(x)."""
    out_mode = 1
