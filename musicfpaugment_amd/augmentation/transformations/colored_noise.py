"""AddColoredNoise (reference augmentation/transformations/colored_noise.py) on the device: for every example one period of
`sample_rate` samples of 1/f^f_decay noise (white noise -> real FFT -> power-law mask -> inverse FFT -> unit RMS, the whole
transform in the LDS of one workgroup: mfpa_colored_noise), tiled to the clip length, mixed in at a random SNR, peak-normalised.

The white noise is ONE torch.normal(0, 1, (B, sample_rate)) on the device per call; the reference draws (sample_rate,) per selected
example, so the two consume the device generator differently -- the noise has the same distribution, not the same samples."""
from __future__ import annotations

from typing import Optional

import torch

from ... import ops
from ..._lib import check, lib, ptr, stream
from .. import _up
from ..transform import BaseWaveformTransform
from . import u8, uniform

DEFAULT_NOISE_RATE = 44100              # colored_noise.py:21-22: what sample_rate=None means to _gen_noise


class AddColoredNoise(BaseWaveformTransform):
    def __init__(self, min_snr_in_db: float = 3.0, max_snr_in_db: float = 30.0, min_f_decay: float = -2.0, max_f_decay: float = 2.0,
                 p: float = 0.5, sample_rate: Optional[int] = None):
        """f_decay: the power decay 1/f^f_decay -- 0 white, 1 pink, 2 brown, -1 blue, -2 violet noise."""
        super().__init__(p=p, sample_rate=sample_rate)
        self.min_snr_in_db = min_snr_in_db
        self.max_snr_in_db = max_snr_in_db
        if self.min_snr_in_db > self.max_snr_in_db:
            raise ValueError("min_snr_in_db must not be greater than max_snr_in_db")
        self.min_f_decay = min_f_decay
        self.max_f_decay = max_f_decay
        if self.min_f_decay > self.max_f_decay:
            raise ValueError("min_f_decay must not be greater than max_f_decay")
        self.noise_period = DEFAULT_NOISE_RATE if sample_rate is None else int(sample_rate)
        try:
            ops.rfft_plan(self.noise_period)       # one period of sample_rate samples is made by the device FFT
        except ValueError as e:
            raise ValueError(f"AddColoredNoise(sample_rate={sample_rate}): {e} -- 8000 and 16000 are taken") from None

    def randomize_parameters(self, x, sample_rate) -> None:
        B, should = x.shape[0], self.transform_parameters["should_apply"]
        self.snr_in_db = uniform(self.min_snr_in_db, self.max_snr_in_db, B)
        self.f_decay = uniform(self.min_f_decay, self.max_f_decay, B)
        self.white = torch.normal(0.0, 1.0, (B, self.noise_period), device=x.device)
        self.transform_parameters.update(snr_in_db=self.snr_in_db[should], f_decay=self.f_decay[should])

    def apply_transform(self, x, sample_rate):
        B, T = x.shape
        noise = ops.colored_noise(self.white, _up(self.f_decay, x.device), T)
        y, snr_d = torch.empty_like(x), _up(self.snr_in_db, x.device)
        on_d = u8(self.transform_parameters["should_apply"], x.device)
        check(lib().mfpa_mix_background(ptr(x), B, T, ptr(noise), ptr(snr_d), ptr(on_d), ptr(y), stream()), "mfpa_mix_background")
        return y

