"""LossyCodec, TelephoneChannel: the lossy-coding entries of the classic fingerprint-robustness battery (MP3 / AAC at a low bit rate,
the telephone channel).  They are not in the reference tree; the conventions are dynamics.py's.  The gate comes first, then one draw
per example for the whole batch on the host, then ONE launch of csrc/codec.hip with per-row parameters and the gate as `apply`
(ops.transform_codec; ops.mu_law behind the band-pass launch of band_filters.py for the telephone).  Both SIMULATE what such a codec
does to a signal: parity with a real MP3, AAC, GSM or G.711 encoder is unpinned."""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from ... import ops
from ..._lib import check, lib, ptr, require_gpu, stream
from ..transform import BaseWaveformTransform
from . import u8, uniform
from .dynamics import _check_range


class LossyCodec(BaseWaveformTransform):
    """The simulated transform codec at a bit rate drawn log-uniformly per example between min_kbps and max_kbps (kbit/s)."""

    def __init__(self, min_kbps: float = 8.0, max_kbps: float = 64.0, p: float = 0.5, sample_rate: Optional[int] = None) -> None:
        super().__init__(p=p, sample_rate=sample_rate)
        _check_range("kbps", min_kbps, max_kbps, 0.0)
        if not (min_kbps > 0.0 and math.isfinite(max_kbps)):
            raise ValueError(f"0 < min_kbps <= max_kbps < inf, got {min_kbps}, {max_kbps}")
        self.min_kbps, self.max_kbps = min_kbps, max_kbps

    def randomize_parameters(self, x, sample_rate) -> None:
        B, should = x.shape[0], self.transform_parameters["should_apply"]
        self.kbps = torch.exp(uniform(math.log(self.min_kbps), math.log(self.max_kbps), B))
        self.transform_parameters.update(kbps=self.kbps[should])

    def rates(self) -> np.ndarray:
        """(B,) float64: the last draw's bit rates in kbit/s, what ops.transform_codec is given."""
        return self.kbps.double().numpy()

    def apply_transform(self, x, sample_rate):
        return ops.transform_codec(x, self.rates(), sample_rate=sample_rate, apply=self.transform_parameters["should_apply"])


class TelephoneChannel(BaseWaveformTransform):
    """The telephone band and G.711-style companding: the 300-3400 Hz band-pass of band_filters.py (mfpa_bandpass_taps + mfpa_fir),
    then an 8-bit mu-law round trip (ops.mu_law), both gated per example.  Nothing is drawn but the gate."""
    low_hz, high_hz, channels = 300.0, 3400.0, 256

    def __init__(self, p: float = 0.5, sample_rate: Optional[int] = None) -> None:
        super().__init__(p=p, sample_rate=sample_rate)

    def cutoffs(self, sample_rate):
        """(lo, hi) as fractions of the sample rate."""
        rate = float(sample_rate)
        if not rate >= 2.0 * self.high_hz:
            raise ValueError(f"the telephone band reaches {self.high_hz} Hz: sample_rate must be at least {2.0 * self.high_hz}, got {sample_rate}")
        return self.low_hz / rate, self.high_hz / rate

    def apply_transform(self, x, sample_rate):
        B, T = x.shape
        should = self.transform_parameters["should_apply"]
        lo, hi = self.cutoffs(sample_rate)
        require_gpu(x, "samples")
        taps, off_d, ntaps_d, half_d = ops.bandpass_taps([lo] * B, [hi] * B, x.device)
        y, apply_d = torch.empty_like(x), u8(should, x.device)
        check(lib().mfpa_fir(ptr(x), B, T, T, ptr(taps), ptr(off_d), ptr(ntaps_d), ptr(half_d), ptr(apply_d), 0, 0, ptr(y), 0, stream()),
              "mfpa_fir")
        return ops.mu_law(y, self.channels, apply=should)
