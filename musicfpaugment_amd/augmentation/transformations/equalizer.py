"""PeakingFilter, LowShelfFilter, HighShelfFilter, ParametricEQ: the equaliser distortions, named after audiomentations' (they are
not in the reference tree) with defaults that sit under an 8 kHz clip's Nyquist frequency.  The gate comes first, then one draw per
example for the whole batch on the host, then the cookbook designs per example in float64 (functional.biquad_coefficients) and ONE
mfpa_sosfilt launch with per-row sections and the gate as `apply` (csrc/iir.hip)."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ... import ops
from ...functional import biquad_coefficients
from ..transform import BaseWaveformTransform
from . import mel_uniform, uniform

IDENTITY_SECTION = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)


def _check_range(name: str, lo: float, hi: float, floor: Optional[float] = None) -> None:
    if hi < lo:
        raise ValueError(f"max_{name} ({hi}) should be larger than min_{name} ({lo}).")
    if floor is not None and lo <= floor:
        raise ValueError(f"min_{name} must be larger than {floor}, got {lo}")


class _ShapedFilter(BaseWaveformTransform):
    """One cookbook biquad of `kind` per example: centre uniform in mel, gain uniform in dB, Q uniform."""
    kind = None

    def __init__(self, min_center_freq: float, max_center_freq: float, min_gain_db: float, max_gain_db: float, min_q: float, max_q: float,
                 p: float = 0.5, sample_rate: Optional[int] = None) -> None:
        super().__init__(p=p, sample_rate=sample_rate)
        _check_range("center_freq", min_center_freq, max_center_freq, 0.0)
        _check_range("gain_db", min_gain_db, max_gain_db)
        _check_range("q", min_q, max_q, 0.0)
        self.min_center_freq, self.max_center_freq = min_center_freq, max_center_freq
        self.min_gain_db, self.max_gain_db = min_gain_db, max_gain_db
        self.min_q, self.max_q = min_q, max_q

    def randomize_parameters(self, x, sample_rate) -> None:
        B, should = x.shape[0], self.transform_parameters["should_apply"]
        if self.max_center_freq >= sample_rate / 2:
            raise ValueError(f"max_center_freq ({self.max_center_freq} Hz) is not below the Nyquist frequency {sample_rate / 2} Hz")
        self.center_freq = mel_uniform(self.min_center_freq, self.max_center_freq, B, integer_bounds=False)
        self.gain_db = uniform(self.min_gain_db, self.max_gain_db, B)
        self.q = uniform(self.min_q, self.max_q, B)
        self.transform_parameters.update(center_freq=self.center_freq[should], gain_db=self.gain_db[should], q=self.q[should])

    def apply_transform(self, x, sample_rate):
        should = self.transform_parameters["should_apply"]
        sos = np.tile(np.array(IDENTITY_SECTION), (x.shape[0], 1, 1))          # an example the gate skips gets the identity
        for b, (f, g, q) in enumerate(zip(self.center_freq.tolist(), self.gain_db.tolist(), self.q.tolist())):
            if should[b]:
                sos[b, 0] = biquad_coefficients(self.kind, sample_rate, f, q, g)
        return ops.sosfilt(x, sos, apply=should)


class PeakingFilter(_ShapedFilter):
    """Boost or cut a band around a centre frequency."""
    kind = "peaking"

    def __init__(self, min_center_freq: float = 50.0, max_center_freq: float = 3800.0, min_gain_db: float = -24.0,
                 max_gain_db: float = 24.0, min_q: float = 0.5, max_q: float = 5.0, p: float = 0.5,
                 sample_rate: Optional[int] = None) -> None:
        super().__init__(min_center_freq, max_center_freq, min_gain_db, max_gain_db, min_q, max_q, p, sample_rate)


class LowShelfFilter(_ShapedFilter):
    """Boost or cut everything below a centre frequency."""
    kind = "lowshelf"

    def __init__(self, min_center_freq: float = 50.0, max_center_freq: float = 2000.0, min_gain_db: float = -18.0,
                 max_gain_db: float = 18.0, min_q: float = 0.1, max_q: float = 0.999, p: float = 0.5,
                 sample_rate: Optional[int] = None) -> None:
        super().__init__(min_center_freq, max_center_freq, min_gain_db, max_gain_db, min_q, max_q, p, sample_rate)


class HighShelfFilter(_ShapedFilter):
    """Boost or cut everything above a centre frequency."""
    kind = "highshelf"

    def __init__(self, min_center_freq: float = 300.0, max_center_freq: float = 3800.0, min_gain_db: float = -18.0,
                 max_gain_db: float = 18.0, min_q: float = 0.1, max_q: float = 0.999, p: float = 0.5,
                 sample_rate: Optional[int] = None) -> None:
        super().__init__(min_center_freq, max_center_freq, min_gain_db, max_gain_db, min_q, max_q, p, sample_rate)


class ParametricEQ(BaseWaveformTransform):
    """n_bands fixed bands, centres geomspace(min_freq, max_freq_fraction * sample_rate, n_bands): a low shelf (Q 0.707), peaking
    bands (Q 1.0) and a high shelf (Q 0.707), one gain drawn per band and example; one launch with S = n_bands sections."""
    SHELF_Q, PEAK_Q = 0.707, 1.0

    def __init__(self, n_bands: int = 7, min_gain_db: float = -12.0, max_gain_db: float = 12.0, min_freq: float = 60.0,
                 max_freq_fraction: float = 0.4, p: float = 0.5, sample_rate: Optional[int] = None) -> None:
        super().__init__(p=p, sample_rate=sample_rate)
        if int(n_bands) != n_bands or not 2 <= n_bands <= ops.SOS_MAX_SECTIONS:
            raise ValueError(f"n_bands must be an integer from 2 to {ops.SOS_MAX_SECTIONS}, got {n_bands}")
        _check_range("gain_db", min_gain_db, max_gain_db)
        if not min_freq > 0.0:
            raise ValueError(f"min_freq must be positive, got {min_freq}")
        if not 0.0 < max_freq_fraction < 0.5:
            raise ValueError(f"max_freq_fraction must lie in (0, 0.5), got {max_freq_fraction}")
        self.n_bands, self.min_gain_db, self.max_gain_db = int(n_bands), min_gain_db, max_gain_db
        self.min_freq, self.max_freq_fraction = min_freq, max_freq_fraction

    def band_centers(self, sample_rate) -> np.ndarray:
        top = self.max_freq_fraction * sample_rate
        if not self.min_freq < top:
            raise ValueError(f"min_freq ({self.min_freq}) must be below max_freq_fraction * sample_rate ({top})")
        return np.geomspace(self.min_freq, top, self.n_bands)

    def band_sections(self, sample_rate, gains_db) -> np.ndarray:
        """(n_bands, 6): the sections of one example from its n_bands gains."""
        centers, last = self.band_centers(sample_rate), self.n_bands - 1
        return np.stack([biquad_coefficients("lowshelf" if i == 0 else "highshelf" if i == last else "peaking", sample_rate, centers[i],
                                             self.SHELF_Q if i in (0, last) else self.PEAK_Q, g) for i, g in enumerate(gains_db)])

    def randomize_parameters(self, x, sample_rate) -> None:
        B, should = x.shape[0], self.transform_parameters["should_apply"]
        self.gains_db = uniform(self.min_gain_db, self.max_gain_db, B * self.n_bands).reshape(B, self.n_bands)
        self.transform_parameters.update(gains_db=self.gains_db[should])

    def apply_transform(self, x, sample_rate):
        should = self.transform_parameters["should_apply"]
        self.band_centers(sample_rate)
        sos = np.tile(np.array(IDENTITY_SECTION), (x.shape[0], self.n_bands, 1))
        for b, gains in enumerate(self.gains_db.tolist()):
            if should[b]:
                sos[b] = self.band_sections(sample_rate, gains)
        return ops.sosfilt(x, sos, apply=should)
