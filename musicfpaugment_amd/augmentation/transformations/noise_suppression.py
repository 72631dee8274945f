"""NoiseSuppression: what a handset's noise suppressor does to music recorded through a call -- it takes sustained notes for noise
and gouges them.  It is not in the reference tree; the conventions are codec.py's.  The gate comes first, then one draw per example
for the whole batch on the host, then one complex STFT, ONE launch of csrc/denoise.hip with the floors per row and the gate as
`apply` (ops.spectral_suppress), and the inverse STFT on the input's phase.  Examples the gate did not select come back bit for bit:
they are taken from the input, not from the transform pair."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ... import ops
from ..._lib import require_gpu
from ..transform import BaseWaveformTransform
from . import u8, uniform
from .dynamics import _check_range


class NoiseSuppression(BaseWaveformTransform):
    """The spectral suppressor with its defaults and a gain floor drawn uniformly per example between min_floor_db and max_floor_db
    (dB, not positive): the lower the floor, the deeper the suppressor may cut."""
    requires_sample_rate = False

    def __init__(self, min_floor_db: float = -30.0, max_floor_db: float = -10.0, p: float = 0.5, sample_rate: Optional[int] = None) -> None:
        super().__init__(p=p, sample_rate=sample_rate)
        _check_range("floor_db", min_floor_db, max_floor_db, -np.inf)
        if not (np.isfinite(min_floor_db) and max_floor_db <= 0.0):
            raise ValueError(f"-inf < min_floor_db <= max_floor_db <= 0, got {min_floor_db}, {max_floor_db}")
        self.min_floor_db, self.max_floor_db = min_floor_db, max_floor_db

    def randomize_parameters(self, x, sample_rate) -> None:
        B, should = x.shape[0], self.transform_parameters["should_apply"]
        self.floor_db = uniform(self.min_floor_db, self.max_floor_db, B)
        self.transform_parameters.update(floor_db=self.floor_db[should])

    def floors(self) -> np.ndarray:
        """(B,) float64: the last draw's floors in dB, what ops.spectral_suppress is given."""
        return np.minimum(self.floor_db.double().numpy(), 0.0)

    def apply_transform(self, x, sample_rate):
        require_gpu(x, "samples")
        should = self.transform_parameters["should_apply"]
        spec, mag, _ = ops.stft_complex(x, want_mag=True)
        y = ops.istft(spec, x.shape[1], mag=ops.spectral_suppress(mag, floor_db=self.floors(), apply=should))
        return torch.where(u8(should, x.device).bool()[:, None], y, x)
