"""LoudnessNormalization: bring an example to a programme loudness (ITU-R BS.1770 / EBU R 128) drawn per example, what a broadcast
chain, a streaming service or a phone does to a query.  The name and the defaults are audiomentations'; it is not in the reference
tree, and the conventions are dynamics.py's.  The gate comes first, then one target per example for the whole batch on the host, then
the meter, the gain and the multiply on the device without a host synchronisation (ops.loudness_normalize, csrc/loudness.hip), the gate
as `apply`: an unselected example comes back bit for bit, and so does digital silence."""
from __future__ import annotations

from typing import Optional

import numpy as np

from ... import ops
from ..transform import BaseWaveformTransform
from . import uniform


class LoudnessNormalization(BaseWaveformTransform):
    """The target loudness in LUFS uniform per example."""

    def __init__(self, min_lufs: float = -31.0, max_lufs: float = -13.0, p: float = 0.5, sample_rate: Optional[int] = None) -> None:
        super().__init__(p=p, sample_rate=sample_rate)
        if not (np.isfinite(min_lufs) and np.isfinite(max_lufs)):
            raise ValueError(f"min_lufs and max_lufs must be finite, got {min_lufs} and {max_lufs}")
        if max_lufs < min_lufs:
            raise ValueError(f"max_lufs ({max_lufs}) should be larger than min_lufs ({min_lufs}).")
        self.min_lufs, self.max_lufs = min_lufs, max_lufs

    def randomize_parameters(self, x, sample_rate) -> None:
        B, should = x.shape[0], self.transform_parameters["should_apply"]
        self.lufs = uniform(self.min_lufs, self.max_lufs, B)
        self.transform_parameters.update(lufs=self.lufs[should])

    def targets(self) -> np.ndarray:
        """(B,) float64: what the last draw gives ops.loudness_normalize, one target per example (the gate decides which are used)."""
        return self.lufs.numpy().astype(np.float64)

    def apply_transform(self, x, sample_rate):
        return ops.loudness_normalize(x, sample_rate, self.targets(), apply=self.transform_parameters["should_apply"])
