"""Compressor, Limiter: amplitude compression, the entry of the classic fingerprint-robustness battery (Haitsma and Kalker) that a
broadcast chain or a phone's automatic gain control applies to a query.  They are not in the reference tree; the conventions are
equalizer.py's.  The gate comes first, then one draw per example for the whole batch on the host, then the parameter rows in float64
(functional.compressor_params) and ONE mfpa_dynamics launch with per-row parameters and the gate as `apply` (csrc/dynamics.hip)."""
from __future__ import annotations

from typing import Optional

import numpy as np

from ... import ops
from ...functional import compressor_params
from ..transform import BaseWaveformTransform
from . import uniform


def _check_range(name: str, lo: float, hi: float, floor: Optional[float] = None) -> None:
    if hi < lo:
        raise ValueError(f"max_{name} ({hi}) should be larger than min_{name} ({lo}).")
    if floor is not None and lo < floor:
        raise ValueError(f"min_{name} must be at least {floor}, got {lo}")


class Compressor(BaseWaveformTransform):
    """Threshold, ratio, attack and release uniform per example; the knee and the make-up gain are fixed."""

    def __init__(self, min_threshold_db: float = -30.0, max_threshold_db: float = -10.0, min_ratio: float = 2.0, max_ratio: float = 10.0,
                 min_attack_ms: float = 1.0, max_attack_ms: float = 20.0, min_release_ms: float = 50.0, max_release_ms: float = 300.0,
                 knee_db: float = 6.0, makeup_db: float = 0.0, p: float = 0.5, sample_rate: Optional[int] = None) -> None:
        super().__init__(p=p, sample_rate=sample_rate)
        _check_range("threshold_db", min_threshold_db, max_threshold_db)
        _check_range("ratio", min_ratio, max_ratio, 1.0)
        _check_range("attack_ms", min_attack_ms, max_attack_ms, 0.0)
        _check_range("release_ms", min_release_ms, max_release_ms, 0.0)
        if not knee_db >= 0.0:
            raise ValueError(f"knee_db must not be negative, got {knee_db}")
        self.min_threshold_db, self.max_threshold_db = min_threshold_db, max_threshold_db
        self.min_ratio, self.max_ratio = min_ratio, max_ratio
        self.min_attack_ms, self.max_attack_ms = min_attack_ms, max_attack_ms
        self.min_release_ms, self.max_release_ms = min_release_ms, max_release_ms
        self.knee_db, self.makeup_db = knee_db, makeup_db

    def randomize_parameters(self, x, sample_rate) -> None:
        B, should = x.shape[0], self.transform_parameters["should_apply"]
        self.threshold_db = uniform(self.min_threshold_db, self.max_threshold_db, B)
        self.ratio = uniform(self.min_ratio, self.max_ratio, B)
        self.attack_ms = uniform(self.min_attack_ms, self.max_attack_ms, B)
        self.release_ms = uniform(self.min_release_ms, self.max_release_ms, B)
        self.transform_parameters.update(threshold_db=self.threshold_db[should], ratio=self.ratio[should],
                                         attack_ms=self.attack_ms[should], release_ms=self.release_ms[should])

    def row_params(self, sample_rate) -> np.ndarray:
        """(B, 6): what the last draw gives ops.compressor, one row per example (the gate decides which rows are used)."""
        return compressor_params(sample_rate, self.threshold_db, self.ratio, self.attack_ms, self.release_ms, self.knee_db, self.makeup_db)

    def apply_transform(self, x, sample_rate):
        return ops.compressor(x, self.row_params(sample_rate), apply=self.transform_parameters["should_apply"])


class Limiter(BaseWaveformTransform):
    """Threshold and release uniform per example; ratio infinity, no knee, no attack time: no sample leaves above the threshold."""

    def __init__(self, min_threshold_db: float = -12.0, max_threshold_db: float = -1.0, min_release_ms: float = 20.0,
                 max_release_ms: float = 200.0, p: float = 0.5, sample_rate: Optional[int] = None) -> None:
        super().__init__(p=p, sample_rate=sample_rate)
        _check_range("threshold_db", min_threshold_db, max_threshold_db)
        _check_range("release_ms", min_release_ms, max_release_ms, 0.0)
        self.min_threshold_db, self.max_threshold_db = min_threshold_db, max_threshold_db
        self.min_release_ms, self.max_release_ms = min_release_ms, max_release_ms

    def randomize_parameters(self, x, sample_rate) -> None:
        B, should = x.shape[0], self.transform_parameters["should_apply"]
        self.threshold_db = uniform(self.min_threshold_db, self.max_threshold_db, B)
        self.release_ms = uniform(self.min_release_ms, self.max_release_ms, B)
        self.transform_parameters.update(threshold_db=self.threshold_db[should], release_ms=self.release_ms[should])

    def row_params(self, sample_rate) -> np.ndarray:
        return compressor_params(sample_rate, self.threshold_db, float("inf"), 0.0, self.release_ms, 0.0, 0.0)

    def apply_transform(self, x, sample_rate):
        return ops.compressor(x, self.row_params(sample_rate), apply=self.transform_parameters["should_apply"])
