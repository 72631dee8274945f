"""PitchShift (torch-audiomentations' transform of that name; the reference has none) on the device: ops.pitch_shift -- the phase
vocoder of csrc/vocoder.hip between the device STFT and its inverse, then the windowed-sinc resampler, one launch per distinct ratio.

The transpositions are small rational frequency ratios p/q, because the resampler is a polyphase filter with q phases: every
reduced p/q != 1 with q <= max_denominator inside the semitone range whose filter bank the resampler takes (q <= 1024).  With the
defaults that is 36 ratios between 4/5 (-3.86 semitones) and 5/4.  The level of an upward shift drops (the vocoder stretches it
by a rate below 1 first: DESIGN.md section 3.14)."""
from __future__ import annotations

import math
from fractions import Fraction
from typing import List, Optional

import torch

from ... import ops
from ..transform import BaseWaveformTransform


def transpositions(min_semitones: float, max_semitones: float, max_denominator: int) -> List[Fraction]:
    """Every reduced p/q != 1 with q <= max_denominator and min <= 12 log2(p/q) <= max that ops.resample_geometry(p, q) accepts,
    in ascending order."""
    lo, hi = 2.0 ** (min_semitones / 12.0), 2.0 ** (max_semitones / 12.0)
    found = set()
    for q in range(1, int(max_denominator) + 1):
        for p in range(max(1, math.floor(lo * q)), math.ceil(hi * q) + 1):
            f = Fraction(p, q)
            if f != 1 and f.denominator == q and min_semitones <= 12.0 * math.log2(p / q) <= max_semitones:
                found.add(f)
    taken = []
    for f in sorted(found):
        try:
            ops.resample_geometry(f.numerator, f.denominator)
        except ValueError:
            continue
        taken.append(f)
    return taken


class PitchShift(BaseWaveformTransform):
    def __init__(self, min_transpose_semitones: float = -4.0, max_transpose_semitones: float = 4.0, p: float = 0.5,
                 sample_rate: Optional[int] = None, max_denominator: int = 16) -> None:
        super().__init__(p=p, sample_rate=sample_rate)
        if min_transpose_semitones > max_transpose_semitones:
            raise ValueError("max_transpose_semitones must be > min_transpose_semitones")
        self.min_transpose_semitones = min_transpose_semitones
        self.max_transpose_semitones = max_transpose_semitones
        self.max_denominator = max_denominator
        self.candidates = transpositions(min_transpose_semitones, max_transpose_semitones, max_denominator)
        if not self.candidates:
            raise ValueError(f"no ratio p/q with q <= {max_denominator} lies between {min_transpose_semitones} and "
                             f"{max_transpose_semitones} semitones")

    def randomize_parameters(self, x, sample_rate) -> None:
        pick = torch.randint(0, len(self.candidates), (x.shape[0],)).tolist()
        self.ratios = [self.candidates[i] for i in pick]
        should = self.transform_parameters["should_apply"].tolist()
        self.transform_parameters["transpositions"] = [f for f, s in zip(self.ratios, should) if s]

    def apply_transform(self, x, sample_rate):
        should = self.transform_parameters["should_apply"].tolist()
        return ops.pitch_shift(x, [f if s else Fraction(1) for f, s in zip(self.ratios, should)])      # ratio 1: bit for bit
