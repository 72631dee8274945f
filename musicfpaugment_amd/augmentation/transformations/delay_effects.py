"""Echo, WowFlutter, Chorus: what an analogue playback chain (a turntable, a cassette, a cheap wireless link) and a reflecting room do
to a query beside equalisation and compression: a slap-back echo, slow and fast speed drift, doubled voices.  They are not in the
reference tree; the conventions are dynamics.py's.  The gate comes first, then one draw per example for the whole batch on the
host, then ONE launch of csrc/delay.hip with per-row parameters and the gate as `apply` (ops.variable_delay, or ops.comb for the
regenerating echo); the delay tensors of WowFlutter and Chorus are elementwise torch on the device (ops.speed_drift_delay,
ops.lfo_delay)."""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from ... import ops
from ..transform import BaseWaveformTransform
from . import uniform
from .dynamics import _check_range


class Echo(BaseWaveformTransform):
    """One echo per example, delay and decay uniform: x[n] + decay x(n - delay) (a fractional delay, ops.variable_delay), or with
    feedback=True the regenerating y[n] = x[n] + decay y[n - D], D the delay rounded to whole samples (ops.comb)."""

    def __init__(self, min_delay_ms: float = 50.0, max_delay_ms: float = 400.0, min_decay: float = 0.2, max_decay: float = 0.6,
                 feedback: bool = False, p: float = 0.5, sample_rate: Optional[int] = None) -> None:
        super().__init__(p=p, sample_rate=sample_rate)
        _check_range("delay_ms", min_delay_ms, max_delay_ms, 0.0)
        _check_range("decay", min_decay, max_decay, 0.0)
        if not max_decay < 1.0:
            raise ValueError(f"max_decay must be below 1, got {max_decay}")
        self.min_delay_ms, self.max_delay_ms = min_delay_ms, max_delay_ms
        self.min_decay, self.max_decay = min_decay, max_decay
        self.feedback = bool(feedback)

    def randomize_parameters(self, x, sample_rate) -> None:
        B, should = x.shape[0], self.transform_parameters["should_apply"]
        self.delay_ms = uniform(self.min_delay_ms, self.max_delay_ms, B)
        self.decay = uniform(self.min_decay, self.max_decay, B)
        self.transform_parameters.update(delay_ms=self.delay_ms[should], decay=self.decay[should])

    def delay_samples(self, sample_rate) -> np.ndarray:
        """(B,) float64: the last draw's delays in samples; whole samples, at least 1, with feedback."""
        d = self.delay_ms.double().numpy() * (float(sample_rate) / 1000.0)
        return np.maximum(np.rint(d), 1.0) if self.feedback else d

    def apply_transform(self, x, sample_rate):
        should, decay = self.transform_parameters["should_apply"], self.decay.double().numpy()
        if self.feedback:
            return ops.comb(x, self.delay_samples(sample_rate), 1.0, 0.0, decay, apply=should)
        return ops.variable_delay(x, self.delay_samples(sample_rate)[:, None, None], decay[:, None], dry=1.0, apply=should)


class WowFlutter(BaseWaveformTransform):
    """Speed drift: the relative speed 1 + wow_depth sin(2 pi wow_hz t + phase) + flutter_depth sin(2 pi flutter_hz t + phase'),
    frequencies, depths and both phases uniform per example."""

    def __init__(self, min_wow_hz: float = 0.3, max_wow_hz: float = 2.0, min_wow_depth: float = 0.0005, max_wow_depth: float = 0.004,
                 min_flutter_hz: float = 5.0, max_flutter_hz: float = 12.0, min_flutter_depth: float = 0.0002,
                 max_flutter_depth: float = 0.0015, p: float = 0.5, sample_rate: Optional[int] = None) -> None:
        super().__init__(p=p, sample_rate=sample_rate)
        _check_range("wow_hz", min_wow_hz, max_wow_hz, 0.0)
        _check_range("wow_depth", min_wow_depth, max_wow_depth, 0.0)
        _check_range("flutter_hz", min_flutter_hz, max_flutter_hz, 0.0)
        _check_range("flutter_depth", min_flutter_depth, max_flutter_depth, 0.0)
        if not max_wow_depth + max_flutter_depth < 1.0:
            raise ValueError("the depths are relative speed deviations and must sum to less than 1")
        self.min_wow_hz, self.max_wow_hz = min_wow_hz, max_wow_hz
        self.min_wow_depth, self.max_wow_depth = min_wow_depth, max_wow_depth
        self.min_flutter_hz, self.max_flutter_hz = min_flutter_hz, max_flutter_hz
        self.min_flutter_depth, self.max_flutter_depth = min_flutter_depth, max_flutter_depth

    def randomize_parameters(self, x, sample_rate) -> None:
        B, should = x.shape[0], self.transform_parameters["should_apply"]
        self.wow_hz = uniform(self.min_wow_hz, self.max_wow_hz, B)
        self.wow_depth = uniform(self.min_wow_depth, self.max_wow_depth, B)
        self.flutter_hz = uniform(self.min_flutter_hz, self.max_flutter_hz, B)
        self.flutter_depth = uniform(self.min_flutter_depth, self.max_flutter_depth, B)
        self.wow_phase = uniform(0.0, 2.0 * math.pi, B)
        self.flutter_phase = uniform(0.0, 2.0 * math.pi, B)
        self.transform_parameters.update(wow_hz=self.wow_hz[should], wow_depth=self.wow_depth[should], flutter_hz=self.flutter_hz[should],
                                         flutter_depth=self.flutter_depth[should], wow_phase=self.wow_phase[should],
                                         flutter_phase=self.flutter_phase[should])

    def components(self):
        """What the last draw gives ops.speed_drift_delay."""
        return [(self.wow_depth.double(), self.wow_hz.double(), self.wow_phase.double()),
                (self.flutter_depth.double(), self.flutter_hz.double(), self.flutter_phase.double())]

    def apply_transform(self, x, sample_rate):
        delay = ops.speed_drift_delay(x.shape[0], x.shape[1], sample_rate, self.components(), device=x.device)
        return ops.variable_delay(x, delay, apply=self.transform_parameters["should_apply"])


class Chorus(BaseWaveformTransform):
    """(1 - mix) x + mix / voices * sum of `voices` copies read at base_ms + depth_ms sin(2 pi rate_hz t + phase_v), the phases spread
    evenly; the number of voices, the depth and the rate uniform per example.  The launch has max_voices voices; an example that
    drew fewer has the others at an infinite delay and gain 0: such a voice adds gain * 0 = 0, and the kernel runs no taps for it
    in a tile where none of its lanes is live, which is every tile of that example."""

    def __init__(self, min_voices: int = 2, max_voices: int = 4, min_depth_ms: float = 1.0, max_depth_ms: float = 4.0,
                 min_rate_hz: float = 0.3, max_rate_hz: float = 2.0, mix: float = 0.5, p: float = 0.5, sample_rate: Optional[int] = None,
                 base_ms: float = 20.0) -> None:
        super().__init__(p=p, sample_rate=sample_rate)
        if int(min_voices) != min_voices or int(max_voices) != max_voices or not 1 <= min_voices <= max_voices <= ops.DELAY_MAX_VOICES:
            raise ValueError(f"1 <= min_voices <= max_voices <= {ops.DELAY_MAX_VOICES} (integers), got {min_voices}, {max_voices}")
        _check_range("depth_ms", min_depth_ms, max_depth_ms, 0.0)
        _check_range("rate_hz", min_rate_hz, max_rate_hz, 0.0)
        if not 0.0 <= mix <= 1.0:
            raise ValueError(f"mix must lie in [0, 1], got {mix}")
        if not base_ms >= max_depth_ms:
            raise ValueError(f"base_ms ({base_ms}) must not be below max_depth_ms ({max_depth_ms}): the delay would turn negative")
        self.min_voices, self.max_voices = int(min_voices), int(max_voices)
        self.min_depth_ms, self.max_depth_ms = min_depth_ms, max_depth_ms
        self.min_rate_hz, self.max_rate_hz = min_rate_hz, max_rate_hz
        self.mix, self.base_ms = float(mix), float(base_ms)

    def randomize_parameters(self, x, sample_rate) -> None:
        B, should = x.shape[0], self.transform_parameters["should_apply"]
        self.voices = torch.randint(self.min_voices, self.max_voices + 1, (B,))
        self.depth_ms = uniform(self.min_depth_ms, self.max_depth_ms, B)
        self.rate_hz = uniform(self.min_rate_hz, self.max_rate_hz, B)
        self.transform_parameters.update(voices=self.voices[should], depth_ms=self.depth_ms[should], rate_hz=self.rate_hz[should])

    def voice_gains(self) -> np.ndarray:
        """(B, max_voices) float64: mix / voices for an example's own voices, 0 for the others."""
        n = self.voices.numpy()[:, None]
        return np.where(np.arange(self.max_voices)[None, :] < n, self.mix / n, 0.0)

    def delays(self, T: int, sample_rate, device) -> torch.Tensor:
        """(B, max_voices, T) float64 on the device: the last draw's delays in samples, +inf for a voice an example did not draw.
        One ops.lfo_delay over the B * max_voices oscillators and one torch.where: no synchronisation."""
        B, V = self.voices.shape[0], self.max_voices
        drawn = np.arange(V)[None, :] < self.voices.numpy()[:, None]                                   # (B, V) on the host
        phase = 2.0 * math.pi * np.arange(V)[None, :] / self.voices.double().numpy()[:, None]
        per_voice = lambda t: np.repeat(t.double().numpy(), V)                                         # noqa: E731
        d = ops.lfo_delay(B * V, T, sample_rate, base_ms=self.base_ms, depth_ms=per_voice(self.depth_ms), rate_hz=per_voice(self.rate_hz),
                          phase=phase.reshape(-1), device=device).reshape(B, V, T)
        return torch.where(ops._upload(torch.from_numpy(drawn), d.device)[:, :, None], d, float("inf"))

    def apply_transform(self, x, sample_rate):
        should = self.transform_parameters["should_apply"]
        if not bool(should.any()):                                                                     # the gate is on the host: nothing to build
            return x.clone()
        return ops.variable_delay(x, self.delays(x.shape[1], sample_rate, x.device), self.voice_gains(), dry=1.0 - self.mix, apply=should)
