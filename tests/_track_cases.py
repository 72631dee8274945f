"""Inputs of the whole-track tests, rebuilt from musicfpaugment_amd.synth seeds (no waveform is shipped): shared by
tools/make_track_goldens.py, which runs the reference on the three g17 inputs, and by the CPU and GPU tests."""
from __future__ import annotations

import numpy as np

from musicfpaugment_amd import synth

HOP = 256
G17_FRAMES = {"a": 2041, "b": 2041, "c": 1501}


def samples(frames: int) -> int:
    """The shortest waveform of `frames` STFT frames (1 + n // 256)."""
    return (frames - 1) * HOP


def noise(n: int, seed: int = 3) -> np.ndarray:
    return synth.noise(seed, n).astype(np.float32)


def noise_gap(n: int, seed: int = 3) -> np.ndarray:
    """The noise with a silent stretch: samples of frames [600, 1700) set to zero (cut to the clip)."""
    x = noise(n, seed)
    x[600 * HOP:1700 * HOP] = 0.0
    return x


def track_noise(n: int, seed: int = 7, noise_seed: int = 5) -> np.ndarray:
    """synth.track alone is too sparse to exercise the pruner: a noise floor under it."""
    return (synth.track(seed, n) + 0.3 * synth.noise(noise_seed, n)).astype(np.float32)


def g17_inputs():
    """{"a": noise, 2041 frames; "b": the same with the gap; "c": track + 0.3 noise, 1501 frames}."""
    na, nc = 2040 * HOP + 100, 1500 * HOP
    return {"a": noise(na), "b": noise_gap(na), "c": track_noise(nc)}
