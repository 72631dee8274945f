"""Substitutes for the torchaudio.transforms classes the reference uses around its pipelines.

`Resample(orig_freq, new_freq)` stands for torchaudio.transforms.Resample with its defaults (sinc_interp_hann,
lowpass_filter_width 6, rolloff 0.99) as the reference calls it at afp/audfprint/peak_extractor.py:378-388,
afp/dejavu/dejavu.py:91-115, testing/generate_queries.py:39, training/background_noise.py:300 and
training/generate_audios.py:51.  The filter is restated from torchaudio's public source (torchaudio is not in the reference
tree): parity with torchaudio itself is unpinned.  The arithmetic runs in csrc/resample.hip; there is no CPU fallback.
"""
from __future__ import annotations

import torch

from . import ops
from ._lib import MfpaError


class Resample:
    def __init__(self, orig_freq: int = 16000, new_freq: int = 16000) -> None:
        if int(orig_freq) != orig_freq or int(new_freq) != new_freq:
            raise ValueError("Frequencies must be of integer type to ensure quality resampling computation.")
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        ops.resample_geometry(self.orig_freq, self.new_freq)           # refuses a pair the kernel does not take, at construction

    def forward(self, waveform: torch.Tensor) -> torch.Tensor:
        """(..., T) float32 on any device -> (..., ceil(T * new_freq / orig_freq)) on the same device; computed on the GPU."""
        if not isinstance(waveform, torch.Tensor) or waveform.dtype != torch.float32 or waveform.dim() < 1:
            raise ValueError("waveform must be a float32 tensor (..., T)")
        if self.orig_freq == self.new_freq:
            return waveform
        x = waveform
        if not x.is_cuda:
            if not torch.cuda.is_available():
                raise MfpaError("Resample computes on the MI355X and none is present; no CPU fallback")
            x = x.cuda()
        lead = x.shape[:-1]
        with torch.cuda.device(x.device):
            y = ops.resample(x.reshape(-1, x.shape[-1]), self.orig_freq, self.new_freq)
        return y.reshape(*lead, y.shape[-1]).to(waveform.device)

    __call__ = forward
