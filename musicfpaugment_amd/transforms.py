"""Substitutes for the torchaudio.transforms classes the reference uses around its pipelines.

`Resample(orig_freq, new_freq)` stands for torchaudio.transforms.Resample with its defaults (sinc_interp_hann,
lowpass_filter_width 6, rolloff 0.99) as the reference calls it at afp/audfprint/peak_extractor.py:378-388,
afp/dejavu/dejavu.py:91-115, testing/generate_queries.py:39, training/background_noise.py:300 and
training/generate_audios.py:51.  The filter is restated from torchaudio's public source (torchaudio is not in the reference
tree): parity with torchaudio itself is unpinned.  The arithmetic runs in csrc/resample.hip; there is no CPU fallback.
The dense kernel there holds at most 1024 phases of 8192 taps; `any_ratio=True` (Resample, Speed, PitchShift) sends a pair of rates
beyond that to the sparse-tap kernel, which walks only the taps that are not zero and takes every pair of rates below 65536 Hz.

`TimeStretch`, `Speed` and `PitchShift` stand for the torchaudio.transforms classes of those names (the reference uses none of
them: they are the tempo and pitch distortions fingerprinting papers test first).  The phase vocoder is restated from torchaudio's
public source too and runs in csrc/vocoder.hip; `Speed` is one resampling.
"""
from __future__ import annotations

import math
from fractions import Fraction
from typing import Optional

import torch

from . import ops
from ._lib import MfpaError


class Resample:
    def __init__(self, orig_freq: int = 16000, new_freq: int = 16000, *, any_ratio: bool = False) -> None:
        if int(orig_freq) != orig_freq or int(new_freq) != new_freq:
            raise ValueError("Frequencies must be of integer type to ensure quality resampling computation.")
        self.orig_freq, self.new_freq, self.any_ratio = int(orig_freq), int(new_freq), bool(any_ratio)
        ops.resample_kernel_for(self.orig_freq, self.new_freq, self.any_ratio)    # refuses a pair no kernel takes, at construction

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
            y = ops.resample(x.reshape(-1, x.shape[-1]), self.orig_freq, self.new_freq, any_ratio=self.any_ratio)
        return y.reshape(*lead, y.shape[-1]).to(waveform.device)

    __call__ = forward


def _on_gpu(x: torch.Tensor, who: str) -> torch.Tensor:
    if x.is_cuda:
        return x
    if not torch.cuda.is_available():
        raise MfpaError(f"{who} computes on the MI355X and none is present; no CPU fallback")
    return x.cuda()


class TimeStretch:
    """torchaudio.transforms.TimeStretch at the library's geometry: n_freq 257 (n_fft 512), hop 256 -- anything else is a
    NotImplementedError.  The phase vocoder runs in csrc/vocoder.hip (ops.phase_vocoder), float64; a complex64 input is computed in
    complex128 and returned as complex64."""

    def __init__(self, hop_length: Optional[int] = None, n_freq: int = 257, fixed_rate: Optional[float] = None) -> None:
        n_fft = (n_freq - 1) * 2
        hop_length = hop_length if hop_length is not None else n_fft // 2
        if n_freq != ops.N_BINS or hop_length != ops.N_HOP:
            raise NotImplementedError(f"TimeStretch is built for n_freq 257 and hop_length 256, not ({n_freq}, {hop_length})")
        self.hop_length, self.n_freq, self.fixed_rate = hop_length, n_freq, fixed_rate

    def forward(self, complex_specgrams: torch.Tensor, overriding_rate: Optional[float] = None) -> torch.Tensor:
        """(..., 257, n_frames) complex -> (..., 257, ceil(n_frames / rate)) on the same device."""
        if not isinstance(complex_specgrams, torch.Tensor) or not torch.is_complex(complex_specgrams):
            raise ValueError("The input to TimeStretch must be complex type.")
        if overriding_rate is None:
            if self.fixed_rate is None:
                raise ValueError("If no fixed_rate is specified, must pass a valid rate to the forward method.")
            rate = self.fixed_rate
        else:
            rate = overriding_rate
        if complex_specgrams.dim() < 2 or complex_specgrams.shape[-2] != self.n_freq:
            raise ValueError(f"complex_specgrams must be (..., {self.n_freq}, n_frames)")
        if rate == 1.0:
            return complex_specgrams
        x = _on_gpu(complex_specgrams, "TimeStretch")
        lead = x.shape[:-2]
        with torch.cuda.device(x.device):
            y, _ = ops.phase_vocoder(x.reshape(-1, *x.shape[-2:]).to(torch.complex128), float(rate))
        return y.reshape(*lead, *y.shape[-2:]).to(device=complex_specgrams.device, dtype=complex_specgrams.dtype)

    __call__ = forward


class Speed:
    """torchaudio.transforms.Speed: play `factor` times faster by ONE resampling from int(factor * orig_freq) to orig_freq (reduced by
    their gcd); pitch and tempo move together.  -> (waveform, lengths).  any_ratio=True: as for Resample (a factor like 1.0123 at
    8 kHz reduces to 4049 : 4000, which only the sparse-tap kernel takes)."""

    def __init__(self, orig_freq: int, factor: float, *, any_ratio: bool = False) -> None:
        self.orig_freq, self.factor = orig_freq, factor
        self.source_sample_rate = int(factor * orig_freq)
        self.target_sample_rate = int(orig_freq)
        if self.source_sample_rate <= 0 or self.target_sample_rate <= 0:
            raise ValueError("Original frequency and desired frequecy should be positive")
        gcd = math.gcd(self.source_sample_rate, self.target_sample_rate)
        self.resampler = Resample(self.source_sample_rate // gcd, self.target_sample_rate // gcd, any_ratio=any_ratio)

    def forward(self, waveform: torch.Tensor, lengths: Optional[torch.Tensor] = None):
        out_lengths = None
        if lengths is not None:
            out_lengths = torch.ceil(lengths * self.target_sample_rate / self.source_sample_rate).to(lengths.dtype)
        return self.resampler(waveform), out_lengths

    __call__ = forward


class PitchShift:
    """torchaudio.transforms.PitchShift's arithmetic on the library's STFT (512 / 256; torchaudio's default hop is 128): stretch by
    rate = 2^(-n_steps / bins_per_octave) with the phase vocoder, resample from int(sample_rate / rate) to sample_rate, crop or
    zero-pad to the input's length.

    The pair int(sample_rate / rate) : sample_rate, reduced by its gcd, is checked at construction like Resample's.  The dense
    resampling kernel holds at most 1024 phases, and most semitone counts at 8 kHz reduce to more: 12 steps (16000 : 8000 = 2 : 1)
    and -1 (7550 : 8000 = 151 : 160) fit, 2 steps (8979 : 8000) do not.  any_ratio=True sends such a pair to the sparse-tap kernel:
    PitchShift(8000, n_steps, any_ratio=True) takes every semitone count.  The pitch moves by `ratio` (the integer pair), not by
    2^(n_steps / bins_per_octave) exactly -- torchaudio's own rounding."""

    def __init__(self, sample_rate: int, n_steps: int, bins_per_octave: int = 12, *, any_ratio: bool = False) -> None:
        self.sample_rate, self.n_steps, self.bins_per_octave = int(sample_rate), n_steps, bins_per_octave
        self.any_ratio = bool(any_ratio)
        self.rate = 2.0 ** (-float(n_steps) / bins_per_octave)
        orig_freq = int(self.sample_rate / self.rate)
        if orig_freq <= 0 or self.sample_rate <= 0:
            raise ValueError("Original frequency and desired frequecy should be positive")
        self.ratio = Fraction(orig_freq, self.sample_rate)
        if self.ratio != 1:
            ops.resample_kernel_for(self.ratio.numerator, self.ratio.denominator, self.any_ratio)     # refused at construction, like Resample

    def forward(self, waveform: torch.Tensor) -> torch.Tensor:
        """(..., T) float32 on any device -> the same shape on the same device; computed on the GPU."""
        if not isinstance(waveform, torch.Tensor) or waveform.dtype != torch.float32 or waveform.dim() < 1:
            raise ValueError("waveform must be a float32 tensor (..., T)")
        x = _on_gpu(waveform, "PitchShift")
        with torch.cuda.device(x.device):
            y = ops.pitch_shift(x.reshape(-1, x.shape[-1]), self.ratio, rates=self.rate, any_ratio=self.any_ratio)
        return y.reshape(waveform.shape).to(waveform.device)

    __call__ = forward
