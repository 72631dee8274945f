"""BaseWaveformTransform on MI355X -- the reference's augmentation/transform.py surface over the kernels of csrc/augment.hip and
csrc/transforms.hip.

A transform is called as `t(samples (B, 1, T) on the GPU, sample_rate=None)` and returns `ObjectDict(samples, sample_rate)`.
`p` is the per-example Bernoulli gate, `transform_parameters` holds the last call's draws under the reference's key names
(`should_apply` plus the transform's own, restricted to the examples the gate selected).

Differences from the reference, on purpose and the same as AugmentFP's (augmentation/__init__.py):
  * the draw convention is AugmentFP's: a transform draws its gate and then its parameters for the WHOLE batch on the host, every
    call, whether or not an example is selected; only the per-sample arithmetic (one kernel launch for the batch) depends on the
    gate.  A Compose of the eight AugmentFP stages therefore consumes `random` and `torch`'s generator exactly like AugmentFP;
  * mono only: the device chain is (B, T), and C > 1 raises MultichannelAudioNotSupportedException;
  * there is no CPU fallback: the samples must already be on the GPU.
"""
from __future__ import annotations

import random
import warnings
from typing import Any, Dict, Optional

import torch
from torch.distributions import Bernoulli

from .._lib import require_gpu


class MultichannelAudioNotSupportedException(Exception):
    pass


class EmptyPathException(Exception):
    pass


class ModeNotSupportedException(Exception):
    pass


class ObjectDict(dict):
    """A dict whose items are attributes too: `out.samples`, `out["samples"]`, `transform(**out)`."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError as e:
            raise AttributeError(name) from e

    def __setattr__(self, name, value):
        self[name] = value

    def __delattr__(self, name):
        try:
            del self[name]
        except KeyError as e:
            raise AttributeError(name) from e


class BaseWaveformTransform(torch.nn.Module):
    supports_multichannel = False
    requires_sample_rate = True

    def __init__(self, p: float = 0.5, sample_rate: Optional[int] = None):
        super().__init__()
        assert 0.0 <= p <= 1.0
        self._p = p
        self.sample_rate = sample_rate
        self.transform_parameters: Dict[Any, Any] = {}
        self.are_parameters_frozen = False
        self.bernoulli_distribution = Bernoulli(self._p)

    @property
    def p(self) -> float:
        return self._p

    @p.setter
    def p(self, p: float) -> None:
        self._p = p
        self.bernoulli_distribution = Bernoulli(self._p)

    @torch.no_grad()
    def forward(self, samples: torch.Tensor, sample_rate: Optional[int] = None) -> ObjectDict:
        if not isinstance(samples, torch.Tensor) or samples.dim() != 3:
            raise RuntimeError(
                "torch-audiomentations expects three-dimensional input tensors, with"
                " dimension ordering like [batch_size, num_channels, num_samples]. If your"
                " audio is mono, you can use a shape like [batch_size, 1, num_samples].")
        sample_rate = sample_rate or self.sample_rate
        B, C, T = samples.shape
        if B * C * T == 0:
            warnings.warn("An empty samples tensor was passed to {}".format(self.__class__.__name__))
            return ObjectDict(samples=samples, sample_rate=sample_rate)
        if C > 1 and not self.supports_multichannel:
            raise MultichannelAudioNotSupportedException(
                "{} only supports mono audio, not multichannel audio".format(self.__class__.__name__))
        if self.requires_sample_rate and sample_rate is None:
            raise RuntimeError("sample_rate is required")
        require_gpu(samples, "samples")
        x = samples[:, 0].to(torch.float32).contiguous()
        self.transform_parameters = {"should_apply": self.bernoulli_distribution.sample((B,)).to(torch.bool)}
        self.randomize_parameters(x, sample_rate)
        y = self.apply_transform(x, sample_rate)
        return ObjectDict(samples=y.unsqueeze(1), sample_rate=sample_rate)

    def randomize_parameters(self, x: torch.Tensor, sample_rate: Optional[int]) -> None:
        """Draw this call's parameters for all B examples of x (B, T), on the host."""

    def apply_transform(self, x: torch.Tensor, sample_rate: Optional[int]) -> torch.Tensor:
        """(B, T) float32 on the GPU -> (B, T): one launch for the batch, examples with should_apply False copied through."""
        raise NotImplementedError()

    def freeze_parameters(self, seed: int = 0) -> None:
        """Like the reference's: reseeds `random` and torch, nothing else -- the next call then draws what the last frozen call drew."""
        self.are_parameters_frozen = True
        random.seed(seed)
        torch.manual_seed(seed)

    def unfreeze_parameters(self) -> None:
        self.are_parameters_frozen = False
