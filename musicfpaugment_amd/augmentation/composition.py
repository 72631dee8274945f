"""Compose, SomeOf, OneOf -- the reference's augmentation/composition.py surface over the device transforms.

Each is called like a transform, `c(samples (B, 1, T), sample_rate=None) -> ObjectDict(samples, sample_rate)`, and hands the
ObjectDict from member to member; the tensors never leave the GPU.  The host-side choices are the reference's:
  Compose   applies every member in order, or in `random.shuffle` order with shuffle=True.  Like the reference's, it stores `p`
            and does not gate on it (its forward never reads it) -- so a Compose consumes no random number of its own;
  SomeOf    `random.random() < p`, then `random.randint(min, max)` members chosen by `random.sample`, applied in index order;
  OneOf     SomeOf(1, ...).
Members that are neither a BaseWaveformTransform nor a BaseCompose are skipped, as in the reference.
"""
from __future__ import annotations

import random
from typing import List, Optional, Tuple, Union

import torch

from .transform import BaseWaveformTransform, ObjectDict


class BaseCompose(torch.nn.Module):
    def __init__(self, transforms: List[torch.nn.Module], shuffle: bool = False, p: float = 1.0):
        super().__init__()
        self.p = p
        self.shuffle = shuffle
        self.are_parameters_frozen = False
        self.transforms = torch.nn.ModuleList(transforms)

    def freeze_parameters(self, seed: int = 0) -> None:
        self.are_parameters_frozen = True
        for t in self.transforms:
            t.freeze_parameters(seed)

    def unfreeze_parameters(self) -> None:
        self.are_parameters_frozen = False
        for t in self.transforms:
            t.unfreeze_parameters()

    def _run(self, inputs: ObjectDict, indexes) -> ObjectDict:
        for i in indexes:
            t = self.transforms[i]
            if isinstance(t, (BaseWaveformTransform, BaseCompose)):
                inputs = t(**inputs)
        return inputs


class Compose(BaseCompose):
    def forward(self, samples: Optional[torch.Tensor] = None, sample_rate: Optional[int] = None) -> ObjectDict:
        indexes = list(range(len(self.transforms)))
        if self.shuffle:
            random.shuffle(indexes)
        return self._run(ObjectDict(samples=samples, sample_rate=sample_rate), indexes)


class SomeOf(BaseCompose):
    """SomeOf(2, [...]) applies exactly two members, SomeOf((1, 3), [...]) one to three, SomeOf((2, None), [...]) two to all."""

    def __init__(self, num_transforms: Union[int, Tuple[int, Optional[int]]], transforms: List[torch.nn.Module], p: float = 1.0):
        super().__init__(transforms=transforms, p=p)
        self.transform_indexes: List[int] = []
        self.num_transforms = num_transforms
        self.all_transforms_indexes = list(range(len(self.transforms)))
        if isinstance(num_transforms, tuple):
            self.min_num_transforms = num_transforms[0]
            self.max_num_transforms = num_transforms[1] if num_transforms[1] else len(transforms)
        else:
            self.min_num_transforms = self.max_num_transforms = num_transforms
        assert self.min_num_transforms >= 1, "min_num_transforms must be >= 1"
        assert self.min_num_transforms <= len(transforms), "num_transforms must be <= len(transforms)"
        assert self.max_num_transforms <= len(transforms), "max_num_transforms must be <= len(transforms)"

    def randomize_parameters(self) -> None:
        n = random.randint(self.min_num_transforms, self.max_num_transforms)
        self.transform_indexes = sorted(random.sample(self.all_transforms_indexes, n))

    def forward(self, samples: Optional[torch.Tensor] = None, sample_rate: Optional[int] = None) -> ObjectDict:
        inputs = ObjectDict(samples=samples, sample_rate=sample_rate)
        if random.random() < self.p:
            self.randomize_parameters()
            inputs = self._run(inputs, self.transform_indexes)
        return inputs


class OneOf(SomeOf):
    def __init__(self, transforms: List[torch.nn.Module], p: float = 1.0):
        super().__init__(num_transforms=1, transforms=transforms, p=p)
