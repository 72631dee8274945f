"""RoomReverb: reverberation without a dataset of measured impulse responses (it is not in the reference tree; the name follows
audiomentations' RoomSimulator).  Each example gets its own shoebox room, source, microphone and decay-time target, drawn on the
host with `random`; ONE ops.simulate_rir launch makes the batch's impulse responses on the device (csrc/rir.hip, time-reversed:
the taps mfpa_fir wants), and the convolution is ApplyImpulseResponse's, launch for launch: mfpa_fir with out_mode 2, division by
the peak of the full convolution, cut to the input length.

`rt60` is the design target of Eyring's formula, not a promise: the walls get the uniform absorption eyring_absorption(room, rt60),
and with a uniform coefficient the image-source decay is slower than Eyring's diffuse-field estimate.  For the room (3.0, 2.5, 2.2) m
at 8 kHz, source (1.1, 0.9, 1.2), microphone (2.2, 1.7, 0.8), targets of 0.1, 0.2 and 0.3 s (orders 16, 32 and 47) measured 0.145,
0.273 and 0.396 s, as 3 x the -5 ... -25 dB span of the Schroeder curve of the response truncated to rt60 seconds
(tests/test_rir_oracle.py).

One call has one reflection order and one response length: the order is the largest of the examples' own orders
min(rir_max_order(room, rt60), max_order), the length ceil(max rt60 of the batch x sample_rate)."""
from __future__ import annotations

import math
import random
from typing import Optional, Sequence

import numpy as np
import torch

from ... import ops
from ..._lib import check, lib, ptr, stream
from ...functional import eyring_absorption, rir_max_order
from .. import _up
from ..transform import BaseWaveformTransform
from . import u8


class RoomReverb(BaseWaveformTransform):
    def __init__(self, min_rt60: float = 0.1, max_rt60: float = 0.5, min_room_dim: Sequence[float] = (3.0, 2.5, 2.2),
                 max_room_dim: Sequence[float] = (10.0, 8.0, 4.0), min_wall_distance: float = 0.5, max_order: int = 64, p: float = 0.5,
                 sample_rate: Optional[int] = None) -> None:
        super().__init__(p=p, sample_rate=sample_rate)
        if not 0.0 < min_rt60 <= max_rt60 or not math.isfinite(max_rt60):
            raise ValueError(f"0 < min_rt60 <= max_rt60 is required, got {min_rt60}, {max_rt60}")
        lo, hi = tuple(float(v) for v in min_room_dim), tuple(float(v) for v in max_room_dim)
        if len(lo) != 3 or len(hi) != 3 or not all(math.isfinite(b) and 0.0 < a <= b for a, b in zip(lo, hi)):
            raise ValueError(f"room dimensions need three sides with 0 < min <= max, got {min_room_dim}, {max_room_dim}")
        if not min_wall_distance > 0.0 or not all(a > 2.0 * min_wall_distance for a in lo):
            raise ValueError(f"min_wall_distance ({min_wall_distance}) must be positive and below half the shortest side of {min_room_dim}")
        if int(max_order) != max_order or not 0 <= max_order <= ops.RIR_MAX_ORDER:
            raise ValueError(f"max_order must be an integer in [0, {ops.RIR_MAX_ORDER}], got {max_order}")
        self.min_rt60, self.max_rt60 = float(min_rt60), float(max_rt60)
        self.min_room_dim, self.max_room_dim = lo, hi
        self.min_wall_distance, self.max_order = float(min_wall_distance), int(max_order)

    def randomize_parameters(self, x, sample_rate) -> None:
        B, should = x.shape[0], self.transform_parameters["should_apply"]
        w = self.min_wall_distance
        room, source, mic, rt60 = np.empty((B, 3)), np.empty((B, 3)), np.empty((B, 3)), np.empty(B)
        for b in range(B):
            room[b] = [random.uniform(a, c) for a, c in zip(self.min_room_dim, self.max_room_dim)]
            source[b] = [random.uniform(w, side - w) for side in room[b]]
            mic[b] = [random.uniform(w, side - w) for side in room[b]]
            while np.array_equal(mic[b], source[b]):
                mic[b] = [random.uniform(w, side - w) for side in room[b]]
            rt60[b] = random.uniform(self.min_rt60, self.max_rt60)
        self.room, self.source, self.mic, self.rt60 = room, source, mic, rt60
        self.absorption = np.repeat(eyring_absorption(room, rt60)[:, None], 6, axis=1)
        self.order = int(np.minimum(rir_max_order(room, rt60), self.max_order).max())
        self.ir_length = int(math.ceil(float(rt60.max()) * sample_rate))
        if not 1 <= self.ir_length <= ops.RIR_MAX_LENGTH:
            raise ValueError(f"max rt60 x sample_rate = {self.ir_length} samples: the response must have 1 to {ops.RIR_MAX_LENGTH}")
        keep = should.numpy()
        self.transform_parameters.update(rt60=torch.from_numpy(rt60[keep]), room=torch.from_numpy(room[keep]),
                                         source=torch.from_numpy(source[keep]), mic=torch.from_numpy(mic[keep]),
                                         absorption=torch.from_numpy(self.absorption[keep]), max_order=self.order)

    def apply_transform(self, x, sample_rate):
        B, T = x.shape
        dev, L, n = x.device, lib(), self.ir_length
        taps = ops.simulate_rir(self.room, self.source, self.mic, self.absorption, self.order, n, sample_rate, reversed=True, device=dev)
        self.transform_parameters["ir"] = taps.flip(-1)              # every row of the batch, selected or not, not reversed
        n_d = _up(torch.full((B,), n, dtype=torch.int32), dev)
        off_d = n_d - 1                                              # y[t] = sum_k ir[n-1-k] x[t + k - (n-1)]
        toff_d = _up(torch.arange(B, dtype=torch.int64) * n, dev)
        y, peak = torch.empty_like(x), torch.empty((B,), dtype=torch.float32, device=dev)
        on_d = u8(self.transform_parameters["should_apply"], dev)
        check(L.mfpa_fir(ptr(x), B, T, T + n - 1, ptr(taps), ptr(toff_d), ptr(n_d), ptr(off_d), ptr(on_d), 1, 2, ptr(y), ptr(peak), stream()),
              "mfpa_fir")
        check(L.mfpa_scale_rows(ptr(y), B, T, ptr(peak), ptr(on_d), 1, ptr(y), stream()), "mfpa_scale_rows")
        return y
