"""AddBackgroundNoise (reference augmentation/transformations/background_noise.py, non-mixup branch) on the device: random slices
of a noise bank resident in HBM, RMS-normalised and concatenated to the clip length, mixed in at a random SNR, peak-normalised.

The bank is given in memory (`noise_bank=`, {scene: [tensors]}) or read ONCE at construction from `background_paths`
({scene: [.wav files or directories]}) -- AugmentFP's resident-bank layout and its `resample_banks=` switch."""
from __future__ import annotations

import random
from typing import Dict, List, Optional

import numpy as np
import torch

from ..._lib import check, lib, ptr, stream
from .. import _find_wavs, _read_wav, _up
from ..transform import BaseWaveformTransform, EmptyPathException
from . import as_bank, bank_offsets, u8, uniform


class AddBackgroundNoise(BaseWaveformTransform):
    def __init__(self, background_paths: Optional[Dict[str, List[str]]] = None, min_snr_in_db: float = 3.0,
                 max_snr_in_db: float = 30.0, p: float = 0.5, sample_rate: Optional[int] = None, *,
                 noise_bank: Optional[Dict[str, List[torch.Tensor]]] = None, resample_banks: bool = False, device="cuda") -> None:
        super().__init__(p=p, sample_rate=sample_rate)
        if min_snr_in_db > max_snr_in_db:
            raise ValueError("min_snr_in_db must not be greater than max_snr_in_db")
        if noise_bank is None:
            if background_paths is None or sample_rate is None:
                raise ValueError("pass `background_paths` ({scene: [files or directories]}) and `sample_rate`, or an in-memory "
                                 "`noise_bank`")
            noise_bank = {scene: [_read_wav(f, int(sample_rate), resample_banks) for f in _find_wavs(paths)]
                          for scene, paths in background_paths.items()}
            noise_bank = {k: v for k, v in noise_bank.items() if len(v) > 0}
        if len(noise_bank) == 0:
            raise EmptyPathException("There are no supported audio files found.")
        self.min_snr_in_db = min_snr_in_db
        self.max_snr_in_db = max_snr_in_db
        self.noise_bank = {k: as_bank(v) for k, v in noise_bank.items()}
        files = [(scene, k) for scene, v in self.noise_bank.items() for k in range(len(v))]
        flat = [self.noise_bank[sc][k] for sc, k in files]
        self._noise_off = dict(zip(files, bank_offsets(flat).tolist()))
        self._noise_dev = torch.cat(flat).to(torch.device(device))

    def _random_background(self, T: int):
        """background_noise.py:64-141: random scene, random file, random offset, until T samples: [(scene, file, offset, length)]."""
        pieces, missing = [], T
        while missing > 0:
            scene = random.choice(list(self.noise_bank.keys()))
            k = random.randrange(len(self.noise_bank[scene]))
            n = len(self.noise_bank[scene][k])
            if n >= missing:
                pieces.append((scene, k, random.randint(0, n - missing), missing))
                missing = 0
            else:
                pieces.append((scene, k, 0, n))
                missing -= n
        return pieces

    def randomize_parameters(self, x, sample_rate) -> None:
        """Which slices, gathered on the device at once (the SNR is drawn after them, as AugmentFP does)."""
        B, T = x.shape
        dev, should = x.device, self.transform_parameters["should_apply"]
        self.pieces = [self._random_background(T) for _ in range(B)]
        P = max(len(pc) for pc in self.pieces)
        src, ln = np.zeros((B, P), dtype=np.int64), np.zeros((B, P), dtype=np.int32)
        for b, pc in enumerate(self.pieces):
            for j, (scene, k, off, n) in enumerate(pc):
                src[b, j], ln[b, j] = self._noise_off[(scene, k)] + off, n
        src_d, ln_d = _up(torch.from_numpy(src), dev), _up(torch.from_numpy(ln), dev)
        self.background = torch.empty((B, T), dtype=torch.float32, device=dev)
        check(lib().mfpa_gather_background(ptr(self._noise_dev), ptr(src_d), ptr(ln_d), B, P, T, ptr(self.background), stream()),
              "mfpa_gather_background")
        self.snr_in_db = uniform(self.min_snr_in_db, self.max_snr_in_db, B)
        sel = _up(torch.nonzero(should).flatten(), dev)              # host-known indices: no device-side nonzero, no sync
        self.transform_parameters.update(background=self.background.index_select(0, sel), snr_in_db=self.snr_in_db[should])

    def apply_transform(self, x, sample_rate):
        B, T = x.shape
        y, snr_d = torch.empty_like(x), _up(self.snr_in_db, x.device)
        on_d = u8(self.transform_parameters["should_apply"], x.device)
        check(lib().mfpa_mix_background(ptr(x), B, T, ptr(self.background), ptr(snr_d), ptr(on_d), ptr(y), stream()),
              "mfpa_mix_background")
        return y
