"""AugmentationDataset: the loader the reference hands its Trainer (training/dataset.py:157-253), from audio files or waveforms
to `(clean, augmented)` pairs, with the samples on the device from the first upload on.

Per track, after mono mix-down and resampling to `sampling_frequency` (dataset.py:20-131):
  * only the first int(max_dur_in_minutes * 60 * 44100) frames of a file are read, counted at the file's own rate (:44);
  * frames of L = int(float32(dur) * float32(sr)) samples every S = int(float32(dur * step_per_cent) * float32(sr)), no end
    padding (:68-83);
  * a frame is kept iff 10 * ln(rms_frame / rms_track) > dbs_threshold (:86-99), evaluated on the device as
    sumsq_frame * N > exp(dbs / 5) * sumsq_track * L in float64 (csrc/segments.hip);
  * the kept frames are shuffled and the first `n_segments` taken (:104-122) -- here: ascending order of one random 32-bit key
    per frame, drawn before the mask is known, so the selection needs no host round trip;
  * `do_norm` divides by the track's max|x| in float32 when it is not 0 (:55-60);
  * tracks without a frame are skipped, the frames un-batched, passed through a shuffle buffer of `buffer_size`, repeated for
    ever and augmented one example at a time (:227-239).

Tracks are ingested in groups: one upload, mfpa_segment_stats / _select / _gather into a pool of rows, ONE host read (the kept
counts), and the group's audio is freed.  The shuffle buffer is TensorFlow's (emit a uniformly random slot, refill it with the
next element of the stream) run on the host over row handles; the samples never leave HBM.

Unpinned against the reference: TensorFlow and torchaudio are not installed where this was written, so TF's float32 reduction
order in the silence rule (a frame within rounding of the threshold may fall on the other side), TF's random streams
(np.random.permutation, tf.random.shuffle, the shuffle buffer) and tfio.audio.resample (here: transforms.Resample, the
torchaudio-style windowed sinc) are not reproduced bit for bit.  The dataset's own draws come from a private generator seeded by
`seed`; the global `random` / `torch` states are consumed by AugmentFP alone, exactly as when it is called directly.
"""
from __future__ import annotations

import json
import os
from typing import Any, Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch.utils.data import IterableDataset

from .. import ops

REFERENCE_RATE = 44100          # dataset.py:44 counts the frames it reads at this rate whatever the file's own


def frame_samples(duration: float, step_per_cent: float, sr: int) -> Tuple[int, int]:
    """(frame length, frame step) in samples as chunk_audio forms them (dataset.py:75-82): float32 products, truncated."""
    L = int(np.float32(duration) * np.float32(sr))
    S = int(np.float32(duration * step_per_cent) * np.float32(sr))
    return L, S


def read_track(path: str, sr: int, max_frames: Optional[int], device) -> torch.Tensor:
    """A PCM / float .wav as a mono float32 tensor at `sr` on `device`: the first `max_frames` frames of the file (at its own
    rate), channel mean (dataset.py:40-41), then transforms.Resample on the device when the rates differ."""
    if not str(path).lower().endswith(".wav"):
        raise NotImplementedError(f"{path}: only .wav inputs (decode other formats offline)")
    from scipy.io import wavfile
    rate, data = wavfile.read(path, mmap=True)
    x = np.asarray(data[:max_frames] if max_frames is not None else data)
    if x.dtype.kind == "i":
        x = x.astype(np.float32) / float(2 ** (8 * x.dtype.itemsize - 1))
    elif x.dtype.kind == "u":                                            # 8-bit PCM is unsigned
        x = (x.astype(np.float32) - 128.0) / 128.0
    else:
        x = x.astype(np.float32)
    if x.ndim == 2:
        x = x.mean(axis=1)
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(device)
    if int(rate) != int(sr) and t.numel():
        with torch.cuda.device(t.device):
            t = ops.resample(t[None], int(rate), int(sr))[0]
    return t


def shuffle_buffer(stream: Iterator[Any], buffer_size: int, rng: np.random.Generator) -> Iterator[Any]:
    """tf.data's shuffle over one pass of `stream`: fill `buffer_size` slots, then emit a uniformly random slot and refill it with
    the next element; at the end of the stream the slots drain in random order.  buffer_size 1 emits the stream order."""
    slots: List[Any] = []
    for item in stream:
        if len(slots) < buffer_size:
            slots.append(item)
            continue
        k = int(rng.integers(len(slots)))
        out, slots[k] = slots[k], item
        yield out
    while slots:
        k = int(rng.integers(len(slots)))
        out, slots[k] = slots[k], slots[-1]
        slots.pop()
        yield out


class AugmentationDataset(IterableDataset):
    """Dataset for the denoising experiments: yields `(clean (L, 1), augmented (L, 1))` float32 tensors on the device, for ever.
    `DataLoader(ds, batch_size=B)` (num_workers=0: worker processes are not supported) gives `(B, L, 1)` pairs, which
    Trainer squeezes; `batches(B)` gives the same shapes with one `batch_augment` per batch and is the fast path:
    `Trainer(model, ds.batches(B))`.

    `paths`: .wav files at any rate.  `tracks=`: waveforms already in memory instead (1-D float32 tensors or arrays, mono, at
    `sampling_frequency`, on any device).  `augment=`: an AugmentFP instance; otherwise one is built, once, from `noise_paths`
    ({scene: [files or directories]}) or from training/splits/{noise_split}.json, as the reference does per example."""

    def __init__(self, paths: Optional[Sequence[str]], sampling_frequency: int, mono: bool = True, n_segments: int = 1,
                 model_duration_seconds: float = 3.0, do_norm: bool = True, buffer_size: int = 32, noise_split: str = "train", *,
                 tracks: Optional[Sequence[Any]] = None, augment=None, noise_paths: Optional[Dict[str, List[str]]] = None,
                 step_per_cent: float = 1.0, dbs_threshold: float = -7.5, max_dur_in_minutes: float = 10.0,
                 tracks_per_group: int = 64, seed: int = 0, device="cuda") -> None:
        if not mono:
            raise NotImplementedError("mono=False: the trainer squeezes one channel (train.py:260-262)")
        if (paths is None) == (tracks is None):
            raise ValueError("pass either `paths` (.wav files) or `tracks=` (waveforms in memory)")
        if int(n_segments) < 1 or int(buffer_size) < 1 or int(tracks_per_group) < 1:
            raise ValueError("n_segments, buffer_size and tracks_per_group must be at least 1")
        self.sampling_frequency = int(sampling_frequency)
        self.n_segments, self.do_norm, self.buffer_size = int(n_segments), bool(do_norm), int(buffer_size)
        self.dbs_threshold, self.tracks_per_group, self.seed = float(dbs_threshold), int(tracks_per_group), int(seed)
        self.device = torch.device(device)
        self.L, self.S = frame_samples(model_duration_seconds, step_per_cent, self.sampling_frequency)
        ops.segment_geometry([], self.L, self.S)                         # refuses a frame the kernels do not take, at construction
        self.max_frames = int(max_dur_in_minutes * 60 * REFERENCE_RATE)
        self.song_paths = None if paths is None else [str(p) for p in paths]
        self.tracks = None if tracks is None else [torch.as_tensor(t, dtype=torch.float32).reshape(-1) for t in tracks]
        if augment is None:
            from ..augmentation import AugmentFP
            from ..augmentation.constants import IMPULSE_RESPONSE_DIR
            if noise_paths is None:
                if noise_split not in ("train", "val", "test"):
                    raise ValueError("noise_split must be 'train', 'val' or 'test'")
                with open(os.path.join("training", "splits", f"{noise_split}.json"), "r") as f:      # dataset.py:191-201
                    noise_paths = json.load(f)
            augment = AugmentFP(noise_paths, self.sampling_frequency, impulse_response_dir=IMPULSE_RESPONSE_DIR,
                                resample_banks=True, device=self.device)
        self.noise_paths = noise_paths
        self.af = augment
        self._rng = np.random.Generator(np.random.PCG64(self.seed))      # permutation, segment keys, buffer draws: nothing global
        self.last_group: Dict[str, Any] = {}                             # what the last ingested group selected (host copies; for tests and tools)

    def __len__(self) -> int:
        return len(self.song_paths if self.song_paths is not None else self.tracks)

    # ------------------------------------------------------------------ ingest
    def _load(self, idx: int) -> torch.Tensor:
        if self.tracks is not None:
            return self.tracks[idx]
        return read_track(self.song_paths[idx], self.sampling_frequency, self.max_frames, self.device)

    def ingest(self, indices: Sequence[int]) -> Tuple[torch.Tensor, List[int]]:
        """One group of tracks -> (pool (len(indices) * n_segments, L) float32 on the device, the valid rows in stream order:
        track after track, each track's winners in their drawn order).  One upload, three launches, one host read."""
        waves = [self._load(int(i)) for i in indices]
        lens = np.array([int(w.numel()) for w in waves], dtype=np.int64)
        off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64) if len(waves) else np.zeros(0, dtype=np.int64)
        seg_off = ops.segment_geometry(lens, self.L, self.S)
        ns, n = int(seg_off[-1]), len(waves)
        keys = self._rng.integers(0, 1 << 32, size=ns, dtype=np.uint32)
        pool = torch.zeros((n * self.n_segments, self.L), dtype=torch.float32, device=self.device)
        if n == 0 or ns == 0:
            return pool, []
        with torch.cuda.device(self.device):
            if all(w.is_cuda for w in waves):
                bank = torch.cat(waves)
            else:                                                        # one upload for the group
                bank = torch.cat([w.cpu() for w in waves]).to(self.device)
            # off | len as int64 and seg_off | keys as 32-bit words: two small uploads beside the audio's one
            meta64 = torch.from_numpy(np.concatenate([off, lens])).to(self.device)
            meta32 = torch.from_numpy(np.concatenate([seg_off.view(np.uint32), keys]).view(np.int32)).to(self.device)
            off_d, len_d = meta64[:n], meta64[n:]
            seg_off_d, keys_d = meta32[:n + 1], meta32[n + 1:]
            seg_sumsq, trk_sumsq, trk_peak = ops.segment_stats(bank, off_d, len_d, seg_off_d, ns, self.L, self.S)
            sel, src, div, kept = ops.segment_select(seg_sumsq, trk_sumsq, trk_peak, off_d, len_d, seg_off_d, self.L, self.S, keys_d,
                                                     self.dbs_threshold, self.n_segments, self.do_norm)
            ops.segment_gather(bank, src, div, self.L, out=pool)
            kept_h = kept.cpu().numpy()                                  # the one host read; it also orders `bank`'s release
        del bank
        rows = [i * self.n_segments + k for i in range(n) for k in range(min(int(kept_h[i]), self.n_segments))]
        self.last_group = {"indices": [int(i) for i in indices], "kept": kept_h, "sel": sel, "seg_off": seg_off, "keys": keys}
        return pool, rows

    # ------------------------------------------------------------------ streams
    def _pass(self) -> Iterator[torch.Tensor]:
        """One pass over the tracks in a fresh permutation: every selected chunk, (L,) views of the group pools."""
        order = self._rng.permutation(len(self))
        for g in range(0, len(order), self.tracks_per_group):
            pool, rows = self.ingest(order[g:g + self.tracks_per_group])
            for r in rows:
                yield pool[r]

    def chunks(self) -> Iterator[torch.Tensor]:
        """The clean stream: .unbatch().shuffle(buffer_size, reshuffle_each_iteration=True).repeat() of dataset.py:228-230."""
        while True:
            n = 0
            for c in shuffle_buffer(self._pass(), self.buffer_size, self._rng):
                n += 1
                yield c
            if n == 0:
                raise RuntimeError("no track has a non-silent chunk of the model's duration: the dataset is empty")

    def __iter__(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        """(clean (L, 1), augmented (L, 1)): AugmentFP.__call__ per example (dataset.py:139-154)."""
        info = torch.utils.data.get_worker_info()
        if info is not None:
            raise RuntimeError("AugmentationDataset feeds from the GPU: use DataLoader(..., num_workers=0)")
        for c in self.chunks():
            aug = self.af(c.reshape(1, -1))                              # (1, L)
            yield c.reshape(-1, 1), aug.reshape(-1, 1)

    def batches(self, batch_size: int) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        """(clean (B, L, 1), augmented (B, L, 1)) with one `batch_augment` per batch: with the default clipping_scope="example" the
        same arithmetic per example as __iter__, the random draws made per batch instead of per example."""
        if int(batch_size) < 1:
            raise ValueError("batch_size must be at least 1")
        stream = self.chunks()
        while True:
            clean = torch.stack([next(stream) for _ in range(int(batch_size))])      # (B, L): one device copy
            aug = self.af.batch_augment(clean[:, None, :])
            yield clean.unsqueeze(-1), aug[:, 0, :, None]
