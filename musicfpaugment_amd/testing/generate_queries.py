"""Query generation of the reference (testing/generate_queries.py): one random crop of `duration` seconds per track, and the
augmented versions of a set of clean queries.  The crops are gathered on the device (mfpa_segment_gather); file decoding
(.wav only) and the pickles stay on the host."""
from __future__ import annotations

import os
import pickle
import random
from typing import Any, List, Sequence, Tuple

import numpy as np
import torch

from .. import ops

WAVEFORM_SAMPLING_RATE = 8000          # testing/parameters.py


def draw_starts(lengths: Sequence[int], nb_samples_segment: int, burn_in: int = 0, seed: int = 42) -> Tuple[List[int], List[int]]:
    """The reference's own draws (generate_queries.py:31-49): random.seed(seed), then one
    random.randrange(burn_in, n - nb_samples_segment - burn_in) per track in order.  A track too short for the range raises inside
    the reference's try block and is skipped without a draw.  Returns (indices of the tracks that got a crop, their starts)."""
    random.seed(seed)
    idx, starts = [], []
    for i, n in enumerate(lengths):
        try:
            start = random.randrange(burn_in, int(n) - nb_samples_segment - burn_in)
        except ValueError:
            continue
        idx.append(i)
        starts.append(start)
    return idx, starts


def generate_clean_queries_batch(tracks: Sequence[Any], sr: int = WAVEFORM_SAMPLING_RATE, duration: int = 8, burn_in: int = 0,
                                 seed: int = 42, return_starts: bool = False, names: Sequence[str] = None, device="cuda"):
    """tracks: mono waveforms at `sr` (1-D float32 tensors or arrays, any device) -> (Q, sr * duration) float32 on the device, one
    crop per track that is long enough, in track order.  Too-short tracks are skipped and reported as in the reference
    ("<name> is <n>long").  `return_starts`: also the indices of the tracks that got a crop and the starts drawn."""
    nseg = int(sr) * int(duration)
    waves = [torch.as_tensor(t, dtype=torch.float32).reshape(-1) for t in tracks]
    lens = [int(w.numel()) for w in waves]
    idx, starts = draw_starts(lens, nseg, burn_in, seed)
    for i in sorted(set(range(len(waves))) - set(idx)):
        print((names[i] if names is not None else f"track {i}") + " is " + str(lens[i]) + "long")
    device = torch.device(device)
    out = torch.zeros((len(idx), nseg), dtype=torch.float32, device=device)
    if idx:
        with torch.cuda.device(device):
            off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
            if all(w.is_cuda for w in waves):
                bank = torch.cat(waves)
            else:
                bank = torch.cat([w.cpu() for w in waves]).to(device)
            src = torch.from_numpy(off[idx] + np.asarray(starts, dtype=np.int64)).to(device)
            ops.segment_gather(bank, src, None, nseg, out=out)
    return (out, idx, starts) if return_starts else out


def generate_clean_queries(md5s: List[str], save_path: str, sr: int = WAVEFORM_SAMPLING_RATE, duration: int = 8, burn_in: int = 0,
                           save: bool = False, seed: int = 42, device="cuda") -> torch.Tensor:
    """The file form (generate_queries.py:23-60), .wav only: missing files are reported and skipped, the others decoded, mixed down,
    resampled to `sr` on the device and cropped; with `save` every crop is pickled as a numpy array to
    <save_path>/<file stem>.pkl.  Returns the (Q, sr * duration) crops."""
    from ..training.dataset import read_track
    present = []
    for f in md5s:
        if os.path.isfile(f):
            present.append(f)
        else:
            print(f + "A file is missing")
    waves = [read_track(f, sr, None, device) for f in present]
    out, idx, _ = generate_clean_queries_batch(waves, sr, duration, burn_in, seed, return_starts=True, names=present, device=device)
    if save:
        host = out.cpu().numpy()
        for row, i in zip(host, idx):
            with open(save_path + "/" + present[i].split("/")[-1].split(".")[0] + ".pkl", "wb") as handle:
                pickle.dump(np.array(row), handle)
    return out


def generate_augmented_queries_batch(clean: torch.Tensor, augment, seed: int = 42) -> torch.Tensor:
    """clean (Q, T) -> augmented (Q, T): `augment.augmentation_pipeline.freeze_parameters(seed)` as generate_queries.py:73, then ONE
    `batch_augment` of the whole set.  The random draws are therefore made per batch, not per file as in the reference's loop
    (:79-86): the same distributions, another assignment of draws to queries."""
    if clean.dim() != 2:
        raise ValueError("clean queries must be (Q, T)")
    augment.augmentation_pipeline.freeze_parameters(seed)
    return augment.batch_augment(clean[:, None, :])[:, 0]
