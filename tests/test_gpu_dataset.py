"""GPU: AugmentationDataset (training/dataset.py) and the query generators (testing/generate_queries.py) on in-memory tracks and
synthetic augmentation banks: every chunk against the numpy restatement of the segment stage (tests/_segments_oracle.py), the
stream order, the shapes the Trainer takes, the replay of an augmented batch, .wav input and one train step."""
import random
from collections import Counter

import numpy as np
import pytest
import torch

from tests import _segments_oracle as so

pytestmark = pytest.mark.gpu

SR = 8000
DUR = 0.05                                                               # L = 400 samples: the chunk logic does not care
LENGTHS = [0, 399, 400, 1000, 2407, 4000, 3203, 801]


@pytest.fixture(scope="module")
def af():
    from musicfpaugment_amd.augmentation import AugmentFP, synthetic_banks
    irs, noises = synthetic_banks(3)
    return AugmentFP(ir_bank=irs, noise_bank=noises)


@pytest.fixture(scope="module")
def tracks():
    L, S = so.frame_samples(DUR, 1.0, SR)
    assert (L, S) == (400, 400)
    out = so.make_tracks(4300, L, S, LENGTHS)
    out[5][:] = 0                                                        # an all-zero track
    out[6][400:800] = 0                                                  # an exactly silent segment
    return out


def _segments(tracks, L, S, do_norm=True):
    """{bytes of a normalised segment: (track, j)} for the kept and for the silent segments, and the kept count per track."""
    kept, silent, counts = {}, {}, []
    for i, t in enumerate(tracks):
        seg, trk, peak = so.stats(t, L, S)
        m = so.keep(seg, trk, len(t), L)
        assert np.all(so.margin(seg, trk, len(t), L) >= 1e-6)
        counts.append(int(m.sum()))
        for j in range(len(seg)):
            (kept if m[j] else silent)[so.divide(t[j * S: j * S + L], peak, do_norm).tobytes()] = (i, j)
    return kept, silent, counts


def _dataset(tracks, af, **kw):
    from musicfpaugment_amd.training.dataset import AugmentationDataset
    a = dict(model_duration_seconds=DUR, tracks=tracks, augment=af)
    a.update(kw)
    return AugmentationDataset(None, SR, **a)


@pytest.mark.parametrize("n_segments,group,buffer", [(1, 64, 32), (2, 3, 4), (16, 5, 1)])
def test_every_chunk_is_a_kept_segment(tracks, af, n_segments, group, buffer):
    ds = _dataset(tracks, af, n_segments=n_segments, tracks_per_group=group, buffer_size=buffer)
    assert (ds.L, ds.S) == (400, 400) and len(ds) == len(tracks)
    kept, silent, counts = _segments(tracks, ds.L, ds.S)
    assert len(silent) >= 3 and max(counts) > 2 and min(counts) == 0
    per_pass = sum(min(c, n_segments) for c in counts)
    stream = ds.chunks()
    for _ in range(2):                                                   # two passes: a fresh permutation, the same multiset sizes
        seen = Counter()
        got = set()
        for _ in range(per_pass):
            c = next(stream)
            assert c.shape == (ds.L,) and c.is_cuda and c.dtype == torch.float32
            b = c.cpu().numpy().tobytes()
            assert b in kept and b not in silent
            assert b not in got                                          # a segment at most once per pass
            got.add(b)
            seen[kept[b][0]] += 1
        assert all(seen[i] == min(counts[i], n_segments) for i in range(len(tracks)))
        if n_segments >= max(counts):
            assert got == set(kept)                                      # the multiset of a pass: every kept segment, once


def test_buffer_of_one_emits_the_stream_order(tracks, af):
    """One group, buffer_size 1: the tracks in the drawn permutation, each track's winners in ascending (key, index) order of the
    keys the dataset drew -- the oracle's selection from those keys."""
    ds = _dataset(tracks, af, n_segments=2, buffer_size=1, seed=7)
    _, _, counts = _segments(tracks, ds.L, ds.S)
    per_pass = sum(min(c, 2) for c in counts)
    stream = ds.chunks()
    got = [next(stream).cpu().numpy() for _ in range(per_pass)]
    g = ds.last_group
    order = g["indices"]
    assert sorted(order) == list(range(len(tracks))) and order != sorted(order)
    perm = [tracks[i] for i in order]
    _, wkept, wsel = so.select_all(perm, ds.L, ds.S, g["keys"], 2)
    assert np.array_equal(g["kept"], wkept) and np.array_equal(g["sel"].cpu().numpy(), wsel)
    seg_off = so.geometry([len(t) for t in perm], ds.L, ds.S)
    want = []
    for i, t in enumerate(perm):
        for s in wsel[2 * i: 2 * i + 2]:
            if s >= 0:
                j = int(s - seg_off[i])
                want.append(so.divide(t[j * ds.S: j * ds.S + ds.L], so.stats(t, ds.L, ds.S)[2]))
    assert len(want) == per_pass and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, want))
    # the same seed gives the same stream; the global generators are not consulted
    random.seed(1); torch.manual_seed(1)
    again = _dataset(tracks, af, n_segments=2, buffer_size=1, seed=7).chunks()
    assert all(np.array_equal(next(again).cpu().numpy(), a) for a in got)


def test_do_norm_off_hands_out_the_samples_themselves(tracks, af):
    ds = _dataset(tracks, af, n_segments=16, do_norm=False)
    kept, _, counts = _segments(tracks, ds.L, ds.S, do_norm=False)
    stream = ds.chunks()
    assert {next(stream).cpu().numpy().tobytes() for _ in range(sum(counts))} == set(kept)


def test_shapes_and_loaders(af):
    from torch.utils.data import DataLoader
    L = 4000
    trk = so.make_tracks(4400, L, L, [3 * L + 5, L, 0, 2 * L + 1])
    ds = _dataset(trk, af, model_duration_seconds=0.5, n_segments=2, buffer_size=3)
    clean, aug = next(iter(ds))
    assert clean.shape == (L, 1) and aug.shape == (L, 1) and clean.is_cuda and aug.is_cuda and aug.dtype == torch.float32
    assert bool(torch.isfinite(aug).all()) and not torch.equal(clean, aug)
    cb, ab = next(iter(DataLoader(ds, batch_size=4)))
    assert cb.shape == (4, L, 1) and ab.shape == (4, L, 1) and cb.is_cuda
    c2, a2 = next(ds.batches(4))
    assert c2.shape == (4, L, 1) and a2.shape == (4, L, 1) and c2.is_cuda and bool(torch.isfinite(a2).all())
    with pytest.raises(NotImplementedError):
        _dataset(trk, af, mono=False)
    with pytest.raises(RuntimeError):
        next(_dataset([np.zeros(3 * L, dtype=np.float32), np.ones(L - 1, dtype=np.float32)], af, model_duration_seconds=0.5).chunks())


def test_an_augmented_batch_replays(af):
    """The dataset draws nothing from the global generators: re-seeded, batch_augment of the clean batch gives the batch's aug."""
    L = 4000
    trk = so.make_tracks(4500, L, L, [3 * L + 5, L, 2 * L + 1, 4 * L])
    gen = _dataset(trk, af, model_duration_seconds=0.5, n_segments=2, buffer_size=4, tracks_per_group=2).batches(3)
    next(gen)                                                            # (a batch that spans groups lies ahead either way)
    for seed in (11, 12):
        random.seed(seed); torch.manual_seed(seed)
        clean, aug = next(gen)
        random.seed(seed); torch.manual_seed(seed)
        want = af.batch_augment(clean[:, :, 0].contiguous()[:, None, :])
        assert torch.equal(aug[:, :, 0], want[:, 0])
    # ... and one example at a time, as __iter__ does
    it = iter(_dataset(trk, af, model_duration_seconds=0.5, buffer_size=1))
    random.seed(13); torch.manual_seed(13)
    clean, aug = next(it)
    random.seed(13); torch.manual_seed(13)
    assert torch.equal(aug[:, 0], af(clean[:, 0].contiguous()[None])[0])


def test_wav_files_are_resampled_on_the_device(af, tmp_path):
    from scipy.io import wavfile
    from musicfpaugment_amd import ops, synth
    L, paths, decoded = 2000, [], []
    for k in range(3):
        x = (synth.batch(1, seed=4600 + k, n=16000 + 37 * k)[0] * 32767).astype(np.int16)
        x[4000 * k: 4000 * k + 4500] //= 64                              # a quiet stretch somewhere
        wavfile.write(tmp_path / f"t{k}.wav", 16000, x)
        paths.append(str(tmp_path / f"t{k}.wav"))
        decoded.append(x.astype(np.float32) / 32768.0)

    def expect(frames):
        out = [ops.resample(torch.from_numpy(d[:frames])[None].cuda(), 16000, SR)[0].cpu().numpy() for d in decoded]
        return _segments(out, L, L)

    from musicfpaugment_amd.training.dataset import AugmentationDataset
    ds = AugmentationDataset(paths, SR, n_segments=16, model_duration_seconds=0.25, augment=af, buffer_size=2)
    kept, _, counts = expect(None)
    assert sum(counts) >= 6
    stream = ds.chunks()
    assert {next(stream).cpu().numpy().tobytes() for _ in range(sum(counts))} == set(kept)
    # only the first int(minutes * 60 * 44100) frames of a file are read, counted at the file's own rate
    minutes = 8000.5 / (60 * 44100)
    ds = AugmentationDataset(paths, SR, n_segments=16, model_duration_seconds=0.25, augment=af, max_dur_in_minutes=minutes)
    assert ds.max_frames == 8000
    kept, _, counts = expect(8000)
    assert sum(counts) >= 3 and all(c <= 2 for c in counts)
    stream = ds.chunks()
    assert {next(stream).cpu().numpy().tobytes() for _ in range(sum(counts))} == set(kept)
    with pytest.raises(NotImplementedError):
        next(AugmentationDataset(["x.mp3"], SR, augment=af).chunks())


def test_one_train_step_from_the_dataset(af):
    from musicfpaugment_amd import synth
    from musicfpaugment_amd.training.train import Trainer
    from musicfpaugment_amd.training.unet import UNet
    from musicfpaugment_amd.training.weights import formula_state_dict
    trk = [synth.batch(1, seed=4700 + k, n=24000 * 2 + 11)[0] for k in range(3)]
    ds = _dataset(trk, af, model_duration_seconds=3.0, n_segments=2, buffer_size=4)
    assert ds.L == 24000
    net = UNet(1, 1, rate=0.0)
    net.load_state_dict(formula_state_dict(3))
    tr = Trainer(net, ds.batches(2), None, learning_rate=1e-3)
    clean, aug = next(tr.train_loader_iter)
    assert clean.shape == (2, 24000, 1) and aug.shape == (2, 24000, 1)
    loss = tr.train_step(clean, aug)
    assert bool(torch.isfinite(loss).all())


def test_clean_queries_replay_the_references_draws():
    from musicfpaugment_amd.testing.generate_queries import generate_clean_queries_batch
    rng = np.random.default_rng(4800)
    lens = [1200, 799, 800, 801, 5000, 0]
    trk = [rng.standard_normal(n).astype(np.float32) for n in lens]
    q, idx, starts = generate_clean_queries_batch(trk, sr=100, duration=8, return_starts=True)
    random.seed(42)                                                      # generate_queries.py:31-49 on the host
    want_idx, want_starts = [], []
    for i, n in enumerate(lens):
        try:
            want_starts.append(random.randrange(0, n - 800))
            want_idx.append(i)
        except ValueError:
            pass
    assert idx == want_idx == [0, 3, 4] and starts == want_starts
    assert q.shape == (3, 800) and q.is_cuda
    for row, i, s in zip(q.cpu().numpy(), idx, starts):
        assert np.array_equal(row.view(np.uint32), trk[i][s: s + 800].view(np.uint32))
    q2 = generate_clean_queries_batch(trk, sr=100, duration=8, burn_in=100, seed=5)
    random.seed(5)
    s0, s4 = random.randrange(100, 1200 - 800 - 100), random.randrange(100, 5000 - 800 - 100)
    assert q2.shape == (2, 800) and np.array_equal(q2[1].cpu().numpy(), trk[4][s4: s4 + 800]) and np.array_equal(q2[0].cpu().numpy(), trk[0][s0: s0 + 800])


def test_query_files_and_augmented_queries(af, tmp_path):
    import pickle
    from scipy.io import wavfile
    from musicfpaugment_amd import ops, synth
    from musicfpaugment_amd.testing.generate_queries import generate_augmented_queries_batch, generate_clean_queries
    x = synth.batch(1, seed=4900, n=40000)[0].astype(np.float32)
    wavfile.write(tmp_path / "abc.wav", 16000, x)
    files = [str(tmp_path / "abc.wav"), str(tmp_path / "missing.wav")]
    q = generate_clean_queries(files, str(tmp_path), sr=SR, duration=2, save=True)
    y = ops.resample(torch.from_numpy(x)[None].cuda(), 16000, SR)[0]
    random.seed(42)
    s = random.randrange(0, y.numel() - 16000)
    assert q.shape == (1, 16000) and torch.equal(q[0], y[s: s + 16000])
    with open(tmp_path / "abc.pkl", "rb") as fh:
        assert np.array_equal(pickle.load(fh), q[0].cpu().numpy())
    aug = generate_augmented_queries_batch(q.repeat(3, 1), af, seed=42)
    af.augmentation_pipeline.freeze_parameters(42)
    assert aug.shape == (3, 16000) and torch.equal(aug, af.batch_augment(q.repeat(3, 1)[:, None, :])[:, 0])
    af.augmentation_pipeline.unfreeze_parameters()
