"""GPU: Audfprint on whole tracks (csrc/audfprint.hip and csrc/hashes.hip, Audfprint_peaks(whole_tracks=True), create_fp_database*(whole_tracks=True)).

Every comparison is EQUALITY: the path is integer or bit-exact float64 by construction, as for the clip kernels.
  1. the same answers as the clip kernels wherever both apply (pick and landmarks, every tile seam);
  2. beyond the clip kernels' limits, against the oracle and the reference's own lists (tests/golden/g17_track.npz);
  3. the maximum, 16384 frames, and one frame more;
  4. landmark capacity: more than 8192 landmarks, 8 and 9 peaks in a frame, cap one short;
  5. shifts = 4;  6. the identification experiment end to end on whole tracks;  7. the file-based entry points.
"""
import os

import numpy as np
import pytest
import torch

from musicfpaugment_amd import synth
from oracle import audfprint as oa
from oracle import hashes as oh
from tests import _identify_oracle as io_
from tests import _track_cases as tc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _ops():
    from musicfpaugment_amd import ops
    return ops


def _analyzer(**kw):
    from musicfpaugment_amd.afp.audfprint.peak_extractor import Audfprint_peaks
    return Audfprint_peaks(None, whole_tracks=True, **kw)


def _oracle(d):
    """(mask (256, T) uint8, unique sorted (time, hash) rows) of one waveform, by the CPU oracle."""
    with np.errstate(all="ignore"):                              # an all-zero clip is 0 / 0 there, as in the reference
        mask = oa.find_peaks(d)[1]
    mask = (np.asarray(mask) != 0).astype(np.uint8)
    return mask, oh.audfprint_hashes_from_mask(mask)


def _rows(uq, n, i):
    return uq[i, :int(n[i])].cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. against the clip kernels
CLIP_FRAMES = 1434                                                   # see clip_masks


@pytest.fixture(scope="module")
def clip_masks():
    """Masks of the CLIP kernels (audfprint_prepare + audfprint_prune) for 8 clips of 251 frames and 4 noise clips of 1434 frames,
    with the spectrograms they came from.  1434 frames (45 chunks of np.mean's reduction) is the most the frame-major float64
    mfpa_audfprint_prepare can be launched with: its LDS request grows by 2 KB per chunk and passes the CU's 160 KB at 46 (the
    1500 frames its documentation names are a launch error, hipErrorInvalidValue).  1500 frames are compared with the oracle
    below, and their landmarks with the clip kernel."""
    ops = _ops()
    out = []
    for wav in (synth.batch(8), np.stack([tc.noise(tc.samples(CLIP_FRAMES), seed=30 + k) for k in range(4)])):
        mag, cmax = ops.stft_mag(torch.from_numpy(wav).cuda(), torch.float64)
        filtered = ops.audfprint_prepare(mag, cmax, mean_order=1, denom_is_clip_max=True)
        mask, npeaks = ops.audfprint_prune(filtered)
        out.append((mag, cmax, mask, npeaks))
    return out


@pytest.mark.parametrize("which, frames", [(0, 251), (1, CLIP_FRAMES)])
def test_pick_track_equals_the_clip_kernels(clip_masks, which, frames):
    mag, cmax, mask, npeaks = clip_masks[which]
    assert mag.shape[2] == frames
    got_mask, got_n = _ops().audfprint_pick_track(mag, cmax)
    assert int(npeaks.min()) > 0
    assert torch.equal(got_n, npeaks)
    assert torch.equal(got_mask, mask)
    if frames <= 512:                                            # the fused clip picker too
        m2, n2 = _ops().audfprint_pick(mag, cmax)
        assert torch.equal(got_mask, m2) and torch.equal(got_n, n2)


def test_pick_track_equals_prepare_plus_prune_on_short_ragged_and_silent_clips():
    """The five batches of test_fused_pick_equals_prepare_plus_prune_bit_for_bit (tests/test_gpu_peaks.py) and one of 1280 samples
    through the pruner's global-workspace form: frame counts that are no multiple of four, a silent clip (denom == 0), a half-silent
    one, the launcher's memset in place of the kernel's own zeroing; exactly ten frames (2304 samples: 2304 // 256 + 1) and six (1280
    samples: the `T < 10` side of the seed over the first ten frames).  Identical masks and counts; and at least one clip of every
    batch of more than ten frames has peaks, so that two empty masks cannot pass for coverage.  With ten frames or fewer the pruner
    seeds its threshold with the maximum over every frame the clip has, so such clips may find no peak at all."""
    ops = _ops()
    for n, B in ((64000, 12), (24000, 5), (2304, 3), (8000 + 77, 4), (130560, 2), (1280, 3)):
        wav = np.stack([synth.clip(700 + i, n=n, tonal=(i % 3 != 1)) for i in range(B)])
        if B > 3:
            wav[1] = 0.0
            wav[2, : n // 2] = 0.0
        mag, cmax = ops.stft_mag(torch.from_numpy(wav).cuda(), torch.float64)
        assert mag.shape[2] == n // 256 + 1
        a_dec = ops.audfprint_a_dec()
        want_mask, want_n = ops.audfprint_prune(ops.audfprint_prepare(mag, cmax, mean_order=1, denom_is_clip_max=True), a_dec)
        got_mask, got_n = ops.audfprint_pick_track(mag, cmax, a_dec)
        assert torch.equal(got_mask, want_mask) and torch.equal(got_n, want_n), (n, B)
        if mag.shape[2] > 10:
            assert int(want_n.max()) > 0, (n, B)
        if B > 3:
            assert int(got_n[1]) == 0                            # the silent clip


def _landmarks_both(mask, cap=8192):
    ops = _ops()
    want = ops.audfprint_landmarks(mask, cap)
    got = ops.audfprint_landmarks_track(mask, cap, want_lists=True)
    return got, want


@pytest.mark.parametrize("which", [0, 1])
def test_landmarks_track_equals_the_clip_kernel_on_picked_masks(clip_masks, which):
    """1434 frames span six tiles: every seam is checked against the one-workgroup kernel."""
    mask = clip_masks[which][2]
    got, want = _landmarks_both(mask)
    assert int(want[3].min()) > 0
    for g, w, name in zip(got, want, ("landmarks", "hashes", "uniq", "counts")):
        assert torch.equal(g, w), name
    nolist = _ops().audfprint_landmarks_track(mask, 8192)
    assert nolist[0] is None and nolist[1] is None and torch.equal(nolist[2], want[2]) and torch.equal(nolist[3], want[3])


def test_1500_frames_equal_the_oracle_and_the_clip_landmark_kernel():
    """The clip pruner's last length.  The picker against the oracle (the clip kernels' first stage cannot be launched here, see
    clip_masks), through the analyzer with the switch on; the landmarks, all four outputs, against the clip kernel on those masks."""
    wav = np.stack([tc.noise(tc.samples(1500), seed=30 + k) for k in range(4)])
    x = torch.from_numpy(wav).cuda()
    mag, cmax = _ops().stft_mag(x, torch.float64)
    mask, npeaks = _ops().audfprint_pick_track(mag, cmax)
    assert mask.shape == (4, 256, 1500)
    an = _analyzer()
    m2, n2, _ = an.find_peaks_batch(x)
    assert torch.equal(m2, mask) and torch.equal(n2, npeaks)
    uq, n = an.hashes_batch(x, shifts=1)
    for b in range(4):
        want_mask, want_rows = _oracle(wav[b])
        assert int(npeaks[b]) == int(want_mask.sum()) > 500
        assert np.array_equal(mask[b].cpu().numpy(), want_mask), b
        np.testing.assert_array_equal(_rows(uq, n, b), want_rows)
    got, want = _landmarks_both(mask)
    assert int(want[3].min()) > 0
    for g, w, name in zip(got, want, ("landmarks", "hashes", "uniq", "counts")):
        assert torch.equal(g, w), name


@pytest.mark.parametrize("T", [1, 62, 63, 256, 257, 319])
def test_landmarks_track_equals_the_clip_kernel_on_random_masks(T):
    """0-8 peaks per frame, bins anywhere (duplicate hashes do not occur within one shift; the seams at 256 / 256 + 62 frames do)."""
    rng = np.random.default_rng(100 + T)
    mask = np.zeros((2, 256, T), np.uint8)
    for b in range(2):
        for t in range(T):
            k = int(rng.integers(0, 9))
            lo = int(rng.integers(0, 200)) if b == 0 else 0          # clip 0: peaks close together (many pairs), clip 1: anywhere
            bins = rng.choice(np.arange(lo, lo + 56) if b == 0 else np.arange(256), k, replace=False)
            mask[b, bins, t] = 1
    got, want = _landmarks_both(torch.from_numpy(mask).cuda())
    assert (want[3].cpu().numpy() >= 0).all()
    if T >= 62:
        assert int(want[3][:, 0].max()) > 0
    for g, w, name in zip(got, want, ("landmarks", "hashes", "uniq", "counts")):
        assert torch.equal(g, w), (T, name)
    for b in range(2):                                               # and the oracle, so that the two kernels do not share a mistake
        n = int(got[3][b, 1])
        np.testing.assert_array_equal(got[2][b, :n].cpu().numpy(), oh.audfprint_hashes_from_mask(mask[b]))


# ------------------------------------------------------------------------------------------------ 2. beyond the old limits
def _batch_of(frames):
    n = tc.samples(frames)
    return np.stack([tc.noise(n), tc.noise_gap(n), tc.track_noise(n), np.zeros(n, np.float32)])


@pytest.mark.parametrize("frames", [1501, 2040, 2041])
def test_long_clips_equal_the_oracle(frames):
    """2040 frames: the last length inside 64 chunks of np.mean's reduction; 2041 the first outside (257 * 2041 = 524537 > 524288)."""
    wav = _batch_of(frames)
    an = _analyzer()
    x = torch.from_numpy(wav).cuda()
    mask, npeaks, spec = an.find_peaks_batch(x)
    uq, n = an.hashes_batch(x, shifts=1)
    assert mask.shape == (4, 256, frames) and spec.shape == (4, 257, frames) and spec.dtype == torch.float64
    for b in range(4):
        want_mask, want_rows = _oracle(wav[b])
        got = mask[b].cpu().numpy()
        assert int(npeaks[b]) == int(want_mask.sum())
        assert np.array_equal(got, want_mask), (frames, b, int(np.count_nonzero(got != want_mask)))
        np.testing.assert_array_equal(_rows(uq, n, b), want_rows)
    assert int(npeaks[0]) > 500 and int(npeaks[1]) > 50 and int(npeaks[2]) > 100 and int(npeaks[3]) == 0 and int(n[3]) == 0
    from oracle import stft as ostft                                 # find_peaks still returns the normalised spectrogram
    sg = ostft.magnitude(wav[2])
    np.testing.assert_allclose(spec[2].cpu().numpy(), sg / sg.max(), rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_g17_inputs_equal_the_reference(name):
    g = np.load(os.path.join(GOLDEN, "g17_track.npz"))
    d = tc.g17_inputs()[name]
    assert synth.digest(d) == str(g[f"digest_{name}"])
    an = _analyzer()
    pklist, mask, spec = an.find_peaks(d)
    np.testing.assert_array_equal(np.array(pklist, np.int64).reshape(-1, 2), g[f"pklist_{name}"].astype(np.int64))
    assert mask.shape == (256, tc.G17_FRAMES[name]) and spec.shape == (257, tc.G17_FRAMES[name])
    uq, n = an.hashes_batch(torch.from_numpy(d).cuda()[None], shifts=1)
    np.testing.assert_array_equal(_rows(uq, n, 0), g[f"rows_{name}"])
    lm = an.peaks2landmarks(pklist)                                  # the reference's call surface, its list order
    assert len(lm) == int(g[f"n_landmarks_{name}"])
    np.testing.assert_array_equal(oh.unique_sorted_hashes(oh.landmarks2hashes(lm)), g[f"rows_{name}"])
    assert lm == [tuple(int(v) for v in r) for r in oh.peaks2landmarks([(int(c), int(b)) for c, b in pklist])]


# ------------------------------------------------------------------------------------------------ 3. the maximum
def test_the_maximum_length_equals_the_oracle_and_one_more_frame_raises():
    d = tc.noise(tc.samples(16384), seed=41)
    an = _analyzer()
    x = torch.from_numpy(d).cuda()[None]
    mask, npeaks, _ = an.find_peaks_batch(x, want_spec=False)
    uq, n = an.hashes_batch(x, shifts=1)
    want_mask, want_rows = _oracle(d)
    assert mask.shape == (1, 256, 16384) and int(npeaks[0]) == int(want_mask.sum()) > 5000
    assert np.array_equal(mask[0].cpu().numpy(), want_mask)
    np.testing.assert_array_equal(_rows(uq, n, 0), want_rows)
    assert int(want_rows[:, 0].max()) > 16000                        # times up to the last frames, below 2^14
    longer = torch.zeros((1, tc.samples(16385)), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="16384.*14 time bits"):
        an.find_peaks_batch(longer)
    with pytest.raises(ValueError, match="16384.*14 time bits"):
        an.hashes_batch(longer)


# ------------------------------------------------------------------------------------------------ 4. landmark capacity
@pytest.fixture(scope="module")
def dense():
    """(256, 2048): four peaks in every frame, all within pairing range of each other -- 3 landmarks per peak, > 8192 in total."""
    m = np.zeros((256, 2048), np.uint8)
    for t in range(2048):
        m[[40 + (t % 5), 50 + (t % 3), 60, 66 - (t % 4)], t] = 1
    return m


def _track_rows(mask_np, cap=None, **kw):
    ops = _ops()
    cap = cap if cap is not None else 3 * int(mask_np.sum())
    lm, hs, uq, counts = ops.audfprint_landmarks_track(torch.from_numpy(mask_np[None]).cuda(), cap, **kw)
    return lm, hs, uq, counts.cpu().numpy()[0]


def test_more_than_8192_landmarks_equal_the_oracle(dense):
    want_lm = oh.peaks2landmarks(oa.pklist_from_mask(dense))
    want = oh.audfprint_hashes_from_mask(dense)
    assert len(want_lm) > 8192 and len(want) == len(want_lm)
    lm, hs, uq, counts = _track_rows(dense, want_lists=True)
    assert counts.tolist() == [len(want_lm), len(want)]
    np.testing.assert_array_equal(uq[0, :counts[1]].cpu().numpy(), want)
    np.testing.assert_array_equal(lm[0, :counts[0]].cpu().numpy(), np.array(want_lm, np.int32))
    np.testing.assert_array_equal(hs[0, :counts[0]].cpu().numpy(), oh.landmarks2hashes(want_lm))
    # the capacity: one below the total overflows, the exact one succeeds
    assert _track_rows(dense, cap=len(want_lm) - 1)[3].tolist() == [-1, -1]
    _, _, uq, counts = _track_rows(dense, cap=len(want_lm))
    assert counts.tolist() == [len(want_lm), len(want)]
    np.testing.assert_array_equal(uq[0, :counts[1]].cpu().numpy(), want)


@pytest.mark.parametrize("frame", [300, 511, 512, 2047])
def test_eight_peaks_in_a_frame_pass_and_nine_are_flagged(dense, frame):
    """... wherever the frame lies: inside a tile, on either side of a seam, in the halo of the tile before it."""
    m8 = dense.copy()
    m8[:, frame] = 0
    m8[[30, 36, 42, 48, 54, 60, 66, 72], frame] = 1
    want = oh.audfprint_hashes_from_mask(m8)
    _, _, uq, counts = _track_rows(m8)
    assert counts[1] == len(want) and counts[0] == len(oh.peaks2landmarks(oa.pklist_from_mask(m8)))
    np.testing.assert_array_equal(uq[0, :counts[1]].cpu().numpy(), want)
    m9 = m8.copy()
    m9[78, frame] = 1
    assert _track_rows(m9)[3].tolist() == [-1, -1]


# ------------------------------------------------------------------------------------------------ 5. shifts
def test_four_shifts_equal_the_union_of_the_oracles_lists():
    d = tc.track_noise(tc.samples(1700), seed=9, noise_seed=10)
    an = _analyzer()
    an.shifts = 4
    uq, n = an.hashes_batch(torch.from_numpy(d).cuda()[None])
    lists = []
    for s in range(4):
        mask = oa.find_peaks(d[int(s / 4 * 256):])[1]
        lists.append(oh.landmarks2hashes(oh.peaks2landmarks(oa.pklist_from_mask(mask))))
    want = oh.unique_sorted_hashes(np.concatenate(lists))
    assert len(want) < sum(len(x) for x in lists)                    # the shifts share rows: the duplicate removal has work to do
    np.testing.assert_array_equal(_rows(uq, n, 0), want)


# ------------------------------------------------------------------------------------------------ 6. end to end
E2E_FRAMES = [1501, 1800, 3200, 2400, 1800, 2900]                    # two of equal length: one device batch


@pytest.fixture(scope="module")
def e2e():
    from musicfpaugment_amd.testing.audfprint_exps import create_fp_database_batch
    tracks = [tc.track_noise(tc.samples(f), seed=20 + i, noise_seed=40 + i) for i, f in enumerate(E2E_FRAMES)]
    names = ["whole%02d" % i for i in range(len(tracks))]
    ht = create_fp_database_batch(tracks, names, whole_tracks=True)
    rows = [_oracle(t)[1] for t in tracks]
    return dict(ht=ht, tracks=tracks, names=names, rows=rows)


def test_database_of_whole_tracks_equals_the_oracle(e2e):
    ht = e2e["ht"]
    table, counts = io_.empty_table()
    for i, r in enumerate(e2e["rows"]):
        io_.store(table, counts, r, i)
    assert ht.names == e2e["names"]
    np.testing.assert_array_equal(np.asarray(ht.hashesperid)[:len(e2e["rows"])], [len(r) for r in e2e["rows"]])
    np.testing.assert_array_equal(ht.counts.cpu().numpy(), counts)
    np.testing.assert_array_equal(ht.table.cpu().numpy().view(np.uint32), table)
    assert max(int(r[:, 0].max()) for r in e2e["rows"]) > 3000       # stored times far beyond a clip's


def test_queries_from_beyond_frame_1500_find_their_track_and_offset(e2e):
    """Twelve clean 8-s excerpts at frame-aligned offsets, two per track.  They start beyond frame 1500 wherever the track is long
    enough to hold 8 s there; the 1501-frame track's end at its last frames (beyond what a 1500-frame clip holds)."""
    from musicfpaugment_amd.afp.audfprint.audfprint_match import Matcher
    from musicfpaugment_amd.afp.audfprint.peak_extractor import Audfprint_peaks
    from musicfpaugment_amd.testing.audfprint_exps import compute_accuracy_batch
    ht, tracks = e2e["ht"], e2e["tracks"]
    owner, cut, q = [], [], []
    for i, f in enumerate(E2E_FRAMES):
        last = f - 1 - 250                                           # last frame an 8-s excerpt can start at
        for start in ((1501, last) if last > 1501 else (last - 150, last)):
            owner.append(i)
            cut.append(start)
            q.append(tracks[i][256 * start:256 * start + 64000])
    assert len(q) == 12 and all(len(x) == 64000 for x in q) and sum(c >= 1501 for c in cut) == 10
    queries = torch.from_numpy(np.stack(q))
    an = Audfprint_peaks(None)
    res, rows = compute_accuracy_batch(queries, owner, ht, an, an, per_query=True)
    assert rows[:, 0].tolist() == owner and rows[:, 2].tolist() == owner and res["No Denoising"] == 1.0
    uq, n = an.hashes_batch(queries.cuda().contiguous())
    got, info = Matcher().match_batch(ht, uq, n, k=64)
    got, info = got.cpu().numpy(), info.cpu().numpy()
    table, counts = ht.table.cpu().numpy().view(np.uint32), ht.counts.cpu().numpy()
    for i in range(12):
        assert info[i, 1] >= 1 and (int(got[i, 0, 0]), int(got[i, 0, 2])) == (owner[i], cut[i]), (i, got[i, 0].tolist())
        qrows = _rows(uq, n, i)
        want = io_.match(table, counts, ht.hashesperid, qrows)
        err = io_.rows_equivalent(got[i, :info[i, 1]], want, io_.rank_ties(table, counts, ht.hashesperid, qrows))
        assert err is None, (i, err)


def test_without_the_switch_a_long_clip_still_raises(e2e):
    from musicfpaugment_amd.afp.audfprint.peak_extractor import Audfprint_peaks
    from musicfpaugment_amd.testing.audfprint_exps import create_fp_database_batch
    x = torch.from_numpy(e2e["tracks"][0]).cuda()[None]
    assert x.shape[1] // 256 + 1 == 1501
    from musicfpaugment_amd._lib import MfpaError
    with pytest.raises((ValueError, MfpaError)):                     # as on the parent: the clip kernels refuse it
        Audfprint_peaks(None).hashes_batch(x)
    with pytest.raises(ValueError, match="1500"):
        create_fp_database_batch([e2e["tracks"][0]], ["long"])
    with pytest.raises(NotImplementedError):                         # a denoiser and a whole track
        from musicfpaugment_amd.training.unet import UNet
        from musicfpaugment_amd.training.weights import formula_state_dict
        net = UNet(1, 1)
        net.load_state_dict(formula_state_dict(0))
        Audfprint_peaks(None, denoising=True, denoising_model="unet", unet=net.cuda().eval(), whole_tracks=True).find_peaks_batch(x)
    short = _analyzer().hashes_batch(x[:, :64000].contiguous())      # the switch on, a clip: the clip kernels, the same rows
    want = Audfprint_peaks(None).hashes_batch(x[:, :64000].contiguous())
    assert torch.equal(short[0], want[0]) and torch.equal(short[1], want[1])


# ------------------------------------------------------------------------------------------------ 7. files
def test_file_entry_points_equal_the_batched_call(tmp_path):
    from scipy.io import wavfile
    from musicfpaugment_amd.afp.audfprint.hash_table import HashTable
    from musicfpaugment_amd.testing.audfprint_exps import create_fp_database, create_fp_database_batch
    d = tc.track_noise(70 * 8000, seed=33, noise_seed=34)            # 70 s: 2188 frames
    path = str(tmp_path / "seventy.wav")
    wavfile.write(path, 8000, d)
    an = _analyzer()
    uq, n = an.hashes_batch(torch.from_numpy(d).cuda()[None], shifts=1)
    want = _rows(uq, n, 0)
    np.testing.assert_array_equal(want, _oracle(d)[1])
    np.testing.assert_array_equal(an.wavfile2hashes(path), want)
    peaks = an.wavfile2peaks(path)
    assert peaks == oa.pklist_from_mask(_oracle(d)[0])
    ht = HashTable(device="cuda")
    dur, nh = an.ingest(ht, path)
    assert (dur, nh) == (70.0, len(want))
    batched = create_fp_database_batch([d], [path], whole_tracks=True)
    assert torch.equal(ht.table, batched.table) and torch.equal(ht.counts, batched.counts)
    db = str(tmp_path / "db.pklz")
    create_fp_database([path], db, whole_tracks=True)
    loaded = HashTable(db, device="cuda")
    assert loaded.names == [path] and torch.equal(loaded.table, batched.table) and torch.equal(loaded.counts, batched.counts)
    assert HashTable(device="cuda").counts.sum() == 0
    create_fp_database([path], str(tmp_path / "off.pklz"))           # the switch off: reported and skipped, as for any unreadable file
    assert int(HashTable(str(tmp_path / "off.pklz"), device="cuda").counts.sum()) == 0
