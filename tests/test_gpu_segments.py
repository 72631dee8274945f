"""GPU: the segment kernels (csrc/segments.hip) against the numpy restatement (tests/_segments_oracle.py): sums and peaks, the
keep rule and the (key, index) selection, the float32 division of the gather, and the bit-for-bit independence of a track's
outputs from its batch and its place in the bank.  tests/test_segments_oracle.py holds the conditions on these inputs that make
the mask comparable (no segment within 1e-6 of the threshold)."""
import numpy as np
import pytest
import torch

from tests import _segments_oracle as so

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture(scope="module")
def ops():
    from musicfpaugment_amd import ops as _ops
    return _ops


def _bank(tracks, lead=1, gap=3):
    """Tracks back to back behind `lead` foreign floats and `gap` between them (NaN: a kernel that reads past a track sees it):
    with the default 1 / 3 the tracks start at odd and even offsets, none 16-byte aligned as a rule."""
    off, parts, pos = [], [np.full(lead, np.nan, dtype=np.float32)], lead
    for t in tracks:
        off.append(pos)
        parts += [t, np.full(gap, np.nan, dtype=np.float32)]
        pos += len(t) + gap
    return np.concatenate(parts), np.array(off, dtype=np.int64), np.array([len(t) for t in tracks], dtype=np.int64)


def _device(ops, tracks, L, S, **kw):
    bank, off, lens = _bank(tracks, **kw)
    seg_off = ops.segment_geometry(lens, L, S)
    d = dict(bank=torch.from_numpy(bank).cuda(), off=torch.from_numpy(off).cuda(), lens=torch.from_numpy(lens).cuda(),
             seg_off=torch.from_numpy(seg_off).cuda(), ns=int(seg_off[-1]), seg_off_h=seg_off, off_h=off, bank_h=bank)
    d["stats"] = ops.segment_stats(d["bank"], d["off"], d["lens"], d["seg_off"], d["ns"], L, S)
    return d


_ORACLE = {}


def _oracle(L, S):
    """(tracks, [stats per track]) of one shape, computed once for the tests that need it."""
    if (L, S) not in _ORACLE:
        tracks = so.gpu_tracks(L, S)
        _ORACLE[(L, S)] = (tracks, [so.stats(t, L, S) for t in tracks])
    return _ORACLE[(L, S)]


def _keys(ns, seed=5):
    k = np.random.default_rng(seed).integers(0, 1 << 32, size=ns, dtype=np.uint32)
    if ns >= 4:
        k[: ns // 2] = k[0]                                              # key ties: broken by index
    return k


@pytest.mark.parametrize("shape", so.GPU_SHAPES, ids=str)
def test_sums_and_peaks_against_the_oracle(ops, shape):
    """trk_peak exactly; every sum within (n - 1) * 2^-53 relative of the exact one: a float32 square is exact in float64 and each
    of the n - 1 additions rounds once (derived, not measured)."""
    L, S = shape
    tracks, want = _oracle(L, S)
    d = _device(ops, tracks, L, S)
    seg, trk, peak = (t.cpu().numpy() for t in d["stats"])
    assert seg.dtype == np.float64 and trk.dtype == np.float64 and peak.dtype == np.float32
    worst = 0.0
    for i, (t, (wseg, wtrk, wpeak)) in enumerate(zip(tracks, want)):
        a, b = d["seg_off_h"][i], d["seg_off_h"][i + 1]
        assert b - a == len(wseg)
        assert peak[i] == wpeak, i
        assert abs(trk[i] - wtrk) <= max(len(t) - 1, 0) * U * wtrk, (i, trk[i], wtrk)
        assert np.all(np.abs(seg[a:b] - wseg) <= (L - 1) * U * wseg), i
        if wtrk > 0:
            worst = max(worst, abs(trk[i] - wtrk) / (max(len(t) - 1, 1) * U * wtrk))
    print(shape, "largest track-sum error / bound:", worst)
    assert len(tracks[0]) == 0 and seg.shape == (d["ns"],) and trk[0] == 0 and peak[0] == 0      # the empty track: 0 / 0 / 0


@pytest.mark.parametrize("n_keep", [1, 2, 16])
@pytest.mark.parametrize("shape", so.GPU_SHAPES, ids=str)
def test_selection_against_the_oracle(ops, shape, n_keep):
    """mask, kept and sel equal the oracle's on exact sums AND the oracle's on the device's own sums; n_keep below and above the
    kept counts (0 .. 8 per track here, tests/_segments_oracle.gpu_tracks)."""
    L, S = shape
    tracks, _ = _oracle(L, S)
    d = _device(ops, tracks, L, S)
    keys = _keys(d["ns"])
    sel, src, div, kept, mask = ops.segment_select(*d["stats"], d["off"], d["lens"], d["seg_off"], L, S, torch.from_numpy(keys.view(np.int32)).cuda(),
                                                   so.DBS, n_keep, True, with_mask=True)
    wmask, wkept, wsel = so.select_all(tracks, L, S, keys, n_keep)
    sums = (d["stats"][0].cpu().numpy(), d["stats"][1].cpu().numpy())
    dmask, dkept, dsel = so.select_all(tracks, L, S, keys, n_keep, sums=sums)
    for got, a, b in ((mask.cpu().numpy() != 0, wmask, dmask), (kept.cpu().numpy(), wkept, dkept), (sel.cpu().numpy(), wsel, dsel)):
        assert np.array_equal(got, a) and np.array_equal(got, b)
    assert kept.dtype == torch.int32 and sel.dtype == torch.int32 and src.dtype == torch.int64
    assert (wkept > 1).any() if n_keep == 1 else (wkept < 16).all()      # the cut to n_keep bites / pads
    assert wkept.min() == 0 and (wkept > 0).any()
    # src: the start sample in the bank; div: the track's peak, 1 for the all-zero track
    sel_h, src_h, div_h = sel.cpu().numpy(), src.cpu().numpy(), div.cpu().numpy()
    peaks = d["stats"][2].cpu().numpy()
    for r in range(len(sel_h)):
        i = r // n_keep
        assert div_h[r] == (peaks[i] if peaks[i] > 0 else 1.0)
        if sel_h[r] < 0:
            assert src_h[r] == -1
        else:
            assert d["seg_off_h"][i] <= sel_h[r] < d["seg_off_h"][i + 1]
            assert src_h[r] == d["off_h"][i] + (sel_h[r] - d["seg_off_h"][i]) * S
    _, _, div1, _ = ops.segment_select(*d["stats"], d["off"], d["lens"], d["seg_off"], L, S, torch.from_numpy(keys.view(np.int32)).cuda(),
                                       so.DBS, n_keep, False)
    assert bool((div1 == 1).all())                                       # do_norm off


def test_key_ties_are_broken_by_index(ops):
    L = S = 4
    t = np.tile(np.array([1, -1, 1, -1], dtype=np.float32), 9)           # nine equal loud segments
    t[8:12] = 0                                                          # ... but the third
    d = _device(ops, [t], L, S)
    keys = np.array([5, 5, 0, 5, 1, 5, 5, 1, 5], dtype=np.uint32)
    sel, _, _, kept = ops.segment_select(*d["stats"], d["off"], d["lens"], d["seg_off"], L, S, torch.from_numpy(keys.view(np.int32)).cuda(),
                                         so.DBS, 10)
    assert int(kept[0]) == 8 and sel.cpu().tolist() == [4, 7, 0, 1, 3, 5, 6, 8, -1, -1]
    big = np.full(9, 2 ** 32 - 1, dtype=np.uint32)                       # the largest key is a key, not the padding
    sel, _, _, kept = ops.segment_select(*d["stats"], d["off"], d["lens"], d["seg_off"], L, S, torch.from_numpy(big.view(np.int32)).cuda(),
                                         so.DBS, 9)
    assert sel.cpu().tolist() == [0, 1, 3, 4, 5, 6, 7, 8, -1]


def test_a_track_of_8192_segments(ops):
    L, S = 4, 1
    t = so.long_track()
    d = _device(ops, [t], L, S)
    assert d["ns"] == so.MAX_PER_TRACK
    wseg, wtrk, wpeak = so.stats(t, L, S)
    seg, trk, peak = (x.cpu().numpy() for x in d["stats"])
    assert peak[0] == wpeak and abs(trk[0] - wtrk) <= (len(t) - 1) * U * wtrk and np.all(np.abs(seg - wseg) <= 3 * U * wseg)
    keys = np.random.default_rng(9).integers(0, 1 << 32, size=d["ns"], dtype=np.uint32)
    sel, _, _, kept, mask = ops.segment_select(*d["stats"], d["off"], d["lens"], d["seg_off"], L, S, torch.from_numpy(keys.view(np.int32)).cuda(),
                                               so.DBS, 8192, True, with_mask=True)
    wmask, wkept, wsel = so.select_all([t], L, S, keys, 8192)
    assert np.array_equal(mask.cpu().numpy() != 0, wmask) and int(kept[0]) == int(wkept[0]) and np.array_equal(sel.cpu().numpy(), wsel)
    with pytest.raises(ValueError):
        ops.segment_geometry([len(t) + 1], L, S)                         # one segment more is refused


@pytest.mark.parametrize("shape", so.GPU_SHAPES, ids=str)
def test_gather_divides_in_float32_and_touches_nothing_else(ops, shape):
    L, S = shape
    tracks, want = _oracle(L, S)
    d = _device(ops, tracks, L, S)
    keys = _keys(d["ns"], 6)
    n_keep = 3
    sel, src, div, kept = ops.segment_select(*d["stats"], d["off"], d["lens"], d["seg_off"], L, S, torch.from_numpy(keys.view(np.int32)).cuda(),
                                             so.DBS, n_keep)
    ldo = L + 5
    buf = torch.full((len(tracks) * n_keep, ldo), float("nan"), device="cuda")
    out = ops.segment_gather(d["bank"], src, div, L, out=buf[:, :L])
    assert out.data_ptr() == buf.data_ptr()
    got, sel_h = buf.cpu().numpy(), sel.cpu().numpy()
    assert np.isnan(got[:, L:]).all()                                    # the padding between rows
    hit = 0
    for r in range(len(sel_h)):
        i = r // n_keep
        if sel_h[r] < 0:
            assert np.isnan(got[r]).all()                                # rows without a segment are left alone
            continue
        j = sel_h[r] - d["seg_off_h"][i]
        ref = so.divide(tracks[i][j * S: j * S + L], want[i][2])
        assert np.array_equal(got[r, :L].view(np.uint32), ref.view(np.uint32)), (r, i, j)
        hit += 1
    assert hit >= 4
    # without `div`: a copy, from any alignment of src
    src2 = torch.from_numpy(d["off_h"][-1] + np.arange(4, dtype=np.int64)).cuda()
    cp = ops.segment_gather(d["bank"], src2, None, L).cpu().numpy()
    for k in range(4):
        assert np.array_equal(cp[k].view(np.uint32), tracks[-1][k: k + L].view(np.uint32))


@pytest.mark.parametrize("shape", [(24, 24), (23, 23), (24, 8), (24000, 24000)], ids=str)
def test_a_tracks_outputs_do_not_depend_on_its_batch_or_its_place(ops, shape):
    """Bit for bit: alone, inside a batch, and at four other alignments in the bank."""
    L, S = shape
    tracks, _ = _oracle(L, S)
    d = _device(ops, tracks, L, S)
    seg, trk, peak = (t.cpu().numpy() for t in d["stats"])
    for i in (3, 5, 7):
        a, b = d["seg_off_h"][i], d["seg_off_h"][i + 1]
        for lead in (0, 1, 2, 3, 6):
            one = _device(ops, [tracks[i]], L, S, lead=lead)
            s1, t1, p1 = (t.cpu().numpy() for t in one["stats"])
            assert np.array_equal(s1.view(np.uint64), seg[a:b].view(np.uint64)), (i, lead)
            assert t1.view(np.uint64)[0] == trk.view(np.uint64)[i] and p1[0] == peak[i], (i, lead)


def test_empty_calls(ops):
    z64 = torch.zeros(0, dtype=torch.int64, device="cuda")
    seg_off = torch.zeros(1, dtype=torch.int32, device="cuda")
    seg, trk, peak = ops.segment_stats(torch.zeros(8, device="cuda"), z64, z64, seg_off, 0, 4, 4)
    assert seg.shape == (0,) and trk.shape == (0,) and peak.shape == (0,)
    assert ops.segment_gather(torch.zeros(8, device="cuda"), z64, None, 4).shape == (0, 4)
    # tracks, but not one segment
    d = _device(ops, [np.ones(3, dtype=np.float32), np.zeros(0, dtype=np.float32)], 4, 4)
    assert d["ns"] == 0 and d["stats"][1].cpu().tolist() == [3.0, 0.0] and d["stats"][2].cpu().tolist() == [1.0, 0.0]
    sel, src, div, kept = ops.segment_select(*d["stats"], d["off"], d["lens"], d["seg_off"], 4, 4, torch.zeros(0, dtype=torch.int32, device="cuda"),
                                             so.DBS, 2)
    assert sel.cpu().tolist() == [-1] * 4 and src.cpu().tolist() == [-1] * 4 and kept.cpu().tolist() == [0, 0]
