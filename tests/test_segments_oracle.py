"""CPU: the numpy restatement of the segment stage (tests/_segments_oracle.py) on hand-laid cases, and two conditions on the
inputs the GPU tests use: no segment so close to the silence threshold that a summation order could decide it, and the
reference's float32 formula agreeing with the float64 rule wherever a segment is at least 1 % away."""
import math

import numpy as np
import pytest

from tests import _segments_oracle as so


def test_frame_samples_are_the_references_float32_products():
    assert so.frame_samples(3.0, 1.0, 8000) == (24000, 24000)
    assert so.frame_samples(3.0, 0.5, 8000) == (24000, 12000)
    assert so.frame_samples(8, 1.0, 8000) == (64000, 64000)
    assert so.frame_samples(0.003, 1.0, 8000) == (int(np.float32(0.003) * np.float32(8000)),) * 2


@pytest.mark.parametrize("N,L,S,want", [(0, 4, 4, 0), (3, 4, 4, 0), (4, 4, 4, 1), (7, 4, 4, 1), (8, 4, 4, 2), (9, 4, 2, 3), (10, 4, 2, 4),
                                        (10, 4, 7, 1), (11, 4, 7, 2), (8195, 4, 1, 8192)])
def test_frame_counts_without_end_padding(N, L, S, want):
    assert so.n_frames(N, L, S) == want


def test_geometry_prefix_and_refusals():
    assert so.geometry([0, 3, 4, 9, 8], 4, 4).tolist() == [0, 0, 0, 1, 3, 5]
    assert so.geometry([], 4, 4).tolist() == [0]
    assert so.geometry([8196], 4, 1) is None and so.geometry([8195], 4, 1).tolist() == [0, 8192]
    assert so.geometry([4], 0, 1) is None and so.geometry([4], 1, 0) is None and so.geometry([-1], 4, 4) is None


def test_hand_laid_track():
    """Eight samples, L = S = 4: segments [1, 1, 1, 1] and [0.1, 0, 0, 0.1]; the whole-track mean square is (4 + 0.02) / 8."""
    x = np.array([1, -1, 1, -1, 0.1, 0, 0, -0.1, 3], dtype=np.float32)       # the ninth sample is the tail: it counts in the reference
    seg, trk, peak = so.stats(x, 4, 4)
    t = np.float32(0.1).astype(np.float64) ** 2
    assert seg.tolist() == [4.0, 2 * t] and trk == math.fsum([13.0, t, t]) and peak == np.float32(3)
    assert so.keep(seg, trk, len(x), 4).tolist() == [True, False]
    assert so.keep_tf32(x, 4, 4).tolist() == [True, False]
    # 10 ln(rms_seg / rms_ref) > dbs  <=>  seg / L > exp(dbs / 5) * trk / N
    for dbs in (-7.5, 0.0, -60.0, 3.0):
        want = 10 * np.log(np.sqrt(seg / 4) / np.sqrt(trk / len(x))) > dbs
        assert so.keep(seg, trk, len(x), 4, dbs).tolist() == want.tolist(), dbs


def test_an_all_zero_track_keeps_nothing_and_a_silent_segment_is_dropped():
    z = np.zeros(12, dtype=np.float32)
    seg, trk, peak = so.stats(z, 4, 4)
    assert not so.keep(seg, trk, 12, 4).any() and not so.keep_tf32(z, 4, 4).any() and peak == 0
    x = np.array([1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1], dtype=np.float32)
    assert so.keep(*so.stats(x, 4, 4)[:2], 12, 4).tolist() == [True, False, True]
    assert np.array_equal(so.divide(z, peak), z)                          # the peak of zeros divides nothing


def test_selection_orders_by_key_then_index():
    mask = np.array([True, False, True, True, True])
    keys = np.array([7, 0, 7, 3, 2 ** 32 - 1], dtype=np.uint32)
    assert so.select(mask, keys, 2).tolist() == [3, 0]
    assert so.select(mask, keys, 6).tolist() == [3, 0, 2, 4, -1, -1]        # equal keys: the lower index first; silent ones never
    assert so.select(np.zeros(3, dtype=bool), keys[:3], 2).tolist() == [-1, -1]


def test_division_is_float32():
    x = np.array([1, 3, -7], dtype=np.float32)
    got = so.divide(x, np.float32(7))
    assert got.dtype == np.float32 and got.tolist() == [np.float32(1) / np.float32(7), np.float32(3) / np.float32(7), -1.0]
    assert got[0] != np.float32(1) * (np.float32(1) / np.float32(7)) or got[1] != np.float32(3) * (np.float32(1) / np.float32(7))
    assert np.array_equal(so.divide(x, np.float32(7), do_norm=False), x)


def _conditions(tracks, L, S):
    total = near = 0
    for t in tracks:
        seg, trk, _ = so.stats(t, L, S)
        if len(seg) == 0:
            continue
        m = so.margin(seg, trk, len(t), L)
        assert np.all(m >= 1e-6), (L, S, len(t), float(m.min()))
        k64, k32 = so.keep(seg, trk, len(t), L), so.keep_tf32(t, L, S)
        far = m >= 1e-2
        assert np.array_equal(k64[far], k32[far]), (L, S, len(t))
        total += len(seg)
        near += int((~far).sum())
    return total, near


@pytest.mark.parametrize("shape", so.GPU_SHAPES, ids=str)
def test_gpu_inputs_are_decided_by_margins_no_summation_order_reaches(shape):
    """Every segment of the GPU tests' tracks lies at least 1e-6 (relative) from the threshold -- the device's sums are within
    (n - 1) * 2^-53 < 3e-12 of the exact ones -- and wherever it lies 1e-2 away the float32 formula gives the same answer."""
    L, S = shape
    tracks = so.gpu_tracks(L, S)
    total, _ = _conditions(tracks, L, S)
    assert total >= 8
    masks = np.concatenate([so.keep(*so.stats(t, L, S)[:2], len(t), L) for t in tracks])
    assert masks.any() and not masks.all()                                # both sides of the threshold


def test_the_long_track_too():
    t = so.long_track()
    assert so.n_frames(len(t), 4, 1) == so.MAX_PER_TRACK
    total, _ = _conditions([t], 4, 1)
    assert total == so.MAX_PER_TRACK


def test_two_hundred_random_tracks():
    rng = np.random.default_rng(7)
    tracks, total, near = [], 0, 0
    for _ in range(200):
        L = int(rng.integers(16, 64))
        t = so.make_track(rng, int(rng.integers(0, 12 * L)), L, L)
        a, b = _conditions([t], L, L)
        total, near = total + a, near + b
    print("segments", total, "inside 1 %", near)
    assert total > 900
