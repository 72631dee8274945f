"""CPU: the oracle (oracle.audfprint.find_peaks + oracle.hashes) reproduces the REFERENCE's peak lists and hash rows on inputs
longer than the clip kernels take (tests/golden/g17_track.npz, written by tools/make_track_goldens.py: 2041 and 1501 frames).
This pins the oracle at these lengths before the device's track kernels are compared with it (tests/test_gpu_track.py)."""
import os

import numpy as np
import pytest

from musicfpaugment_amd import synth
from oracle import audfprint as oa
from oracle import hashes as oh
from tests import _track_cases as tc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g17_track.npz")


@pytest.fixture(scope="module")
def g17():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def inputs():
    return tc.g17_inputs()


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_inputs_are_the_recorded_ones(g17, inputs, name):
    d = inputs[name]
    assert d.dtype == np.float32 and len(d) == int(g17[f"n_samples_{name}"])
    assert 1 + len(d) // 256 == tc.G17_FRAMES[name]
    assert synth.digest(d) == str(g17[f"digest_{name}"])


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_oracle_reproduces_the_reference_on_long_inputs(g17, inputs, name):
    pklist, mask, _ = oa.find_peaks(inputs[name])
    assert mask.shape == (256, tc.G17_FRAMES[name])
    np.testing.assert_array_equal(np.array(pklist, np.int64).reshape(-1, 2), g17[f"pklist_{name}"].astype(np.int64))
    landmarks = oh.peaks2landmarks(pklist)
    assert len(landmarks) == int(g17[f"n_landmarks_{name}"])
    np.testing.assert_array_equal(oh.unique_sorted_hashes(oh.landmarks2hashes(landmarks)), g17[f"rows_{name}"])
    np.testing.assert_array_equal(oh.audfprint_hashes_from_mask(mask), g17[f"rows_{name}"])


def test_the_inputs_exercise_what_they_are_for(g17):
    """(a) is past 64 chunks of np.mean's reduction and holds more landmarks than one 256-frame tile can take from one frame range;
    (b) has a silent stretch of more than 1000 frames with no peak in it; (c) is the first length past the LDS pruner."""
    assert 257 * tc.G17_FRAMES["a"] > 64 * 8192 >= 257 * 2040
    pa, pb = g17["pklist_a"], g17["pklist_b"]
    assert len(pa) > 1000 and int(np.bincount(pa[:, 0]).max()) >= 4
    inside = (pb[:, 0] > 610) & (pb[:, 0] < 1690)
    assert not inside.any() and (pb[:, 0] >= 1700).any() and (pb[:, 0] < 600).any()
    assert tc.G17_FRAMES["c"] == 1501 and len(g17["pklist_c"]) > 300
