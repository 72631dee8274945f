"""CPU: the float64 restatements of tests/_transforms_oracle.py against golden g19 (the REAL _gen_noise of the reference, float32
on the CPU) and against the properties a band filter must have.  julius is in neither tree, so the band filter is property-tested
only: parity with julius is unpinned."""
import math

import numpy as np
import pytest

from tests import _transforms_oracle as to


@pytest.fixture(scope="module")
def g19(golden):
    return golden("g19_colored_noise")


def test_g19_holds_what_the_gpu_tests_rely_on(g19):
    assert g19["rates"].tolist() == [600, 1000, 8000] and g19["f_decay"].tolist() == [-2.0, 0.0, 1.0, 2.0]
    cases = list(to.g19_cases(g19))
    assert len(cases) == 24
    for sr, white, fd, T, y in cases:
        assert white.shape == (sr,) and white.dtype == np.float32 and y.shape == (T,) and y.dtype == np.float32
        assert T % sr != 0 and (T > sr or T < sr)


def test_colored_noise_oracle_reproduces_the_reference_to_float32_rounding(g19):
    """A float32 rfft and irfft of N points each put at most ~log2(N) roundings on an element, the mask (a powf and a division),
    the 1/N and the RMS division a handful more: |golden - oracle| <= (2 log2 N + 6) * 2^-24 * max|y|.  Measured on this
    fixture: 4.9e-7 ... 1.1e-6 absolute on unit-RMS signals, a tenth of the bound."""
    for sr, white, fd, T, y in to.g19_cases(g19):
        want = to.colored_noise(white, fd, T)
        err = np.abs(y.astype(np.float64) - want).max()
        bound = (2 * math.log2(sr) + 6) * 2.0 ** -24 * np.abs(want).max()
        assert err <= bound, (sr, fd, T, err, bound)
        assert abs(np.sqrt(np.mean(want[:min(T, sr)] ** 2)) - 1.0) < (1e-6 if T >= sr else 0.2)
    ref = to.reference_error(g19)
    assert set(ref) == {600, 1000, 8000} and all(1e-8 < e < 4e-6 for e in ref.values()), ref


def test_colored_noise_oracle_tiles_one_period_and_takes_a_batch():
    rng = np.random.default_rng(5)
    white = rng.standard_normal((3, 20)).astype(np.float32)
    fd = np.array([-1.0, 0.0, 2.0], dtype=np.float32)
    y = to.colored_noise(white, fd, 61)
    assert y.shape == (3, 61)
    assert np.array_equal(y[:, :20], y[:, 20:40]) and np.array_equal(y[:, 0], y[:, 60])
    for b in range(3):
        assert np.array_equal(y[b], to.colored_noise(white[b], fd[b], 61))
    flat = to.colored_noise(white[1], 0.0, 20)                                   # f_decay 0: the white noise itself, unit RMS
    w = white[1].astype(np.float64)
    assert np.allclose(flat, w / (np.sqrt(np.mean(w * w)) + 1e-8), atol=1e-13)


@pytest.mark.parametrize("lo,hi", [(0.02, 0.3), (0.1, 0.5), (1.25e-4, 0.2), (0.249, 0.251)])
def test_band_taps_sum_to_zero_and_each_low_pass_to_one(lo, hi):
    half = to.band_half(lo)
    assert half == int(8 / lo / 2)
    tl, th = to.lowpass_taps_on(lo, half), to.lowpass_taps_on(hi, half)
    assert len(tl) == len(th) == 2 * half + 1
    assert abs(tl.sum() - 1.0) < 1e-12 and abs(th.sum() - 1.0) < 1e-12
    taps = to.bandpass_taps(lo, hi)
    assert abs(taps.sum()) < 1e-12 and np.allclose(taps, taps[::-1], atol=1e-15)


def test_band_filter_passes_its_band_and_stops_the_rest():
    t = np.arange(4000, dtype=np.float64)
    inside, below, above = (np.sin(2 * np.pi * f * t) for f in (0.15, 0.02, 0.4))
    mid = slice(500, 3500)                                                       # away from the replicate-padded edges
    bp = lambda x: to.bandpass(x, 0.1, 0.2)
    assert np.abs(bp(inside) - inside)[mid].max() < 0.01
    assert np.abs(bp(below))[mid].max() < 0.01 and np.abs(bp(above))[mid].max() < 0.01
    assert np.abs(bp(np.full(4000, 0.7))).max() < 1e-12                          # zero DC gain, edges included
    x = inside + below
    assert np.allclose(to.bandstop(x, 0.1, 0.2) + to.bandpass(x, 0.1, 0.2), x, atol=1e-15)
    assert np.abs(to.bandstop(x, 0.1, 0.2) - below)[mid].max() < 0.02


def test_band_above_half_the_rate_is_refused():
    with pytest.raises(ValueError, match="A cutoff above 0.5 does not make sense."):
        to.bandpass_taps(0.3, 0.51)
