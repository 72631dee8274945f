"""CPU: the numpy restatement of the shoebox image-source response (tests/_rir_oracle.py) against the properties its definition
implies.  It must hold here before the kernel is compared with it on the GPU (tests/test_gpu_rir.py)."""
import math

import numpy as np
import pytest

from tests import _rir_oracle as ro

needs_longdouble = pytest.mark.skipif(not ro.HAVE_LONGDOUBLE, reason="np.longdouble is no wider than float64 here: no error unit")


def test_image_counts():
    for N, want in ((0, 1), (1, 7), (2, 25), (7, 575), (17, 7175)):
        assert ro.image_count(N) == want
        amp, tau = ro.images(ro.ROOM, ro.SOURCE, ro.MIC, ro.ALPHA, N, 8000)
        assert len(amp) == len(tau) == want
    assert [ro.image_count(N) for N in (16, 32, 47)] == [6017, 45825, 142975]


def test_order_zero_is_one_windowed_sinc():
    fs, c, half = 8000, 343.0, 40
    d = math.sqrt(sum((s - m) ** 2 for s, m in zip(ro.SOURCE, ro.MIC)))
    tau = d * fs / c
    h = ro.rir(**ro.case(0, 256))
    k = np.arange(256)
    x = k - tau
    want = np.where(np.abs(x) <= half, 0.5 * (1 + np.cos(np.pi * x / half)) * np.sinc(x), 0.0) / (4 * np.pi * d)
    np.testing.assert_allclose(h, want, rtol=0, atol=1e-15)
    assert abs(np.argmax(np.abs(h)) - tau) <= 0.5 and 0.8 / (4 * np.pi * d) < h.max() <= 1 / (4 * np.pi * d)
    assert np.count_nonzero(h) == 80                                 # the integers within 40 of a fractional tau, and nothing else


def test_fully_absorbing_walls_leave_the_direct_path():
    for N in (1, 7):
        assert np.array_equal(ro.rir(**ro.case(N, 512, absorption=1.0)), ro.rir(**ro.case(0, 512)))


@needs_longdouble
def test_error_unit_and_reciprocity():
    """Swapping source and microphone leaves every image's distance and gain as they were up to rounding: the response changes
    by the summation's rounding only."""
    case = ro.case(7, 2048)
    E = ro.error_unit(case)
    h = ro.rir(**case)
    swapped = ro.rir(**ro.case(7, 2048, source=ro.MIC, mic=ro.SOURCE))
    D = float(np.max(np.abs(h - swapped)))
    print(f"order 7, length 2048: peak {np.max(np.abs(h)):.4f}  E = {E:.3e}  swap = {D:.3e} = {D / E:.2f} E")
    assert 0 < E < 1e-13 and D <= ro.BOUND * E


def test_integer_delay_is_finite():
    """Source (1, 1, 1), microphone (1.5, 1, 1), c = 250 m/s at 8 kHz: d = 0.5 m and tau = 16 exactly; the tap at 16 is amp, its
    neighbours inside the window vanish with sin(pi j)."""
    case = ro.case(0, 128, source=(1.0, 1.0, 1.0), mic=(1.5, 1.0, 1.0), c=250.0)
    amp, tau = ro.images(case["room"], case["source"], case["mic"], case["absorption"], 0, 8000, 250.0)
    assert tau[0] == 16.0
    h = ro.rir(**case)
    assert np.all(np.isfinite(h)) and h[16] == amp[0] == 1 / (4 * np.pi * 0.5)
    assert np.max(np.abs(np.delete(h, 16))) < 1e-15


def test_decay_time_grows_with_the_target():
    """Room (3.0, 2.5, 2.2) m at 8 kHz, Eyring targets 0.1, 0.2, 0.3 s at orders 16, 32, 47: the measured decay (3 x the -5 ... -25 dB
    span of the Schroeder curve of the response cut at rt60) is longer than the target and strictly increasing."""
    room, src, mic, fs = (3.0, 2.5, 2.2), (1.1, 0.9, 1.2), (2.2, 1.7, 0.8), 8000
    got = []
    for rt60 in (0.1, 0.2, 0.3):
        N = math.ceil(343.0 * rt60 / min(room))
        h = ro.rir(room, src, mic, ro.eyring_absorption(room, rt60), N, int(math.ceil(rt60 * fs)), fs)
        got.append(ro.decay_time(h, fs))
    print("orders", [math.ceil(343.0 * t / 2.2) for t in (0.1, 0.2, 0.3)], "decay times", [round(g, 3) for g in got])
    assert [math.ceil(343.0 * t / 2.2) for t in (0.1, 0.2, 0.3)] == [16, 32, 47]
    assert got[0] < got[1] < got[2] and all(g > t for g, t in zip(got, (0.1, 0.2, 0.3)))
