"""CPU: the oracle of the lossy-coding kernels (tests/_codec_oracle.py) against itself: the properties the definition of
include/mfpa.h promises, and the margin condition that makes the GPU comparisons of tests/test_gpu_codec.py well posed."""
import math
import os
import re

import numpy as np
import pytest

from tests import _codec_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mfpa.h")).read()
G = int(re.search(r"#define MFPA_CODEC_FRAMES (\d+)", HEADER).group(1))


def test_constants_agree_with_the_header_and_the_python_layer():
    from musicfpaugment_amd import ops
    assert G == ops.CODEC_FRAMES and (G + 1) * 8 == 256
    assert int(re.search(r"#define MFPA_CODEC_MAX_BANDS (\d+)", HEADER).group(1)) == ops.CODEC_MAX_BANDS == 32
    assert tuple(ops.CODEC_BAND_EDGES) == co.DEFAULT_EDGES and len(co.DEFAULT_EDGES) == 20
    assert np.array_equal(ops.codec_band_edges(), np.array(co.DEFAULT_EDGES, dtype=np.int32))
    for mode, name in enumerate(("ENCODE", "DECODE", "ROUNDTRIP")):
        assert int(re.search(rf"#define MFPA_MULAW_{name} (\d+)", HEADER).group(1)) == mode == getattr(ops, f"MULAW_{name}")
    assert [ops.codec_frames(T) for T in (1, 256, 257, 513)] == [co.n_frames(T) for T in (1, 256, 257, 513)] == [2, 2, 3, 4]
    for k in co.RATES + (math.inf,):
        assert ops.codec_bit_budget(k) == co.budget(k)
    assert co.budget(8.0) == 8000.0 * 256.0 / 8000.0 - 6 * 19


def test_the_cosine_table_is_the_mdct_kernel():
    w, C = co._tables(np.float64)
    n, k = np.arange(co.N)[:, None], np.arange(co.M)[None, :]
    assert np.max(np.abs(C - np.cos(np.pi / co.M * (n + 0.5 + co.M / 2) * (k + 0.5)))) < 1e-12      # the plain formula's argument error
    assert np.max(np.abs(w - np.sin(np.pi * (np.arange(co.N) + 0.5) / co.N))) == 0.0
    wl, Cl = co._tables(np.longdouble)
    assert np.max(np.abs(Cl - C)) <= 2.0 ** -54 and np.max(np.abs(wl - w)) <= 4e-16        # one rounding; numpy's sine of a rounded argument
    assert np.max(np.abs(wl[:co.M] ** 2 + wl[co.M:] ** 2 - 1)) < 1e-18                                # Princen-Bradley


@pytest.mark.parametrize("T", co.lengths(G))
def test_lossless_reconstructs_the_input(T):
    x = co.two_tones(T)
    y, lam, coded = co.reference(x, math.inf)
    t = co.truth(x, math.inf)[0]
    E = float(np.max(np.abs(y - t)))
    print(f"T={T}: |y - x| = {np.max(np.abs(y - x)):.3g}, E = {E:.3g}, |truth - x| = {float(np.max(np.abs(t - x))):.3g}")
    assert float(np.max(np.abs(t - x))) < 1e-17                  # the TDAC identity, to the long double's own rounding
    assert np.max(np.abs(y - x)) <= 4.0 * E                      # so the float64 definition is within a few E of the input
    assert np.all(np.isneginf(lam)) and not coded.any() and lam.shape == (co.n_frames(T),)


def test_snr_rises_with_the_rate():
    x = co.two_tones(4097)
    snr = [co.snr_db(x, co.reference(x, co.budget(k))[0]) for k in co.RATES]
    print("SNR dB at", co.RATES, "kbit/s:", [round(s, 2) for s in snr])
    assert all(b > a + 1.0 for a, b in zip(snr, snr[1:])) and 6.0 < snr[0] < 10.0 and snr[-1] > 40.0


def test_no_budget_and_silence_give_exact_zeros():
    x = co.two_tones(1000)
    for R in (co.budget(0.0), -1.0, -math.inf):
        y, lam, coded = co.reference(x, R)
        assert not y.any() and np.all(np.isnan(lam)) and not coded.any()
    for R in (co.budget(16.0), math.inf):
        y, lam, coded = co.reference(co.silence(700), R)
        assert not y.any() and not coded.any() and not np.any(np.isnan(y))
    both = np.stack([co.two_tones(700), co.silence(700)])
    y, lam, coded = co.reference(both, co.budget(16.0))
    assert y[0].any() and not y[1].any() and np.all(np.isnan(lam[1])) and not np.any(np.isnan(y))


def test_a_coded_band_carries_noise_of_the_allocated_power_and_the_rest_is_zero():
    x = co.two_tones(2048)
    y, lam, coded = co.reference(x, co.budget(8.0))
    assert np.all(coded[1:-1] > 0) and np.all(coded <= co.M) and np.all(np.isfinite(lam[1:-1])) and np.all(lam[1:-1] < 0)
    lam64 = co.reference(x, co.budget(64.0))[1]
    assert np.all(lam64[1:-1] < lam[1:-1])                       # more bits: a lower water line


def test_margin_condition_of_every_gpu_case():
    """Every discrete decision of every coded case the GPU tests run lies at least MARGIN from its threshold."""
    worst = math.inf
    for name, x, kbps in (c for T in co.lengths(G) for c in co.coded_cases(T)):
        R = co.budget(kbps)
        m = min(co.decision_margin(row, r) for row, r in zip(np.atleast_2d(x), np.broadcast_to(R, (np.atleast_2d(x).shape[0],))))
        worst = min(worst, m)
        assert m >= co.MARGIN, f"{name}: a decision {m:.3g} from its threshold: change the case's seed"
    print(f"smallest decision margin over the coded cases: {worst:.3g}")


@pytest.mark.parametrize("T,channels", co.MULAW_CASES)
def test_mulaw_oracle_and_its_margin(T, channels):
    x = co.mulaw_signal(T)
    codes = co.mulaw_encode(x, channels)
    assert codes.min() >= 0 and codes.max() <= channels - 1
    assert np.array_equal(codes, co.mulaw_encode(x, channels, np.longdouble))
    assert co.mulaw_margin(x, channels) >= co.MARGIN
    y = co.mulaw_decode(codes, channels)
    assert np.max(np.abs(y)) <= 1.0 and np.max(np.abs(y - co.mulaw_decode(codes, channels, np.longdouble))) < 1e-15
    if channels >= 256:                                          # half a step 1 / mu of c times dy/dc = ln(1 + mu) (abs(y) + 1 / mu), and its growth over the step
        inside = np.abs(x) <= 1.0
        assert np.max(np.abs(y - x)[inside]) <= np.log1p(channels - 1.0) / (channels - 1.0) * (1.0 / (channels - 1.0) + np.max(np.abs(x[inside]))) * (1.0 + 2.0 * np.log1p(channels - 1.0) / (channels - 1.0))
    if T >= 3:
        assert codes[0] == channels // 2 and codes[1] == channels - 1 and codes[2] == 0
