"""CPU: the float64 restatement of torchaudio's Resample (tests/_resample_oracle.py) that the device kernel is checked against --
its geometry on the specified table, its float32 summation bound, what it does to tones, and (where torchaudio is installed) its
agreement with the real transform."""
import numpy as np
import pytest
import torch

from tests import _resample_oracle as ro

EPS = 2.0 ** -24


@pytest.mark.parametrize("pair", sorted(ro.TABLE), ids=str)
def test_geometry_table(pair):
    assert ro.geometry(*pair) == ro.TABLE[pair]
    o, n, width, K = ro.TABLE[pair]
    assert ro.taps32(*pair).shape == (n, K)


@pytest.mark.parametrize("case", sorted(ro.LENGTHS), ids=str)
def test_output_lengths(case):
    orig, new, L = case
    y = ro.resample(np.ones((1, L)), orig, new)
    assert y.shape == (1, ro.LENGTHS[case]) and ro.out_len(orig, new, L) == ro.LENGTHS[case]


@pytest.mark.parametrize("case", sorted(ro.LENGTHS), ids=str)
def test_float32_convolution_stays_within_the_summation_bound(case):
    """float32 conv1d with the oracle's taps differs from the float64 sum by at most (K + 2) * 2^-24 * conv(|taps|, |x|): K products
    and K - 1 additions, each one rounding, in any order -- the bound the device test uses."""
    orig, new, L = case
    o, n, width, K = ro.geometry(orig, new)
    x = np.random.default_rng(L).standard_normal((2, L)).astype(np.float32)
    want, bound = ro.resample(x, orig, new, with_bound=True)
    xp = torch.nn.functional.pad(torch.from_numpy(x)[:, None], (width, width + o))
    got = torch.nn.functional.conv1d(xp, torch.from_numpy(ro.taps32(orig, new))[:, None], stride=o)      # (B, n, J)
    got = got.transpose(1, 2).reshape(2, -1)[:, :want.shape[1]].numpy().astype(np.float64)
    ratio = np.abs(got - want) / ((K + 2) * EPS * bound + 1e-300)
    print(case, "largest |error| / bound:", float(ratio.max()))
    assert ratio.max() <= 1.0


def _tone(freq, sr, seconds=1.0):
    return np.sin(2 * np.pi * freq * np.arange(int(sr * seconds)) / sr)[None]


def test_a_tone_below_the_new_nyquist_is_reproduced():
    y = ro.resample(_tone(1000, 44100), 44100, 8000)
    assert y.shape == (1, 8000)
    err = np.abs(y - _tone(1000, 8000))[0, 100:-100].max()
    print("1 kHz tone, 44100 -> 8000: max |error| away from the edges", err)
    assert err < 3e-4                                   # 2 x the 1.35e-4 of the float64 restatement; only libm can move it


def test_a_tone_above_the_new_nyquist_is_removed():
    y = ro.resample(_tone(6000, 44100), 44100, 8000)
    peak = np.abs(y)[0, 100:-100].max()
    print("6 kHz tone, 44100 -> 8000: max |y| away from the edges", peak)
    assert peak < 4e-3                                  # 2 x the measured 1.76e-3


@pytest.mark.parametrize("pair", sorted(ro.TABLE), ids=str)
def test_against_torchaudio(pair):
    """Pins the restatement wherever torchaudio exists.  torchaudio convolves in float32, so the comparison allows the float32
    summation bound on top of one float32 rounding of the result."""
    ta = pytest.importorskip("torchaudio")
    orig, new = pair
    K = ro.TABLE[pair][3]
    x = np.random.default_rng(orig + new).standard_normal((2, 3001)).astype(np.float32)
    want, bound = ro.resample(x, orig, new, with_bound=True)
    got = ta.transforms.Resample(orig, new)(torch.from_numpy(x)).numpy().astype(np.float64)
    assert got.shape == want.shape
    assert np.all(np.abs(got - want) <= (K + 3) * EPS * bound)
