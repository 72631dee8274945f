"""CPU: the numpy phase-vocoder oracle (tests/_vocoder_oracle.py) against an independent restatement in torch ops -- torchaudio's
public source as text, with its own torch.linspace, cumsum and polar -- to 8 E, and two properties that depend on neither:
a stretched sinusoid has the length round(T / rate) and keeps its frequency.

The level is NOT asserted.  For rates below 1 the algorithm repeats frame 0 (floor(i r) = 0 for several i), whose reflect-padded
phases do not fit a sinusoid; the accumulated phase then runs off the frames' own and neighbouring frames cancel in the overlap-add:
mid-signal RMS drops to 0.55-0.77 of the input's.  For rates above 1 it is 1.0000.  This is torchaudio's algorithm, not this
restatement of it."""
import math

import numpy as np
import pytest
import torch

from tests import _istft_oracle as io
from tests import _vocoder_oracle as vo
from tests._vocoder_oracle import TONE_RATES, TONES, dominant_frequency, middle_half, noise_spectrum, tones

needs_longdouble = pytest.mark.skipif(not vo.HAVE_LONGDOUBLE, reason="np.longdouble is no wider than float64 here: no error unit")

SIZES = (511, 1000, 8548, 24000, 64000)                    # 2, 4, 34, 94, 251 frames
RATES = (0.5, 0.7, 0.9, 1.0, 1.1, 1.3, 2.0)


def torch_phase_vocoder(spec, rate):
    """torchaudio.functional.phase_vocoder (hop 256, 257 bins) for one (257, n_frames) complex128 tensor."""
    if rate == 1.0:
        return spec
    phase_advance = torch.linspace(0, math.pi * 256, 257, dtype=torch.float64)[..., None]
    # t_i = i * rate, rounded once (include/mfpa.h).  torch.arange(0, n, rate) has this length, but its CPU kernel forms the values in
    # vector blocks, (block start * rate) + (lane * rate): two roundings, which land on the other side of an integer now and then
    # (rate 0.7: frame j - 1 for j) -- another input frame, not a rounding difference.  A device arange multiplies once, like this.
    n_out = len(torch.arange(0, spec.size(-1), rate, dtype=torch.float64))
    time_steps = torch.arange(n_out, dtype=torch.float64) * rate
    alphas = time_steps % 1.0
    phase_0 = spec[..., :1].angle()
    padded = torch.nn.functional.pad(spec, [0, 2])
    s0 = padded.index_select(-1, time_steps.long())
    s1 = padded.index_select(-1, time_steps.long() + 1)
    angle_0, angle_1, norm_0, norm_1 = s0.angle(), s1.angle(), s0.abs(), s1.abs()
    phase = angle_1 - angle_0 - phase_advance
    phase = phase - 2 * math.pi * torch.round(phase / (2 * math.pi))
    phase = phase + phase_advance
    phase = torch.cat([phase_0, phase[..., :-1]], dim=-1)
    phase_acc = torch.cumsum(phase, -1)
    mag = alphas * norm_1 + (1 - alphas) * norm_0
    return torch.polar(mag, phase_acc)


def test_frame_counts_are_those_of_arange():
    for n in (1, 2, 3, 4, 251, 16384):
        for r in (0.5, 0.7, 1.0, 1.3, 2.0, 300.0):
            assert vo.frames(n, r) == len(np.arange(0, n, r)) == len(torch.arange(0, n, r, dtype=torch.float64)), (n, r)
    for r in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert vo.frames(10, r) == -1
    # pi k: torch.linspace's own values where its kernel fuses 256 pi - pi (256 - k), at most one ulp of 256 pi away where it does not
    lin = torch.linspace(0, math.pi * 256, 257, dtype=torch.float64).numpy()
    assert np.abs(vo.phase_advance() - lin).max() <= np.spacing(256 * math.pi) and np.array_equal(vo.phase_advance()[:128], lin[:128])


@needs_longdouble
@pytest.mark.parametrize("T", SIZES)
def test_oracle_against_the_torch_restatement(T):
    spec = noise_spectrum(T)
    nF = spec.shape[2]
    for rate in RATES + (nF + 0.5,):
        E = vo.error_unit(spec, rate)
        out, n = vo.phase_vocoder(spec, rate)
        assert n.tolist() == [vo.frames(nF, rate)] * 3 and out.shape == (3, 257, n[0])
        worst = 0.0
        for b in range(3):
            want = torch_phase_vocoder(torch.from_numpy(spec[b]), rate).numpy()
            assert want.shape == out[b].shape
            worst = max(worst, float(np.abs(out[b] - want).max()))
        if rate == 1.0:
            assert E == 0.0 and worst == 0.0 and np.array_equal(out, spec)
            continue
        print(f"oracle vs torch ops T={T} rate={rate}: {worst / E:.3f} E (E = {E:.3e})")
        assert worst <= 8 * E, (T, rate, worst / E)


@needs_longdouble
def test_error_unit_has_the_documented_size():
    assert 1e-13 < vo.error_unit(noise_spectrum(1000), 0.5) < 1e-10                 # 4 frames -> 8
    assert 1e-10 < vo.error_unit(noise_spectrum(64000), 0.5) < 2e-7                 # 251 frames -> 502


def test_oracle_edges():
    spec = noise_spectrum(1000).copy()
    spec[0, 5] = 0                                                                 # a row of exactly zero bins: magnitude 0, phase 0
    spec[1, 0] = 2.0j                                                              # imaginary DC and Nyquist
    spec[1, 256] = -3.0j
    out, n = vo.phase_vocoder(spec, [0.7, 1.3, float("nan")], ld_out=9)
    assert n.tolist() == [6, 4, -1] and out.shape == (3, 257, 9)
    assert not out[0, 5].any() and not out[0, :, 6:].any() and not out[1, :, 4:].any() and not out[2].any()
    assert np.allclose(np.abs(out[1, 0, 0]), 2.0) and np.allclose(out[1, 0, 0], 2.0j) and np.allclose(out[1, 256, 0], -3.0j)
    out, n = vo.phase_vocoder(spec, [0.5, 1.0, 2.0], ld_out=7)                      # 8 frames do not fit into 7
    assert n.tolist() == [-1, 4, 2] and np.array_equal(out[1, :, :4], spec[1]) and not out[0].any()
    # frame 0 of every output is frame 0 of the input; magnitudes interpolate
    assert np.allclose(out[2, :, 0], spec[2, :, 0], rtol=1e-14, atol=1e-14)
    assert np.allclose(np.abs(out[2, :, 1]), np.abs(spec[2, :, 2]), rtol=1e-13, atol=1e-14)


@pytest.mark.parametrize("rate", TONE_RATES, ids=lambda r: f"{r:.4f}")
def test_a_stretched_sinusoid_keeps_its_frequency(rate):
    """Bound 1e-4 relative (the estimator's own error on a clean sinusoid of this length is below 1e-6; measured through the
    oracle on this grid: at most 1.5e-5)."""
    x = tones()
    T = x.shape[1]
    spec = io.torch_stft(x).numpy()
    out, n = vo.phase_vocoder(spec, rate)
    L = vo.stretched_length(T, rate)
    y = io.torch_istft(torch.from_numpy(out), L).numpy()
    assert y.shape == (len(TONES), L) and L == round(T / rate)
    for f, row in zip(TONES, y):
        got = dominant_frequency(middle_half(row))
        print(f"tone {f} Hz rate {rate:.4f}: {abs(got - f) / f:.2e} relative, mid RMS {np.sqrt(np.mean(middle_half(row) ** 2)) / (0.5 / np.sqrt(2)):.4f}")
        assert abs(got - f) / f <= 1e-4, (f, rate, got)


def test_the_estimator_on_clean_sinusoids():
    for f, row in zip(TONES, tones().numpy()):
        assert abs(dominant_frequency(middle_half(row)) - f) / f < 1e-6
