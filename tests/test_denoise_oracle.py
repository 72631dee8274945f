"""CPU: the spectral suppressor's definition (tests/_denoise_oracle.py, the numpy restatement of include/mfpa.h) held against
properties that do not come from the code under test: a closed form, a brute-force minimum, exact scaling by powers of two, the
bounds of the gain, the corners (silence, silence then signal, one frame), and what it is for -- the waveform SNR of a noise-free
tonal signal plus noise rises through STFT -> suppressor -> inverse STFT."""
import numpy as np
import pytest

from tests import _denoise_oracle as o


@pytest.fixture(scope="module")
def mags():
    return o.magnitudes(9, 150)


def test_fixed_noise_without_decision_direction_is_the_closed_form(mags):
    rng = np.random.default_rng(3)
    noise = 10.0 ** rng.uniform(-4.0, 2.0, mags.shape[:2])
    xi_min, g_floor = o.DEFAULTS["xi_min"], o.DEFAULTS["g_floor"]
    y, g, n = o.suppress(mags, a=0.0, noise=noise)
    p = mags * mags
    want = np.maximum(1.0 - 1.0 / (1.0 + np.maximum(np.maximum(p / noise[:, :, None] - 1.0, 0.0), xi_min)), g_floor)
    assert np.array_equal(g, want) and np.array_equal(n, np.broadcast_to(noise[:, :, None], mags.shape))
    assert np.array_equal(y, g * mags)


@pytest.mark.parametrize("back,ahead", [(0, 0), (0, 5), (5, 0), (48, 48)])
def test_windowed_minimum_is_the_brute_force(mags, back, ahead):
    alpha, bias = 0.7, 3.0
    _, _, n = o.suppress(mags, alpha=alpha, back=back, ahead=ahead, bias=bias)
    B, F, nF = mags.shape
    s = o.smooth(mags * mags, alpha)
    for t in range(nF):
        lo, hi = max(0, t - back), min(nF - 1, t + ahead)
        want = s[:, :, lo]
        for u in range(lo + 1, hi + 1):
            want = np.minimum(want, s[:, :, u])
        assert np.array_equal(n[:, :, t], bias * want), t
    if back == ahead == 0:
        assert np.array_equal(n, bias * s)


@pytest.mark.parametrize("scale", [2.0 ** -7, 2.0 ** 9])
def test_scaling_by_a_power_of_two_scales_y_and_keeps_g(mags, scale):
    y, g, n = o.suppress(mags)
    y2, g2, n2 = o.suppress(mags * scale)
    assert np.array_equal(g2, g) and np.array_equal(y2, y * scale) and np.array_equal(n2, n * (scale * scale))


def test_gain_bounds_and_corners(mags):
    y, g, n = o.suppress(mags)
    assert np.all(g >= o.DEFAULTS["g_floor"]) and np.all(g <= 1.0) and np.all(y <= mags) and np.all(y >= 0.0)
    assert np.all(y[2] == 0.0) and np.all(n[2] == 0.0)                       # the all-zero row
    assert np.all(np.isfinite(y[1])) and np.all(np.isfinite(g[1])) and np.all(np.isfinite(n[1]))   # zeros, then signal: q = +inf inside
    assert np.all(g[1, :, 60 - 48 - 1:60] <= 1.0) and np.any(g[1, :, 60:70] == 1.0)               # ... the gain is 1 there, not NaN
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(y))
    # denom divides, apply gates
    den = np.array([2.0, 3.0, 1.0, 0.5, 7.0])
    gate = np.array([True, False, True, False, True])
    y3, g3, n3 = o.suppress(mags, denom=den, apply=gate)
    assert np.array_equal(y3[gate], (y / den[:, None, None])[gate]) and np.array_equal(y3[~gate], (mags / den[:, None, None])[~gate])
    assert np.all(g3[~gate] == 1.0) and np.all(n3[~gate] == 0.0) and np.array_equal(g3[gate], g[gate])


@pytest.mark.parametrize("a,bias", [(0.9, 3.0), (0.5, 1.0), (0.0, 2.0)])
def test_one_frame(a, bias):
    m = o.magnitudes(7, 1)
    _, g, _ = o.suppress(m, a=a, bias=bias, xi_min=1e-9, g_floor=0.0)
    # s = p, n = bias p >= p: the instantaneous term is 0 and xi = a
    want = max(1.0 - 1.0 / (1.0 + max(a, 1e-9)), 0.0)
    assert np.all(g[m > 0] == want)
    assert a == 0.0 or abs(want - a / (1.0 + a)) < 1e-15


@pytest.mark.parametrize("kind,snr_in", o.CHAIN_CASES)
def test_the_chain_improves_waveform_snr_by_more_than_3_db(kind, snr_in):
    clean = o.tonal()
    x = o.noisy(clean, kind, snr_in)
    before, after = o.snr_db(clean, x), o.snr_db(clean, o.chain(x))
    print(f"{kind} noise at {snr_in} dB: {before:.2f} -> {after:.2f} dB")
    assert abs(before - snr_in) < 1e-9 and after > before + 3.0
