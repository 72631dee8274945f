"""CPU: the delay lines' oracle (tests/_delay_oracle.py) against facts that do not depend on it: integer delays are shifts, a delay
past either end is silence, the comb's impulse response is its coefficients, Schroeder's all-pass keeps the energy, and a
constant-speed ramp turns a sinusoid into a sinusoid of the scaled frequency.  The last one measures the interpolator's own error,
INTERP_ERR, which tests/test_gpu_delay.py reuses as its yardstick."""
import numpy as np
import pytest

from tests import _delay_oracle as do


def _shifted(x, D):
    y = np.zeros_like(x)
    T = x.shape[-1]
    if 0 <= D < T:
        y[..., D:] = x[..., :T - D]
    elif -T < D < 0:
        y[..., :T + D] = x[..., -D:]
    return y


def test_header_constants_are_mirrored():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mfpa.h")).read()
    for name, value in (("MFPA_VARIDELAY_TILE", do.TILE), ("MFPA_VARIDELAY_WINDOW", do.WINDOW), ("MFPA_DELAY_MAX_VOICES", do.MAX_VOICES)):
        assert int(re.search(r"#define %s (\d+)" % name, header).group(1)) == value


@pytest.mark.parametrize("filter_len", [3, 33, 81, 255])
def test_integer_delays_are_exact_shifts(filter_len):
    T = 300
    x = do.signal(T, seed=3, B=2)
    delays, gains, dry = [0, 1, 17, -4, T - 1, T, -T, 129], [0.5, -0.25, 0.125, 0.3, 0.7, 1.0, 2.0, -0.9], 0.6
    d = np.broadcast_to(np.array(delays, dtype=np.float64)[None, :, None], (2, len(delays), T))
    want = dry * x
    for D, g in zip(delays, gains):
        want = want + g * _shifted(x, D)
    for f in (do.reference, do.truth):
        y = f(x, d, gains, dry, filter_len)
        assert np.array_equal(np.asarray(y, dtype=np.float64), want) or f is do.truth
    assert float(np.max(np.abs(do.truth(x, d, gains, dry, filter_len) - want))) < 1e-15     # long double sums round differently
    assert np.array_equal(do.reference(x[0], d[0, 2], 1.0, 0.0, filter_len), _shifted(x[0], 17))


@pytest.mark.parametrize("filter_len", [3, 81, 255])
def test_a_delay_past_either_end_is_silence(filter_len):
    T, half = 200, (filter_len - 1) // 2
    x = do.signal(T, seed=4)
    for value in (T + half, T + half + 0.5, 1e6, 1e300, np.inf, -(T + half + 1.0), -1e6, -1e300, -np.inf, np.nan):
        y = do.reference(x, np.full(T, value), 1.0, 0.0, filter_len)
        assert not y.any(), value
        assert not do.live_mask(np.full(T, value), T, filter_len)[[0, T - 1]].all()
    y = do.reference(x, np.full(T, np.nan), 0.5, 0.25, filter_len)                 # the dry path is untouched
    assert np.array_equal(y, 0.25 * x)
    # a window that only touches the row contributes, and only there
    y = do.reference(x, np.full(T, T + half - 1.5), 1.0, 0.0, filter_len)
    assert y[:T - 2].any() == 0 and y[-1] != 0.0


def test_the_combs_impulse_response_is_its_coefficients():
    b0, bD, aD, D, T = 0.5, 0.25, -0.6, 7, 64
    h = do.comb_reference(do.impulse(T, 0), D, b0, bD, aD)
    want = np.zeros(T)
    want[0] = b0
    v = bD + aD * b0
    for k in range(D, T, D):
        want[k] = v
        v = v * aD
    assert np.array_equal(h, want)
    assert np.array_equal(do.comb_reference(do.impulse(T, 3), T + 5, b0, bD, aD), b0 * do.impulse(T, 3))      # D beyond the row
    x = do.signal(T, seed=5, B=3)
    rows = do.comb_reference(x, [1, 5, 64], [1.0, 0.5, -0.3], [0.0, 0.5, 1.0], [0.9, 0.0, 0.3])
    for b, q in enumerate([(1, 1.0, 0.0, 0.9), (5, 0.5, 0.5, 0.0), (64, -0.3, 1.0, 0.3)]):
        assert np.array_equal(rows[b], do.comb_reference(x[b], *q))
        y = np.zeros(T)
        for n in range(T):                                                                                    # the formula, sample by sample
            D_ = q[0]
            y[n] = q[1] * x[b, n] + (q[2] * (x[b, n - D_] if n >= D_ else 0.0) + q[3] * (y[n - D_] if n >= D_ else 0.0))
        assert np.array_equal(rows[b], y)


@pytest.mark.parametrize("g", [0.5, 0.7, -0.6])
def test_the_allpass_comb_keeps_the_energy(g):
    h = do.comb_reference(do.impulse(20000, 0), 13, -g, 1.0, g)                     # g^(20000 / 13) is far below 1e-12
    assert abs(float(np.sum(h * h)) - 1.0) < 1e-12


@pytest.mark.parametrize("eps", [0.01, -0.03])
def test_a_constant_speed_ramp_scales_a_sinusoids_frequency(eps):
    """1 kHz at 8 kHz read at p = (1 + eps) n is (1 + eps) kHz.  The oracle's largest error against the analytic sinusoid over the
    interior is the 81-tap Hann-windowed sinc's own at an eighth of the sample rate: 4.15e-6 for both slopes."""
    x, d, want, interior = do.ramp_case(eps)
    assert x.shape == (do.RAMP_T,) and interior.sum() > 3000
    err = float(np.max(np.abs(do.reference(x, d, 1.0, 0.0, 81) - want)[interior]))
    print(f"eps={eps}: INTERP_ERR measured {err:.4e}, recorded {do.INTERP_ERR[eps]:.4e}")
    assert 0.99 * do.INTERP_ERR[eps] <= err <= do.INTERP_ERR[eps]
    # the frequency itself, from the interpolated zero crossings of the interior
    y = do.reference(x, d, 1.0, 0.0, 81)
    n = np.nonzero(interior)[0]
    seg = y[n[0]:n[-1] + 1]
    k = np.nonzero((seg[:-1] < 0.0) & (seg[1:] >= 0.0))[0]
    t = k + seg[k] / (seg[k] - seg[k + 1])
    f = (len(t) - 1) / (t[-1] - t[0]) * do.SAMPLE_RATE
    assert abs(f / (1000.0 * (1.0 + eps)) - 1.0) < 1e-5


def test_delay_builders():
    d = do.speed_drift_delay(2, 4000, 8000, [(0.002, [0.8, 2.0], 0.3), (0.0, 8.0, 0.0), (0.001, 0.0, 0.0)])
    assert d.shape == (2, 4000) and not d[:, 0].any()
    speed = -np.diff(d, axis=1)                                                      # minus the derivative: the speed deviation
    n = np.arange(3999) + 0.5
    for b, hz in enumerate((0.8, 2.0)):
        assert np.max(np.abs(speed[b] - 0.002 * np.sin(2.0 * np.pi * hz * n / 8000 + 0.3))) < 1e-8
    l = do.lfo_delay(2, 1600, 8000, 20.0, [1.0, 2.0], 5.0, 0.0)                      # one period of 5 Hz
    assert np.allclose(l[:, 0], 160.0) and abs(l[1].max() - l[1].min() - 2 * 2.0 * 8.0) < 0.1


def test_a_single_impulse_rows_own_error_is_no_yardstick():
    """Why tests/test_gpu_delay.py holds an impulse row against the E of its five-row case and not against its own: over such a row E
    is the rounding luck of the two or three outputs near the impulse that are not tiny.  On "ramp_0.01, T = 127, 255 taps, V = 3"
    the definition evaluated in float64 with correctly rounded sinpi and cospi (no device involved, every other operation the
    reference's) misses 8 E of the impulse-at-0 row alone and sits at a fraction of the E of the case."""
    T, filter_len, V = 127, 255, 3
    x, d, g = do.rows(T), do.FAMILIES["ramp_0.01"](do.ROWS, V, T, 127), do.case_gains(V)
    want = do.truth(x, d, g, do.DRY, filter_len), do.reference(x, d, g, do.DRY, filter_len)
    y = do.reference_rounded_functions(x, d, g, do.DRY, filter_len)
    D_row, E_row = do.errors(y[2], (want[0][2], want[1][2]))
    D_case, E_case = do.errors(y, want)
    print(f"row 2 alone: D={D_row:.4e} E={E_row:.4e} D/E={D_row / E_row:.2f}; the case: D={D_case:.4e} E={E_case:.4e} D/E={D_case / E_case:.2f}")
    assert D_row > do.BOUND * E_row and 2.0e-16 < D_row < 3.0e-16 and E_row < 3.0e-17
    assert D_case <= 2.0 * E_case and D_row < 0.5 * E_case
    for b in range(2):                                                   # a seeded-signal row alone is a fair case
        D, E = do.errors(y[b], (want[0][b], want[1][b]))
        assert D <= 2.0 * E


def test_a_fraction_that_rounds_to_one_weighs_the_last_tap():
    """frac == 1 (a tiny negative position) is the one case in which j = half + 1 passes |t| <= half; the result is the sample at
    whole + 1 = 0 to within the float64 sine of pi."""
    for filter_len in (3, 81):
        T = 50
        x = do.signal(T, seed=6)
        d = do.near_one(1, 1, T, (filter_len - 1) // 2)[0, 0]
        assert d[0] == 2.0 ** -60 and (0.0 - d[0]) - np.floor(0.0 - d[0]) == 1.0
        for f in (do.reference, do.reference_rounded_functions, do.truth):
            assert abs(float(f(x, d, 1.0, 0.0, filter_len)[0] - x[0])) < 1e-15
