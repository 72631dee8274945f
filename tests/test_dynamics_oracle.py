"""CPU: properties of the compressor's definition as tests/_dynamics_oracle.py states it (the oracle the GPU tests measure against),
and of the host functions that form its parameters."""
import numpy as np
import pytest

from tests import _dynamics_oracle as do

T = 3000


@pytest.fixture(scope="module")
def x():
    return do.signal(T, seed=3, B=2)


def test_the_limiter_never_exceeds_its_threshold(x):
    q = do.case("lim")
    for run in (do.reference, do.truth):
        y = run(2.0 * x, q)[0]
        assert float(np.max(np.abs(y))) <= 10.0 ** (q[0] / 20.0) * (1.0 + 1e-12)
    assert float(np.max(np.abs(2.0 * x))) > 1.5                                        # there was something to limit


def test_no_time_constants_return_the_level_itself(x):
    q = do.case("inst")
    xl = do.levels(x, q)
    assert float(xl.max()) > 3.0 and float(xl.min()) == 0.0
    for run in (do.reference, do.truth):
        y, gr, zf = run(xl, q, level_in=True)
        assert np.array_equal(y, xl) and np.array_equal(gr, xl) and np.array_equal(zf, np.stack([xl[:, -1], xl[:, -1]], -1))


def test_ratio_one_reduces_nothing(x):
    for knee in (0.0, 6.0):
        y, gr, _ = do.reference(x, do.params(-20.0, 1.0, knee, 5.0, 100.0, 0.0))
        assert not gr.any() and np.array_equal(y, x)


@pytest.mark.parametrize("ratio", [2.0, 4.0, float("inf")])
def test_a_constant_above_the_threshold_settles(ratio):
    """0.5 is -6.02 dB, o = 13.98 dB over a threshold of -20 dB: the output level settles to threshold + o / ratio."""
    q = do.params(-20.0, ratio, 6.0, 5.0, 100.0, 0.0)
    y = do.reference(np.full(8000, 0.5), q)[0]
    o = 20.0 * np.log10(0.5) + 20.0
    assert abs(20.0 * np.log10(y[-1]) - (-20.0 + o / ratio)) <= 1e-9


@pytest.mark.parametrize("name", list(do.CASES))
@pytest.mark.parametrize("cut", [1, 1024, 1500])
def test_two_calls_through_the_state_are_one_call(x, name, cut):
    q = do.case(name)
    for level_in in (False, True):
        xin = do.levels(x, q) if level_in else x
        y, gr, zf = do.reference(xin, q, level_in=level_in)
        y0, g0, z0 = do.reference(xin[:, :cut], q, level_in=level_in)
        y1, g1, z1 = do.reference(xin[:, cut:], q, zi=z0, level_in=level_in)
        assert np.array_equal(np.concatenate([y0, y1], 1), y) and np.array_equal(np.concatenate([g0, g1], 1), gr) and np.array_equal(z1, zf)


def _level_in_errors(x, q):
    xl = do.levels(x, q)
    r = do.reference(xl, q, level_in=True)[0]
    return do.errors(r, (do.truth(xl, q, level_in=True)[0], r))


def test_the_reference_has_an_error_to_measure_against(x):
    """E > 0 on the three cases with memory, output and gain reduction, full and level-in mode; "inst" in level-in mode is exact."""
    for name in do.WITH_MEMORY:
        q = do.case(name)
        (ty, tg, _), (ry, rg, _) = do.truth(x, q), do.reference(x, q)
        Ey, Eg, El = do.errors(ry, (ty, ry))[1], do.errors(rg, (tg, rg))[1], _level_in_errors(x, q)[1]
        print(f"{name}: E(y) = {Ey:.2e}, E(gr) = {Eg:.2e}, E(level-in) = {El:.2e}")
        assert 0.0 < Ey < 1e-14 and 0.0 < Eg < 1e-12 and 0.0 < El < 1e-12              # a few roundings of values below 1 and below 64
    assert _level_in_errors(x, do.case("inst")) == (0.0, 0.0)


def test_rows_are_independent_and_per_row_parameters_are_the_shared_ones(x):
    q5 = do.five_rows()
    x5 = do.signal(600, seed=1, B=5)
    y, gr, zf = do.reference(x5, q5)
    for b in range(5):
        yb, gb, zb = do.reference(x5[b], q5[b])
        assert np.array_equal(yb, y[b]) and np.array_equal(gb, gr[b]) and np.array_equal(zb, zf[b])


def test_host_parameter_functions_agree_with_the_oracle():
    from musicfpaugment_amd import functional as F
    from musicfpaugment_amd import ops
    assert ops.time_coef(0.0, 8000) == 0.0 and ops.time_coef(0.005, 8000) == do.time_coef(0.005, 8000) == float(np.exp(-1.0 / 40.0))
    np.testing.assert_array_equal(ops.time_coef([0.0, 0.1], 8000), [0.0, do.time_coef(0.1, 8000)])
    for name, c in do.CASES.items():
        np.testing.assert_array_equal(F.compressor_params(8000, c[0], c[1], c[3], c[4], c[2], c[5]), do.case(name))
    rows = F.compressor_params(8000, [c[0] for c in do.CASES.values()], [c[1] for c in do.CASES.values()], 5.0, [c[4] for c in do.CASES.values()])
    assert rows.shape == (4, 6) and np.array_equal(rows[:, 0], [-20.0, -12.0, -6.0, -20.0]) and rows[2, 1] == 1.0
    assert np.all(rows[:, 2] == 6.0) and np.all(rows[:, 3] == do.time_coef(0.005, 8000))
