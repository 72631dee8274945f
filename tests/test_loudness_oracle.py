"""CPU: the numpy restatement of csrc/loudness.hip (tests/_loudness_oracle.py) against the definition in long double, with the plain
float64 definition's own error as the yardstick (D <= 8 E); the K-weighting design against the table of ITU-R BS.1770-4; and the
conformance signals of BS.1770, EBU Tech 3341 and EBU Tech 3342 through the plain float64 definition.

Worst D/E seen here: segments 3.1 (the 48 kHz K-weighting, hop 512), gated powers 0.23."""
import functools

import numpy as np
import pytest
import scipy.signal

from tests import _loudness_oracle as o

BS1770_TABLE = np.array([[1.53512485958697, -2.69169618940638, 1.19839281085285, 1.0, -1.69065929318241, 0.73248077421585],
                         [1.0, -2.0, 1.0, 1.0, -1.99004745483398, 0.99007225036621]])
T = 3 * o.SUPER + 17
HOPS = (1, 3, 16, 17, 512, 1024, 1025, 2500)


def _sos(sample_rate, design="bs1770"):
    from musicfpaugment_amd.functional import k_weighting_sos
    return k_weighting_sos(sample_rate, design)


def test_k_weighting_reproduces_the_table_of_bs1770_at_48_khz():
    sos = _sos(48000)
    assert sos.shape == (2, 6) and sos.dtype == np.float64
    assert np.max(np.abs(sos - BS1770_TABLE)) <= 1e-12


def test_k_weighting_designs_and_refusals():
    ta = _sos(48000, "torchaudio")
    assert ta.shape == (2, 6) and np.all(ta[:, 3] == 1.0)
    f = np.geomspace(20.0, 20000.0, 400)
    db = [20.0 * np.log10(np.abs(scipy.signal.sosfreqz(s, worN=f, fs=48000)[1])) for s in (ta, BS1770_TABLE)]
    assert 0.01 < np.max(np.abs(db[0] - db[1])) <= 0.05                        # another filter, 0.043 dB from the table at the most
    for fs in (8000, 16000, 22050, 44100, 96000):
        sos = _sos(fs)
        assert np.all(sos[:, 3] == 1.0) and np.array_equal(sos[1, :3], [1.0, -2.0, 1.0])
        poles = np.concatenate([np.roots(s[3:]) for s in sos])
        assert np.all(np.abs(poles) < 1.0)
    for bad in (dict(sample_rate=0), dict(sample_rate=float("nan")), dict(sample_rate=3000), dict(sample_rate=48000, design="a-weighting")):
        with pytest.raises(ValueError):
            _sos(**bad)


@functools.lru_cache(maxsize=None)
def _signal(rows: int = 2) -> np.ndarray:
    return np.random.default_rng(5).uniform(-1.0, 1.0, (rows, T))


@pytest.mark.parametrize("rate", [8000, 48000, None], ids=["k8k", "k48k", "unweighted"])
def test_restated_segments_within_eight_of_the_plain_definitions_error(rate):
    sos = _sos(rate) if rate else None
    for hop in HOPS:
        D = E = 0.0
        for x in _signal():
            t = o.truth_segments(x, sos, hop)
            D = max(D, float(np.max(np.abs(o.restate_segments(x, sos, hop)[0] - t))))
            E = max(E, float(np.max(np.abs(o.plain_segments(x, sos, hop) - t))))
        print(f"{rate} hop={hop}: D={D:.3e} E={E:.3e} D/E={D / E if E else 0:.2f}")
        assert D <= o.BOUND * E, (hop, D, E)
        assert E > 0 or hop == 1                                                # one square per segment: no sum, no error


def test_restated_peak_is_exact_and_skips_nan():
    x = _signal()[0].copy()
    assert o.restate_segments(x, None, 100)[1] == np.max(np.abs(x))
    x[7] = np.nan
    assert o.restate_segments(x, None, 100)[1] == np.nanmax(np.abs(x))


def _programme(seed: int, C: int, nseg: int, hop: int) -> np.ndarray:
    """Segment energies (C, nseg) of a programme with loud, quiet and near-silent stretches: every gate takes decisions."""
    rng = np.random.default_rng(seed)
    runs = rng.integers(35, 70, size=nseg // 35 + 1)                            # stretches longer than the longest block (30 segments)
    level = np.repeat(rng.permutation(np.resize([1e-9, 3e-5, 1e-3, 0.02, 0.3], len(runs))), runs)[:nseg]
    return hop * level[None, :] * rng.uniform(0.5, 1.5, (C, nseg))


@pytest.mark.parametrize("win,rel", [(4, 0.1), (30, 0.01), (1, 0.1)])
def test_restated_gate_within_eight_of_the_plain_definitions_error(win, rel):
    hop, surround = 800, [1.0, 1.0, 1.0, 1.41, 1.41]
    D, E = np.zeros(4), np.zeros(4)
    for seed in range(12):
        C = (1, 2, 5)[seed % 3]
        weights = surround if C == 5 else None
        seg = _programme(seed, C, 300 + 37 * seed, hop)
        t = o.definition_gate(seg, hop, win, rel, weights, dtype=np.longdouble)
        assert t["margin"] >= 1e-9, (seed, t["margin"])                         # no decision within rounding of its threshold
        r, p = o.restate_gate(seg, hop, win, rel, weights), o.definition_gate(seg, hop, win, rel, weights)
        assert 0 < t["n_rel"] < t["n_abs"] < len(t["blocks"]), "the case must exercise both gates"
        for got in (r, p):
            assert (got["n_abs"], got["n_rel"]) == (t["n_abs"], t["n_rel"])
        for i, key in enumerate(("power", "abs_power", "lo", "hi")):
            D[i] = max(D[i], abs(float(np.longdouble(r[key]) - t[key])))
            E[i] = max(E[i], abs(float(np.longdouble(p[key]) - t[key])))
    print(f"win={win}: D={D} E={E}")
    assert np.all(D <= o.BOUND * E) and np.all(E[:2] > 0)                      # the ranks select: their error is one block power's


def test_rank_formulas_are_the_nearest_ranks():
    for n in range(1, 5000):
        assert o.rank_indices(n) == (int((n - 1) * 0.10 + 0.5), int((n - 1) * 0.95 + 0.5))


def test_gain_restatement_rules():
    x = np.random.default_rng(2).uniform(-0.5, 0.5, (5, 2, 64)).astype(np.float32)
    gated = np.array([1e-3, 0.0, 2e-3, 5e-4, 1e-3])
    target = np.full(5, o.power_of(-23.0))
    peak = np.abs(x).max(axis=2).astype(np.float64)
    y, g = o.restate_gain(x, gated, target, apply=[True, True, True, True, False])
    assert np.array_equal(y[1], x[1]) and np.array_equal(y[4], x[4]) and g[1] == 1.0 and g[4] == 1.0
    assert g[0] == np.sqrt(target[0] / gated[0]) and np.array_equal(y[0], (x[0].astype(np.float64) * g[0]).astype(np.float32))
    y2, g2 = o.restate_gain(x, gated, np.full(5, o.power_of(0.0)), peak, 0.9)
    assert np.all(g2[[0, 2, 3, 4]] == 0.9 / peak.max(axis=1)[[0, 2, 3, 4]])      # the limit binds
    assert np.max(np.abs(y2)) <= 0.9 * (1 + 1e-7)


@pytest.mark.parametrize("rate,want", [(48000, -3.01), (8000, -3.01), (44100, -3.01)])
def test_bs1770_full_scale_sine_reads_minus_3_01(rate, want):
    r = o.plain_loudness(o.sine(997.0, rate, 20.0, 0.0), rate, _sos(rate))
    print(rate, o.lufs_of(r["power"]))
    assert abs(o.lufs_of(r["power"]) - want) <= 0.05


@pytest.mark.parametrize("case", sorted(o.TECH_3341))
def test_ebu_tech_3341_integrated_loudness(case):
    parts, want = o.TECH_3341[case]
    r = o.plain_loudness(o.steps(48000, parts), 48000, _sos(48000))
    print(case, o.lufs_of(r["power"]))
    assert abs(o.lufs_of(r["power"]) - want) <= 0.1


@pytest.mark.parametrize("case", sorted(o.TECH_3342))
def test_ebu_tech_3342_loudness_range(case):
    parts, want = o.TECH_3342[case]
    r = o.plain_loudness(o.steps(48000, parts), 48000, _sos(48000), win=30, rel=0.01)
    print(case, o.lra_of(r["lo"], r["hi"]))
    assert abs(o.lra_of(r["lo"], r["hi"]) - want) <= 1.0
