"""GPU: csrc/delay.hip (ops.variable_delay, ops.comb) against tests/_delay_oracle.py, and the fronts over it: the functional
entries and the Echo / WowFlutter / Chorus transforms.

The variable delay is held against the long-double truth with the float64 definition's own error as the yardstick (D <= 8 E, and
the reference's bits where E == 0); every accuracy case prints its D/E.  The comb is held against the numpy restatement bit for bit.

Coverage of the accuracy cases: every delay family (tests/_delay_oracle.py, FAMILIES) runs at every T of (1, half, TILE - 1, TILE,
TILE + 1, 2 TILE + 3) with every filter_len of (3, 33, 81, 255); V walks (1, 3, 8) over those 24 combinations so that each T and
each filter_len meets each V, and at 2 TILE + 3 / 81 taps all three V run.  Every combination is three cases: B = 5, the two
rows of the seeded signal and a unit impulse at n = 0, TILE - 1 and TILE (which shows every tap weight on its own) launched
together and held against the E of the five rows; and B = 1 twice, each seeded-signal row launched alone and held against the
truth, the reference and the E of that row alone.  The five single-row launches must also equal the B = 5 launch bit for bit.

An impulse row is part of the B = 5 case and is not a case of its own: over such a row alone E is the luck of the two or three
roundings of the few outputs near the impulse that are not tiny.  tests/test_delay_oracle.py shows it on the CPU, no device
involved: on "ramp_0.01, T = 127, 255 taps, V = 3", row 2, the definition evaluated in float64 with correctly rounded sinpi and
cospi has D = 2.47e-16 against that row's E = 2.54e-17 (9.7), which is 0.05 of the case's E.  Those rows' own ratios are printed.

Worst D/E on one MI355X, per family the B = 5 cases / the B = 1 cases: integer 1.00 / 1.00, frac_0.25
1.10 / 1.12, frac_0.5 1.00 / 1.24, frac_1-2^-50 1.00 / 1.00, lfo 1.00 / 1.00, ramp_0.01 1.00 / 1.00, ramp_-0.03 1.20 / 1.20, negative
1.00 / 1.18, edges 1.05 / 1.26, random 0.58 / 1.00 (1.00 is mostly the reference's very bits).  Printed only, an impulse row
against its own E: lfo 4.44, random 3.31, negative 1.97, ramp_0.01 9.72 (the row named above), the others at most 1.32.
T = 2 WINDOW + 5: lfo 0.00, random 0.02, edges 0.77."""
import functools
import random

import numpy as np
import pytest
import torch

from tests import _delay_oracle as do

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
B = 5
TILE, WINDOW = do.TILE, do.WINDOW
FILTERS = (3, 33, 81, 255)
T_NAMES = ("1", "half", "TILE-1", "TILE", "TILE+1", "2TILE+3")
VOICES = (1, 3, 8)
GAINS, DRY, FAMILIES = do.GAINS, do.DRY, do.FAMILIES


def _ops():
    from musicfpaugment_amd import ops
    return ops


def _length(name: str, filter_len: int) -> int:
    return {"1": 1, "half": (filter_len - 1) // 2, "TILE-1": TILE - 1, "TILE": TILE, "TILE+1": TILE + 1, "2TILE+3": 2 * TILE + 3}[name]


@functools.lru_cache(maxsize=None)
def _rows(T: int) -> np.ndarray:
    x = do.rows(T)
    x.setflags(write=False)
    return x


def _dev(a: np.ndarray, dtype=torch.float64) -> torch.Tensor:
    return torch.from_numpy(np.array(a, order="C")).to(dtype).to(DEV)


def _ratio(D, E):
    return "exact" if E == 0.0 and D == 0.0 else "inf" if E == 0.0 else format(D / E, ".2f")


def _check(tag: str, got: torch.Tensor, t: np.ndarray, r: np.ndarray) -> float:
    got = got.cpu().numpy()
    D, E = do.errors(got, (t, r))
    print(f"{tag}: D={D:.3e} E={E:.3e} D/E={_ratio(D, E)}")
    if E == 0.0:
        assert np.array_equal(got, r), tag
    assert D <= do.BOUND * E, (tag, D, E)
    return D / E if E else 0.0


def _accuracy(family: str, T: int, filter_len: int, V: int) -> float:
    """One parameter combination: the B = 5 case (the five rows together, its E over the five rows) and two B = 1 cases (each
    seeded-signal row launched alone, against the truth, the reference and the E of that row alone)."""
    ops = _ops()
    half = (filter_len - 1) // 2
    x, d, g = _rows(T), FAMILIES[family](B, V, T, half), do.case_gains(V)
    t, r = do.truth(x, d, g, DRY, filter_len), do.reference(x, d, g, DRY, filter_len)
    xd, dd = _dev(x), _dev(d)
    tag = f"{family} T={T} taps={filter_len} V={V}"
    together = ops.variable_delay(xd, dd, g, dry=DRY, filter_len=filter_len)
    alone = [ops.variable_delay(xd[b:b + 1], dd[b:b + 1], g[b:b + 1], dry=DRY[b:b + 1], filter_len=filter_len) for b in range(B)]
    for b in range(2, B):                                                               # the impulse rows on their own E: printed only (docstring)
        D, E = do.errors(together[b].cpu().numpy(), (t[b], r[b]))
        print(f"{tag} impulse row {b}: D={D:.3e} E={E:.3e} D/E={_ratio(D, E)}")
    worst = _check(f"{tag} B={B}", together, t, r)
    for b in range(2):
        worst = max(worst, _check(f"{tag} B=1 signal row {b}", alone[b], t[b:b + 1], r[b:b + 1]))
    assert torch.equal(torch.cat(alone), together), tag
    return worst


@pytest.mark.parametrize("t_name", T_NAMES)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_varidelay_within_eight_of_the_definitions_errors(family, t_name):
    worst = 0.0
    for i, filter_len in enumerate(FILTERS):
        T = _length(t_name, filter_len)
        voices = VOICES if (t_name, filter_len) == ("2TILE+3", 81) else (VOICES[(T_NAMES.index(t_name) + i) % 3],)
        for V in voices:
            worst = max(worst, _accuracy(family, T, filter_len, V))
    print(f"family {family} T={t_name}: worst D/E = {worst:.2f}")


@pytest.mark.parametrize("family", ["lfo", "random", "edges"])
def test_varidelay_two_windows_long(family):
    """T = 2 WINDOW + 5: nine tiles, the read positions of the random family spread over the whole row."""
    T, V, filter_len = 2 * WINDOW + 5, 3, 81
    x, d = _rows(T), FAMILIES[family](B, V, T, 40)
    want = do.truth(x, d, GAINS[:V], DRY, filter_len), do.reference(x, d, GAINS[:V], DRY, filter_len)
    _check(f"{family} T={T}", _ops().variable_delay(_dev(x), _dev(d), GAINS[:V], dry=DRY, filter_len=filter_len), *want)


# ----------------------------------------------------------------------------- exact cases
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("T", [1, TILE, 2 * TILE + 3])
def test_integer_delays_are_the_numpy_expression_bit_for_bit(T, dtype):
    ops = _ops()
    x = do.signal(T, seed=9, B=3)
    if dtype == torch.float32:
        x = x.astype(np.float32).astype(np.float64)
    delays = [0, T, 1, -1, T - 1, -T, 17, 3]
    for filter_len in FILTERS:
        want = DRY[:3, None] * x
        for D_, g in zip(delays, GAINS):
            sh = np.zeros_like(x)
            if 0 <= D_ < T:
                sh[:, D_:] = x[:, :T - D_]
            elif -T < D_ < 0:
                sh[:, :T + D_] = x[:, -D_:]
            want = want + g * sh
        d = np.broadcast_to(np.array(delays, dtype=np.float64)[None, :], (3, 8))
        y = ops.variable_delay(_dev(x, dtype), _dev(d), GAINS, dry=DRY[:3], filter_len=filter_len)
        assert y.dtype == dtype and np.array_equal(y.cpu().numpy(), want.astype(np.float32) if dtype == torch.float32 else want), (T, filter_len)
    z = torch.zeros((3, T), dtype=dtype, device=DEV)
    assert not ops.variable_delay(z, _dev(do.lfo(3, 3, T)), GAINS[:3], dry=0.5).any()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_unselected_rows_are_the_inputs_bits(dtype):
    ops = _ops()
    T = 2 * TILE + 3
    x, d = _dev(_rows(T), dtype), _dev(do.lfo(B, 3, T))
    gate = torch.tensor([True, False, True, False, False])
    y = ops.variable_delay(x, d, GAINS[:3], dry=DRY)
    for g in (gate, gate.to(DEV), gate.tolist()):
        yg = ops.variable_delay(x, d, GAINS[:3], dry=DRY, apply=g)
        assert torch.equal(yg[~gate], x[~gate]) and torch.equal(yg[gate], y[gate])
    assert torch.equal(ops.variable_delay(x, d, apply=torch.zeros(B, dtype=torch.bool)), x)
    q = ([5, 64, 300, 7, 1], 0.5, 0.25, [0.5, -0.5, 0.9, 0.0, 0.3])
    c = ops.comb(x, *q)
    cg = ops.comb(x, *q, apply=gate)
    assert torch.equal(cg[~gate], x[~gate]) and torch.equal(cg[gate], c[gate]) and not torch.equal(c[1], x[1])
    assert torch.equal(ops.comb(x, *q, apply=[False] * B), x)


# ----------------------------------------------------------------------------- invariances
@pytest.mark.parametrize("family", ["lfo", "random", "edges", "ramp_0.01"])
def test_a_row_does_not_depend_on_its_batch(family):
    ops = _ops()
    T, V = 2 * TILE + 3, 3
    x, d = _dev(_rows(T)), _dev(FAMILIES[family](B, V, T, 40))
    g = np.broadcast_to(GAINS[:V], (B, V)) * (1.0 + 0.1 * np.arange(B))[:, None]
    y = ops.variable_delay(x, d, g, dry=DRY)
    assert torch.equal(ops.variable_delay(x, d, g, dry=DRY), y)
    for b in range(B):
        assert torch.equal(ops.variable_delay(x[b:b + 1], d[b:b + 1], g[b:b + 1], dry=DRY[b:b + 1])[0], y[b]), b
        xs, ds = x.clone(), d.clone()                                                   # row b at position 0, another neighbour family
        xs[0], ds[0] = x[b], d[b]
        ds[1:] = _dev(do.random_delays(B - 1, V, T, seed=b))
        gs, g0 = g.copy(), DRY.copy()
        gs[0], g0[0] = g[b], DRY[b]
        assert torch.equal(ops.variable_delay(xs, ds, gs, dry=g0)[0], y[b]), b


def test_constant_voices_equal_their_expansion():
    ops = _ops()
    T = 2 * TILE + 3
    x = _dev(_rows(T))
    for V in VOICES:
        c = do.constant(B, V, T, 2.3, 37.7)[:, :, 0]
        full = ops.variable_delay(x, _dev(np.broadcast_to(c[:, :, None], (B, V, T))), GAINS[:V], dry=DRY)
        for form in (_dev(c), _dev(c[:, :, None]), _dev(c)[:, :, None].expand(B, V, T), c, c[:, :, None]):
            assert torch.equal(ops.variable_delay(x, form, GAINS[:V], dry=DRY), full), V
        row0 = ops.variable_delay(x, _dev(c[:1]).expand(B, V), GAINS[:V], dry=DRY)      # a stride of 0 over the batch
        assert torch.equal(row0, ops.variable_delay(x, _dev(np.broadcast_to(c[:1, :, None], (B, V, T))), GAINS[:V], dry=DRY))
    assert torch.equal(ops.variable_delay(x, _dev(c).float(), GAINS[:V], dry=DRY),
                       ops.variable_delay(x, _dev(c).float().double(), GAINS[:V], dry=DRY))      # float32 delays are upcast


@pytest.mark.parametrize("filter_len", [3, 81, 255])
def test_staged_and_direct_paths_give_the_same_bits_at_the_window_boundary(filter_len):
    """Tile 0 reads along a steep ramp from position 0; its last lane reads at P + 0.5 or one sample further.  With
    P = WINDOW - filter_len - 1 the tile's window [0 - half, P + half + 1] holds exactly WINDOW samples (staged); one further it
    holds WINDOW + 1 (direct).  The two delay tensors differ in that one sample only, so every other output must keep its bits,
    and both runs meet the oracle."""
    ops = _ops()
    T, V = 2 * WINDOW + 5, 2
    P = WINDOW - filter_len - 1
    n = np.arange(T, dtype=np.float64)
    slope = (P - 1.0) / (TILE - 2)
    d = np.stack([np.where(n < TILE, n - slope * n, 11.5), np.where(n < TILE, n - 0.5 * slope * n, -3.25)])[None].repeat(2, 0)
    d[:, 0, TILE - 1] = (TILE - 1) - (P + 0.5)
    staged, direct = d.copy(), d.copy()
    direct[:, 0, TILE - 1] -= 1.0
    x = _rows(T)[:2]
    for dd in (staged, direct):                                                         # the window sizes the kernel will find, from the header's constants
        p = n[:TILE] - dd[0, 0, :TILE]
        size = (np.floor(p.max()) + (filter_len - 1) // 2 + 1) - (np.floor(p.min()) - (filter_len - 1) // 2) + 1
        assert size == (WINDOW if dd is staged else WINDOW + 1)
    ys = ops.variable_delay(_dev(x), _dev(staged), GAINS[:V], dry=DRY[:2], filter_len=filter_len)
    yd = ops.variable_delay(_dev(x), _dev(direct), GAINS[:V], dry=DRY[:2], filter_len=filter_len)
    _check(f"staged taps={filter_len}", ys, do.truth(x, staged, GAINS[:V], DRY[:2], filter_len), do.reference(x, staged, GAINS[:V], DRY[:2], filter_len))
    _check(f"direct taps={filter_len}", yd, do.truth(x, direct, GAINS[:V], DRY[:2], filter_len), do.reference(x, direct, GAINS[:V], DRY[:2], filter_len))
    same = torch.ones(T, dtype=torch.bool, device=DEV)
    same[TILE - 1] = False
    assert torch.equal(ys[:, same], yd[:, same]) and ys[:, :TILE].abs().max() > 0.1


@pytest.mark.parametrize("filter_len", [33, 81])
def test_one_wild_sample_sends_the_tile_down_the_direct_path_and_changes_nothing_else(filter_len):
    ops = _ops()
    T, V = 2 * WINDOW + 5, 3
    x, smooth = _dev(_rows(T)), do.lfo(B, V, T)
    ys = ops.variable_delay(x, _dev(smooth), GAINS[:V], dry=DRY, filter_len=filter_len)
    wild = smooth.copy()
    spots = [(0, 0, 5), (1, 2, TILE + 100), (2, 1, 3 * TILE), (3, 0, T - 1), (4, 2, WINDOW)]
    for b, v, n in spots:
        wild[b, v, n] = n - (T - 60.5) if n < T // 2 else n - 50.25                    # reads at the other end of the row
    yw = ops.variable_delay(x, _dev(wild), GAINS[:V], dry=DRY, filter_len=filter_len)
    same = torch.ones((B, T), dtype=torch.bool, device=DEV)
    for b, v, n in spots:
        same[b, n] = False
    assert torch.equal(ys[same], yw[same])
    _check(f"wild taps={filter_len}", yw, do.truth(_rows(T), wild, GAINS[:V], DRY, filter_len), do.reference(_rows(T), wild, GAINS[:V], DRY, filter_len))


@pytest.mark.parametrize("family", ["lfo", "random", "frac_0.5"])
def test_float32_is_the_float64_result_rounded_once(family):
    ops = _ops()
    T, V = 2 * TILE + 3, 3
    x32, d = _dev(_rows(T), torch.float32), _dev(FAMILIES[family](B, V, T, 40))
    y64 = ops.variable_delay(x32.double(), d, GAINS[:V], dry=DRY)
    y32 = ops.variable_delay(x32, d, GAINS[:V], dry=DRY)
    assert y32.dtype == torch.float32 and y64.dtype == torch.float64 and torch.equal(y32, y64.float())
    assert torch.equal(ops.variable_delay(x32, d, GAINS[:V], dry=DRY, out_dtype=torch.float64), y64)
    assert torch.equal(ops.variable_delay(x32.double(), d, GAINS[:V], dry=DRY, out_dtype=torch.float32), y32)


# ----------------------------------------------------------------------------- guards
@pytest.mark.parametrize("filter_len", [3, 81, 255])
def test_delays_that_are_not_finite_or_absurd_contribute_exactly_nothing(filter_len):
    ops = _ops()
    T, V = 2 * TILE + 3, 3
    x, d = _rows(T), do.lfo(B, V, T)
    bad = [np.inf, -np.inf, np.nan, 1e300, -1e300]
    rng = np.random.default_rng(3)
    hit = np.zeros((B, V, T), dtype=bool)
    for k in range(60):
        b, v, n = rng.integers(B), rng.integers(V), rng.integers(T)
        d[b, v, n], hit[b, v, n] = bad[k % 5], True
    d[0, :, 7] = np.nan                                                                 # every voice of one sample: the dry path alone
    hit[0, :, 7] = True
    y = ops.variable_delay(_dev(x), _dev(d), GAINS[:V], dry=DRY, filter_len=filter_len)
    assert torch.isfinite(y).all()
    assert not do.live_mask(d, T, filter_len)[hit].any()
    _check(f"guards taps={filter_len}", y, do.truth(x, d, GAINS[:V], DRY, filter_len), do.reference(x, d, GAINS[:V], DRY, filter_len))
    assert float(y[0, 7]) == DRY[0] * x[0, 7]
    one = np.where(hit[:, :1], d[:, :1], 4.5)                                           # one voice, nothing dry: exact zeros at the hits
    y1 = ops.variable_delay(_dev(x[:2]), _dev(one[:2]), 1.0, filter_len=filter_len).cpu().numpy()
    assert not y1[hit[:2, 0]].any() and np.count_nonzero(y1[~hit[:2, 0]]) > T
    allbad = np.full((B, V, T), np.nan)
    assert torch.equal(ops.variable_delay(_dev(x), _dev(allbad), GAINS[:V], dry=1.0), _dev(x))     # a tile without a live lane


# ----------------------------------------------------------------------------- physics
@pytest.mark.parametrize("eps", [0.01, -0.03])
def test_a_constant_speed_ramp_scales_a_sinusoids_frequency(eps):
    """Within 2 INTERP_ERR of the analytic sinusoid over the interior; INTERP_ERR (4.15e-6) is the oracle's own figure measured on
    the CPU (tests/test_delay_oracle.py), ten orders of magnitude above the float64 noise the factor 2 leaves room for."""
    x, d, want, interior = do.ramp_case(eps)
    y = _ops().variable_delay(_dev(x[None]), _dev(d[None]), filter_len=81)[0].cpu().numpy()
    err = float(np.max(np.abs(y - want)[interior]))
    print(f"eps={eps}: device error {err:.4e}, INTERP_ERR {do.INTERP_ERR[eps]:.4e}")
    assert err <= 2.0 * do.INTERP_ERR[eps]


# ----------------------------------------------------------------------------- the comb
CORNERS = {"feedback_echo": (1.0, 0.0, 0.6), "feed_forward": (0.8, -0.5, 0.0), "allpass": (-0.7, 1.0, 0.7)}


@pytest.mark.parametrize("corner", list(CORNERS))
@pytest.mark.parametrize("T", [1, 257, 4099])
def test_comb_is_the_numpy_restatement_bit_for_bit(T, corner):
    ops = _ops()
    b0, bD, aD = CORNERS[corner]
    x = do.signal(T, seed=T, B=2)
    x32 = x.astype(np.float32)
    for D_ in (1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 5):
        if D_ < 1:
            continue
        want = do.comb_reference(x, D_, b0, bD, aD)
        y = ops.comb(_dev(x), D_, b0, bD, aD)
        assert y.dtype == torch.float64 and np.array_equal(y.cpu().numpy(), want), (T, D_)
        want32 = do.comb_reference(x32.astype(np.float64), D_, b0, bD, aD)
        y32 = ops.comb(_dev(x32, torch.float32), D_, b0, bD, aD)
        assert y32.dtype == torch.float32 and np.array_equal(y32.cpu().numpy(), want32.astype(np.float32)), (T, D_)
        assert np.array_equal(ops.comb(_dev(x32, torch.float32), D_, b0, bD, aD, out_dtype=torch.float64).cpu().numpy(), want32)


@pytest.mark.parametrize("T", [257, 4099])
def test_comb_rows_with_their_own_parameters_and_alone(T):
    ops = _ops()
    x = do.signal(T, seed=2, B=B)
    D_, b0, bD, aD = [1, 64, 257, T - 1, T + 5], [1.0, 0.8, -0.7, 0.5, 1.0], [0.0, -0.5, 1.0, 0.25, 0.3], [0.6, 0.0, 0.7, -0.9, 0.99]
    want = do.comb_reference(x, D_, b0, bD, aD)
    y = ops.comb(_dev(x), D_, b0, bD, aD)
    assert np.array_equal(y.cpu().numpy(), want)
    assert torch.equal(ops.comb(_dev(x), torch.tensor(D_), torch.tensor(b0, dtype=torch.float64), np.array(bD), torch.tensor(aD, dtype=torch.float64)), y)
    for b in range(B):
        assert torch.equal(ops.comb(_dev(x[b:b + 1]), D_[b], b0[b], bD[b], aD[b])[0], y[b]), b
    mixed = ops.comb(_dev(x), D_, 1.0, 0.0, 0.5)                                        # one per row beside numbers
    assert np.array_equal(mixed.cpu().numpy(), do.comb_reference(x, D_, 1.0, 0.0, 0.5))


# ----------------------------------------------------------------------------- the fronts
@pytest.mark.parametrize("shape", [(900,), (3, 900), (2, 1, 900)], ids=str)
@pytest.mark.parametrize("where", ["host", "device"])
def test_functional_fronts_are_the_ops_calls_they_document(shape, where):
    from musicfpaugment_amd import functional as F
    ops = _ops()
    dev = DEV if where == "device" else torch.device("cpu")
    n, T, sr = int(np.prod(shape[:-1])), shape[-1], 8000
    for dtype in (torch.float64, torch.float32):
        w = torch.from_numpy(do.signal(T, seed=len(shape), B=n).reshape(shape)).to(dtype).to(dev)
        rows = w.reshape(-1, T).to(DEV)

        def same(y, want):
            assert y.device == w.device and y.dtype == dtype and y.shape == w.shape
            assert torch.equal(y.reshape(-1, T).to(DEV), want)

        delays = torch.tensor([[10.0 * 8.0, 20.5 * 8.0]], dtype=torch.float64, device=DEV).expand(n, 2)
        same(F.echo(w, sr, [10.0, 20.5], [0.5, 0.25], 0.9, 0.8), ops.variable_delay(rows, delays, [0.8 * 0.5, 0.8 * 0.25], dry=0.8 * 0.9))
        same(F.echo(w, sr, 10.0, 0.5), ops.variable_delay(rows, delays[:, :1], [0.5], dry=1.0))
        same(F.comb(w, sr, 5.0, 0.5, 0.25, -0.5), ops.comb(rows, 40, 0.5, 0.25, -0.5))
        same(F.feedback_echo(w, sr, 5.0, 0.6), ops.comb(rows, 40, 1.0, 0.0, 0.6))
        same(F.feedback_echo(w, sr, 5.0, 0.6, mix=0.25), ops.comb(rows, 40, 1.0, -(1.0 - 0.25) * 0.6, 0.6))
        same(F.allpass_comb(w, sr, 5.0, 0.7), ops.comb(rows, 40, -0.7, 1.0, 0.7))
        same(F.vibrato(w, sr), ops.variable_delay(rows, ops.lfo_delay(n, T, sr, base_ms=1.0, depth_ms=1.0, rate_hz=5.0)))
        cd = torch.stack([ops.lfo_delay(n, T, sr, base_ms=20.0, depth_ms=2.0, rate_hz=0.8, phase=2.0 * np.pi * v / 3) for v in range(3)], 1)
        same(F.chorus(w, sr), ops.variable_delay(rows, cd, 0.5 / 3, dry=0.5))
        same(F.flanger(w, sr), ops.variable_delay(rows, ops.lfo_delay(n, T, sr, base_ms=2.0, depth_ms=1.0, rate_hz=0.5), 0.7, dry=1.0))
        same(F.wow_flutter(w, sr, phase=(0.3, 1.0)),
             ops.variable_delay(rows, ops.speed_drift_delay(n, T, sr, [(0.002, 0.8, 0.3), (0.0008, 8.0, 1.0)])))
        same(F.wow_flutter(w, sr, wow_depth=0.0, flutter_depth=0.0), rows)              # no drift: the input's bits


def test_delay_builders_agree_with_numpy():
    ops = _ops()
    n, T, sr = 3, 16000, 8000
    a = ops.lfo_delay(n, T, sr, base_ms=[20.0, 5.0, 1.0], depth_ms=2.0, rate_hz=[0.8, 5.0, 0.3], phase=torch.tensor([0.0, 1.0, -2.0]))
    want = do.lfo_delay(n, T, sr, [20.0, 5.0, 1.0], 2.0, [0.8, 5.0, 0.3], [0.0, 1.0, -2.0])
    assert a.dtype == torch.float64 and a.shape == (n, T) and a.is_cuda and np.max(np.abs(a.cpu().numpy() - want)) < 1e-9
    comps = [([0.002, 0.004, 0.0005], [0.8, 0.3, 2.0], [0.0, 1.0, 2.0]), (0.0008, [8.0, 12.0, 5.0], 0.5), (0.0, 3.0, 0.0), (0.001, 0.0, 0.0)]
    b = ops.speed_drift_delay(n, T, sr, comps)
    assert b.dtype == torch.float64 and b.shape == (n, T) and np.max(np.abs(b.cpu().numpy() - do.speed_drift_delay(n, T, sr, comps))) < 1e-9
    assert not b[:, 0].any() and not ops.speed_drift_delay(n, T, sr, []).any()


def test_wow_keeps_the_mean_frequency_over_whole_periods():
    """Wow alone at 2 Hz, depth 0.002, on 1 kHz at 8 kHz: the delay returns to 0 after every 4000 samples, so the frequency taken
    from the interpolated upward zero crossings between sample 100 and sample 100 + 3 * 4000 is the input's to 1e-4 (the window's
    ends sit within one cycle of whole periods: 8 samples of at most 0.2 % deviation in 12000)."""
    from musicfpaugment_amd import functional as F
    T = 12400
    x = np.sin(2.0 * np.pi * 1000.0 * np.arange(T) / 8000.0 + 0.1)
    y = F.wow_flutter(_dev(x), 8000, wow_hz=2.0, wow_depth=0.002, flutter_depth=0.0).cpu().numpy()
    assert np.max(np.abs(y - x)) > 0.1                                                   # it did move the samples

    def frequency(s, lo, hi):
        k = np.nonzero((s[:-1] < 0.0) & (s[1:] >= 0.0))[0]
        t = k + s[k] / (s[k] - s[k + 1])
        a, b = np.searchsorted(t, lo), np.searchsorted(t, hi)
        return (b - a) / (t[b] - t[a]) * 8000.0
    assert abs(frequency(x, 100.0, 12100.0) / 1000.0 - 1.0) < 1e-6
    assert abs(frequency(y, 100.0, 12100.0) / 1000.0 - 1.0) < 1e-4
    assert abs(frequency(y, 100.0, 1900.0) / 1000.0 - 1.0) > 5e-4                        # inside a half period the pitch does move


def _transforms(p: float):
    from musicfpaugment_amd.augmentation.transformations.delay_effects import Chorus, Echo, WowFlutter
    return [Echo(min_delay_ms=5.0, max_delay_ms=40.0, p=p, sample_rate=8000), Echo(min_delay_ms=5.0, max_delay_ms=40.0, feedback=True, p=p, sample_rate=8000),
            WowFlutter(p=p, sample_rate=8000), Chorus(p=p, sample_rate=8000)]


@pytest.mark.parametrize("p", [1.0, 0.5, 0.0])
def test_transforms_are_the_ops_calls_on_their_draws(p):
    from musicfpaugment_amd.augmentation.transformations.delay_effects import Chorus, Echo, WowFlutter
    ops = _ops()
    x = torch.from_numpy(do.signal(2100, seed=2, B=4)).float().to(DEV)
    seen = set()
    for i, t in enumerate(_transforms(p)):
        random.seed(7 + i)
        torch.manual_seed(7 + i)
        out = t(x.unsqueeze(1))
        should = t.transform_parameters["should_apply"]
        assert out.samples.shape == (4, 1, 2100) and out.sample_rate == 8000
        tp = {k: v.tolist() for k, v in t.transform_parameters.items() if k != "should_apply"}                # the selected examples' draws
        assert all(len(v) == int(should.sum()) for v in tp.values())
        y = out.samples[:, 0]
        assert torch.equal(y[~should], x[~should])                                                           # unselected: the input's bits
        for b in torch.nonzero(should)[:, 0].tolist():                                                       # selected: every row changed
            assert not torch.equal(y[b], x[b]), (type(t).__name__, b)
        if isinstance(t, Echo):
            assert sorted(tp) == ["decay", "delay_ms"] and all(5.0 <= v <= 40.0 for v in tp["delay_ms"]) and all(0.2 <= v <= 0.6 for v in tp["decay"])
            ds, dc = t.delay_samples(8000), t.decay.double().numpy()
            want = ops.comb(x, ds, 1.0, 0.0, dc, apply=should) if t.feedback else ops.variable_delay(x, ds[:, None], dc[:, None], dry=1.0, apply=should)
        elif isinstance(t, WowFlutter):
            assert sorted(tp) == ["flutter_depth", "flutter_hz", "flutter_phase", "wow_depth", "wow_hz", "wow_phase"]
            want = ops.variable_delay(x, ops.speed_drift_delay(4, 2100, 8000, t.components()), apply=should)
        else:
            assert isinstance(t, Chorus) and sorted(tp) == ["depth_ms", "rate_hz", "voices"] and all(2 <= v <= 4 for v in tp["voices"])
            d = t.delays(2100, 8000, DEV)
            assert d.shape == (4, 4, 2100) and torch.equal(torch.isinf(d[:, :, 0]).sum(1).cpu(), 4 - t.voices)
            want = ops.variable_delay(x, d, t.voice_gains(), dry=0.5, apply=should)
            b = 0                                                                                             # an example's own voices alone give its row
            nv = int(t.voices[b])
            if should[b]:
                assert torch.equal(ops.variable_delay(x[b:b + 1], d[b:b + 1, :nv], t.voice_gains()[b:b + 1, :nv], dry=0.5)[0], y[b])
        assert torch.equal(y, want)
        t.freeze_parameters(seed=3)                                                                          # frozen: the same draws again
        a = t(x.unsqueeze(1)).samples
        t.freeze_parameters(seed=3)
        assert torch.equal(t(x.unsqueeze(1)).samples, a)
        seen |= set(should.tolist())
    assert seen == ({True} if p == 1.0 else {False} if p == 0.0 else {True, False})
    if p == 0.0:
        for t in _transforms(0.0):
            assert torch.equal(t(x.unsqueeze(1)).samples[:, 0], x)


def test_transforms_run_inside_compose_someof_and_oneof():
    from musicfpaugment_amd.augmentation.composition import Compose, OneOf, SomeOf
    ops = _ops()
    x = torch.from_numpy(do.signal(2100, seed=4, B=4)).float().to(DEV)
    ts = _transforms(0.7)
    random.seed(1)
    torch.manual_seed(1)
    out = Compose(ts)(x.unsqueeze(1), 8000)
    y = x
    for t in ts:                                                                        # the stages by hand on the draws they report
        should = t.transform_parameters["should_apply"]
        if hasattr(t, "feedback"):
            ds, dc = t.delay_samples(8000), t.decay.double().numpy()
            y = ops.comb(y, ds, 1.0, 0.0, dc, apply=should) if t.feedback else ops.variable_delay(y, ds[:, None], dc[:, None], dry=1.0, apply=should)
        elif hasattr(t, "components"):
            y = ops.variable_delay(y, ops.speed_drift_delay(4, 2100, 8000, t.components()), apply=should)
        else:
            y = ops.variable_delay(y, t.delays(2100, 8000, DEV), t.voice_gains(), dry=0.5, apply=should)
    assert torch.equal(out.samples[:, 0], y)
    chain = Compose([SomeOf((1, 2), _transforms(1.0)), OneOf(_transforms(1.0)[:3])])
    got = chain(x.unsqueeze(1), 8000).samples
    assert got.shape == (4, 1, 2100) and torch.isfinite(got).all() and not torch.equal(got[:, 0], x)
