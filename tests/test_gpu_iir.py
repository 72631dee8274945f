"""GPU: csrc/iir.hip (ops.sosfilt) against the long-double truth with scipy.signal.sosfilt's own error as the yardstick
(tests/_iir_oracle.py: D <= 8 E), bit for bit against the numpy restatement of the kernel, its exact cases, batch independence and
states, and the fronts over it: functional.lfilter / biquad / *_biquad and the equaliser transforms.

Worst D/E seen on the device (printed by every case): see DESIGN.md section 3.15."""
import functools
import random

import numpy as np
import pytest
import torch

from tests import _iir_oracle as io

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
B, T_MAX = 5, io.LENGTHS[-1]
SINGLES = ("peak50_q8_8k", "peak20_q4_44k", "lowpass1000_8k", "lowpass30_8k", "peak3900_q10_8k", "peak100_q07_8k")


def _ops():
    from musicfpaugment_amd import ops
    return ops


def _filters(S: int, per_row: bool):
    """name -> sections (S, 6), or with per_row (5, S, 6): five different filters for one launch."""
    F = io.filters()
    one = [F[n] for n in SINGLES]
    if S == 1:
        return {"five_singles": np.stack(one[:B])} if per_row else dict(zip(SINGLES, one))
    if S == 2:
        pairs = [np.concatenate([one[i], one[(i + 1) % 6]]) for i in range(6)]
        return {"five_pairs": np.stack(pairs[:B])} if per_row else {"peak50+peak20": pairs[0], "lowpass30+peak3900": pairs[3]}
    gains = np.array([6.0, -4.0, 3.0, -9.0, 12.0, -2.0, 5.0])
    eights = [np.concatenate([io.seven_bands(8000 if i % 2 == 0 else 44100, np.roll(gains, i)), one[i]]) for i in range(B)]
    return {"five_eights": np.stack(eights)} if per_row else {"seven_bands_8k+peak50": eights[0]}


@functools.lru_cache(maxsize=None)
def _signal() -> np.ndarray:
    return io.signal(T_MAX, seed=11, B=B)


@functools.lru_cache(maxsize=None)
def _wanted(S: int, per_row: bool, name: str):
    """(truth, reference) of the five rows at the longest length, once: a causal filter's output over a prefix is the prefix of its
    output, and row b filtered alone is row b of the batch."""
    sos = _filters(S, per_row)[name]
    return io.truth(_signal(), sos)[0], io.reference(_signal(), sos)[0]


def _dev(x: np.ndarray, dtype=torch.float64) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).to(DEV)


@pytest.mark.parametrize("per_row", [False, True], ids=["shared", "per_row"])
@pytest.mark.parametrize("rows", [1, B])
@pytest.mark.parametrize("S", [1, 2, 8])
def test_float64_within_eight_of_scipys_errors(S, rows, per_row):
    ops = _ops()
    for name, sos in _filters(S, per_row).items():
        t, r = _wanted(S, per_row, name)
        for T in io.LENGTHS:
            y = ops.sosfilt(_dev(_signal()[:rows, :T]), sos[:rows] if per_row else sos).cpu().numpy()
            D, E = io.errors(y, None, None, want=(t[:rows, :T], r[:rows, :T]))
            print(f"S={S} B={rows} {name} T={T}: D={D:.3e} E={E:.3e} D/E={D / E:.2f}")
            assert E > 0 and D <= io.BOUND * E, (name, T, D, E)


@pytest.mark.parametrize("S,per_row", [(1, True), (8, True), (2, False)])
def test_device_is_the_numpy_restatement_bit_for_bit(S, per_row):
    """The kernel is built without fused multiply-adds and tests/_iir_oracle.py restates its order of operations: same bits, states
    included."""
    ops = _ops()
    (name, sos), = list(_filters(S, per_row).items())[:1]
    zi = np.random.default_rng(5).uniform(-1.0, 1.0, (B, S, 2))
    for T in (1, io.L + 1, io.SUPER - 1, io.SUPER + 1, 2 * io.SUPER + 17):
        x = _signal()[:, :T]
        y, zf = ops.sosfilt(_dev(x), sos, zi=_dev(zi))
        for b in range(B):
            wy, wz = io.restate(x[b], sos[b] if per_row else sos, zi[b])
            assert np.array_equal(y[b].cpu().numpy(), wy) and np.array_equal(zf[b].cpu().numpy(), wz), (name, T, b)


@pytest.mark.parametrize("T", [1, io.L, io.SUPER + 1, T_MAX])
def test_float32_is_the_float64_result_rounded_once(T):
    ops = _ops()
    x32 = _dev(_signal()[:, :T], torch.float32)
    for S, per_row in ((1, True), (8, False)):
        (sos,) = list(_filters(S, per_row).values())[:1]
        assert torch.equal(ops.sosfilt(x32, sos), ops.sosfilt(x32.double(), sos).float())
        assert torch.equal(ops.sosfilt(x32, sos, clamp=True), ops.sosfilt(x32.double(), sos, clamp=True).float())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("T", io.LENGTHS)
def test_exact_cases(T, dtype):
    ops = _ops()
    x = _dev(_signal()[:, :T], dtype)
    assert torch.equal(ops.sosfilt(x, io.IDENTITY), x)                                         # the identity section: the input
    assert torch.equal(ops.sosfilt(x, np.tile(io.IDENTITY, (8, 1))), x)
    xi = _dev(np.random.default_rng(T).integers(-1000, 1000, (B, T)).astype(np.float64), dtype)   # exact operands: scipy's output exactly
    fir = np.array([[0.5, -2.0, 0.25, 1.0, 0.0, 0.0], [3.0, 1.0, -0.5, 1.0, 0.0, 0.0]])
    want = io.reference(xi.cpu().numpy().astype(np.float64), fir)[0]
    assert np.array_equal(ops.sosfilt(xi, fir).cpu().numpy(), want.astype(xi.cpu().numpy().dtype))
    (sos,) = _filters(2, True).values()
    gate = torch.tensor([True, False, True, False, False])
    y, gated = ops.sosfilt(x, sos), ops.sosfilt(x, sos, apply=gate)
    assert torch.equal(gated[~gate], x[~gate]) and torch.equal(gated[gate], y[gate])           # the gate: the input, or the ungated result
    assert torch.equal(ops.sosfilt(x, sos, apply=gate.to(DEV)), gated)
    loud = ops.sosfilt(x * 4, sos)
    assert torch.equal(ops.sosfilt(x * 4, sos, clamp=True), torch.clamp(loud, -1.0, 1.0)) and (T < 100 or float(loud.abs().max()) > 1.0)


@pytest.mark.parametrize("S,per_row", [(1, False), (1, True), (8, False), (8, True)])
def test_a_row_does_not_depend_on_its_batch(S, per_row):
    ops = _ops()
    (sos,) = list(_filters(S, per_row).values())[:1]
    for T in (io.L + 1, 2 * io.SUPER + 17):
        x = _dev(_signal()[:, :T], torch.float32)
        y = ops.sosfilt(x, sos)
        for b in range(B):
            assert torch.equal(ops.sosfilt(x[b:b + 1], sos[b:b + 1] if per_row else sos)[0], y[b]), (T, b)


@pytest.mark.parametrize("T", [io.SUPER, io.SUPER + 5, 2 * io.SUPER, 2 * io.SUPER + 17])
def test_final_states_and_streaming(T):
    """zf against scipy's with random initial states, five filters of eight sections in one launch (E over the 80 state values), and
    a signal filtered in two calls joined by the state against the one-shot truth, split at 64 L and 64 L + 5."""
    ops = _ops()
    (sos,) = _filters(8, True).values()
    x = _signal()[:, :T]
    zi = np.random.default_rng(T).uniform(-1.0, 1.0, (B, 8, 2))
    y, zf = ops.sosfilt(_dev(x), sos, zi=_dev(zi))
    (ty, tz), (ry, rz) = io.truth(x, sos, zi), io.reference(x, sos, zi)
    E, Es = float(np.max(np.abs(ry - ty))), float(np.max(np.abs(rz - tz)))
    D, Ds = float(np.max(np.abs(y.cpu().numpy() - ty))), float(np.max(np.abs(zf.cpu().numpy() - tz)))
    print(f"T={T}: output D/E={D / E:.2f}, state D/E={Ds / Es:.2f}")
    assert D <= io.BOUND * E and Ds <= io.BOUND * Es
    for n in (io.SUPER, io.SUPER + 5):
        if n < T:
            y0, z0 = ops.sosfilt(_dev(x[:, :n]), sos, zi=_dev(zi))
            y1, z1 = ops.sosfilt(_dev(x[:, n:]), sos, zi=z0)
            D2 = float(np.max(np.abs(torch.cat([y0, y1], 1).cpu().numpy() - ty)))
            Ds2 = float(np.max(np.abs(z1.cpu().numpy() - tz)))
            print(f"T={T} split at {n}: output D/E={D2 / E:.2f}, state D/E={Ds2 / Es:.2f}")
            assert D2 <= io.BOUND * E and Ds2 <= io.BOUND * Es


def _close_to_scipy(got: torch.Tensor, x: np.ndarray, sos, clamp: bool):
    """A front's output against scipy's in the project's convention; float32 fronts against the float64 result rounded once."""
    sos = io.normalized(sos)
    t, r = io.truth(x, sos)[0], io.reference(x, sos)[0]
    if clamp:
        t, r = np.clip(t, -1.0, 1.0), np.clip(r, -1.0, 1.0)
    assert got.shape == x.shape
    D, E = float(np.max(np.abs(got.double().cpu().numpy() - t))), float(np.max(np.abs(r - t)))
    if got.dtype == torch.float32:                                            # one rounding of a value within D of the truth
        E = E + float(np.max(np.abs(t))) * 2.0 ** -24 / io.BOUND
    assert D <= io.BOUND * E, (D, E)


@pytest.mark.parametrize("shape", [(700,), (3, 700), (2, 3, 700)], ids=str)
@pytest.mark.parametrize("where", ["host", "device"])
def test_functional_fronts_against_scipy(shape, where):
    from musicfpaugment_amd import functional as F
    x = np.random.default_rng(len(shape)).uniform(-1.0, 1.0, shape)
    dev = DEV if where == "device" else torch.device("cpu")
    for dtype in (torch.float64, torch.float32):
        w = torch.from_numpy(x).to(dtype).to(dev)
        xs = w.double().cpu().numpy()
        b, a = [0.3, -0.2, 0.1], [1.0, -1.6, 0.8]
        y = F.lfilter(w, a, b, clamp=False)
        assert y.device == w.device and y.dtype == dtype
        _close_to_scipy(y, xs, [b + a], False)
        _close_to_scipy(F.lfilter(w * 3, a, b), (w * 3).double().cpu().numpy(), [b + a], True)   # clamp=True is the default
        _close_to_scipy(F.lfilter(w, [2.0, -1.0], [1.0, 0.5], clamp=False), xs, [[1.0, 0.5, 0.0, 2.0, -1.0, 0.0]], False)
        _close_to_scipy(F.biquad(w, 0.6, -0.4, 0.2, 2.0, -3.2, 1.6), xs, [[0.6, -0.4, 0.2, 2.0, -3.2, 1.6]], True)
        _close_to_scipy(F.equalizer_biquad(w, 8000, 1000.0, 6.0, 2.0), xs, [F.biquad_coefficients("peaking", 8000, 1000.0, 2.0, 6.0)], True)
        _close_to_scipy(F.bass_biquad(w, 8000, -3.0), xs, [F.biquad_coefficients("lowshelf", 8000, 100.0, 0.707, -3.0)], True)
    if len(shape) >= 2:                                                                      # one filter per channel, and every filter on every row
        C = shape[-2]
        a2, b2 = [[1.0, -0.5 - 0.1 * c, 0.1] for c in range(C)], [[0.5, 0.1 * c, 0.0] for c in range(C)]
        w = torch.from_numpy(x).to(dev)
        y = F.lfilter(w, torch.tensor(a2, dtype=torch.float64), torch.tensor(b2, dtype=torch.float64), clamp=False)
        z = F.lfilter(w, a2, b2, clamp=False, batching=False)
        assert z.shape == shape[:-1] + (C, shape[-1])
        for c in range(C):
            _close_to_scipy(y[..., c, :], x[..., c, :], [b2[c] + a2[c]], False)
            _close_to_scipy(z[..., c, :], x, [b2[c] + a2[c]], False)


def _sections(t, sample_rate: int, n: int) -> np.ndarray:
    """The sections a transform's last call used, rebuilt from what it drew: the identity for a row its gate skipped."""
    from musicfpaugment_amd import functional as F
    from musicfpaugment_amd.augmentation.transformations.equalizer import ParametricEQ
    should = t.transform_parameters["should_apply"].tolist()
    if isinstance(t, ParametricEQ):
        return np.stack([t.band_sections(sample_rate, g) if s else np.tile(io.IDENTITY, (t.n_bands, 1)) for s, g in zip(should, t.gains_db.tolist())])
    return np.stack([F.biquad_coefficients(t.kind, sample_rate, f, q, g)[None] if s else io.IDENTITY
                     for s, f, g, q in zip(should, t.center_freq.tolist(), t.gain_db.tolist(), t.q.tolist())])


def _transforms(p: float):
    from musicfpaugment_amd.augmentation.transformations.equalizer import HighShelfFilter, LowShelfFilter, ParametricEQ, PeakingFilter
    return [LowShelfFilter(p=p, sample_rate=8000), PeakingFilter(p=p, sample_rate=8000), HighShelfFilter(p=p, sample_rate=8000),
            ParametricEQ(p=p, sample_rate=8000), ParametricEQ(n_bands=2, p=p, sample_rate=8000), ParametricEQ(n_bands=8, p=p, sample_rate=8000)]


@pytest.mark.parametrize("p", [1.0, 0.5])
def test_transforms_are_sosfilt_on_their_draws(p):
    ops = _ops()
    x = torch.from_numpy(io.signal(2100, seed=2, B=4)).float().to(DEV)
    seen = set()
    for i, t in enumerate(_transforms(p)):
        random.seed(7 + i)
        torch.manual_seed(7 + i)
        out = t(x.unsqueeze(1))
        should = t.transform_parameters["should_apply"]
        assert out.samples.shape == (4, 1, 2100) and out.sample_rate == 8000
        sos = _sections(t, 8000, 4)
        assert torch.equal(out.samples[:, 0], ops.sosfilt(x, sos, apply=should))
        assert torch.equal(out.samples[:, 0][~should], x[~should])
        if should.any():
            sel = torch.nonzero(should)[:, 0].to(DEV)
            assert torch.equal(out.samples[:, 0][should], ops.sosfilt(x[sel], sos[should.numpy()]))
            assert not torch.equal(out.samples[:, 0][should], x[should])
        seen |= set(should.tolist())
    assert seen == ({True} if p == 1.0 else {True, False})                                     # the seeds exercise both sides of the gate


def test_compose_is_the_three_stages_by_hand_and_a_bad_rate_is_refused():
    from musicfpaugment_amd.augmentation.composition import Compose, OneOf, SomeOf
    from musicfpaugment_amd.augmentation.transformations.equalizer import PeakingFilter
    ops = _ops()
    x = torch.from_numpy(io.signal(2100, seed=4, B=4)).float().to(DEV)
    ts = _transforms(0.7)[:3]
    random.seed(1)
    torch.manual_seed(1)
    out = Compose(ts)(x.unsqueeze(1), 8000)
    y = x
    for t in ts:
        y = ops.sosfilt(y, _sections(t, 8000, 4), apply=t.transform_parameters["should_apply"])
    assert torch.equal(out.samples[:, 0], y)
    chain = Compose([SomeOf((1, 2), _transforms(1.0)[:3]), OneOf(_transforms(1.0)[3:])])
    assert chain(x.unsqueeze(1), 8000).samples.shape == (4, 1, 2100)
    with pytest.raises(ValueError):
        PeakingFilter(p=1.0)(x.unsqueeze(1), 7600)                                            # max_center_freq 3800 Hz is the Nyquist frequency


def test_a_sinusoid_at_the_centre_gains_what_the_design_says():
    """1 kHz at 8 kHz through +6 dB at 1 kHz, Q 2: the poles have radius sqrt(a2) = 0.90, so after 512 samples the transient is below
    0.9^512 = 4e-24 of its start; over whole periods (8 samples) the RMS gain is 10^(6/20)."""
    from musicfpaugment_amd import functional as F
    n = np.arange(512 + 4096)
    x = 0.25 * np.sin(2.0 * np.pi * 1000.0 * n / 8000.0 + 0.3)
    y = F.equalizer_biquad(torch.from_numpy(x).to(DEV), 8000, 1000.0, 6.0, 2.0).cpu().numpy()
    gain = np.sqrt(np.mean(y[512:] ** 2) / np.mean(x[512:] ** 2))
    assert abs(gain - 10.0 ** (6.0 / 20.0)) <= 1e-6 * 10.0 ** (6.0 / 20.0), gain
