"""GPU: csrc/loudness.hip against tests/_loudness_oracle.py BIT FOR BIT -- segment energies and peaks, the gate with its counts, block
powers and rank powers, the gain -- then the conformance signals of ITU-R BS.1770, EBU Tech 3341 and EBU Tech 3342 on the device
within the documents' tolerances, ops.true_peak, and the fronts: functional.loudness and LoudnessNormalization.

Readings seen on the device: DESIGN.md section 3.21."""
import functools

import numpy as np
import pytest
import torch

from tests import _iir_oracle as io
from tests import _loudness_oracle as o

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ROWS = 5
LENGTHS = (1, 15, 16, 17, 1023, 1024, 1025, 2049, 3089)
T_MAX = LENGTHS[-1]
SURROUND = [1.0, 1.0, 1.0, 1.41, 1.41]


def _ops():
    from musicfpaugment_amd import ops
    return ops


def _sos(rate, design="bs1770"):
    from musicfpaugment_amd.functional import k_weighting_sos
    return k_weighting_sos(rate, design)


def _sections(name):
    if name == "unweighted":
        return None
    if name in ("k8k", "k48k"):
        return _sos(8000 if name == "k8k" else 48000)
    F = io.filters()
    if name == "peak50":
        return F["peak50_q8_8k"]
    return np.concatenate([io.seven_bands(8000), F["peak50_q8_8k"]])          # eight sections, low-frequency ones among them


def _hops(T):
    return sorted({1, 3, 16, 17, 512, 1024, 1025, 2500, T, T + 1})


@functools.lru_cache(maxsize=None)
def _signal(dtype) -> np.ndarray:
    x = np.random.default_rng(21).uniform(-1.0, 1.0, (ROWS, T_MAX))
    return x.astype(np.float32) if dtype == "float32" else x


def _dev(x: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _same(a, b) -> bool:
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("name", ["unweighted", "peak50", "k8k", "k48k", "eight"])
def test_segments_and_peak_bit_for_bit(name, dtype):
    ops, sos = _ops(), _sections(name)
    for T in LENGTHS:
        x = _signal(dtype)[:, :T]
        filtered = [o.restate_filtered(row, sos) for row in x]
        for hop in _hops(T):
            seg, peak = ops.loudness_segments(_dev(x), sos, hop, return_peak=True)
            seg, peak = seg.cpu().numpy(), peak.cpu().numpy()
            assert seg.shape == (ROWS, T // hop) and seg.dtype == np.float64 and peak.shape == (ROWS,)
            for r in range(ROWS):
                want_seg, want_peak = o.restate_segments(x[r], sos, hop, y=filtered[r])
                assert _same(seg[r], want_seg), (T, hop, r)
                assert peak[r] == want_peak == np.max(np.abs(x[r].astype(np.float64)))
            one, one_peak = ops.loudness_segments(_dev(x[3:4]), sos, hop, return_peak=True)      # a row's bits do not depend on R or on its position
            assert _same(one.cpu().numpy()[0], seg[3]) and one_peak.item() == peak[3]


def test_segments_of_examples_without_peak_and_a_nan_sample():
    ops, sos = _ops(), _sos(8000)
    x = _signal("float32")[:4, :2049].reshape(2, 2, 2049).copy()
    seg = ops.loudness_segments(_dev(x), sos, 800)
    assert seg.shape == (2, 2, 2)
    for b in range(2):
        for c in range(2):
            assert _same(seg[b, c].cpu().numpy(), o.restate_segments(x[b, c], sos, 800)[0])
    x[1, 0, 900] = np.nan                                                      # the peak skips it; the filter carries it on
    seg, peak = ops.loudness_segments(_dev(x), sos, 800, return_peak=True)
    want_seg, want_peak = o.restate_segments(x[1, 0], sos, 800)
    assert _same(seg[1, 0].cpu().numpy(), want_seg) and np.isnan(want_seg[1]) and not np.isnan(want_seg[0])
    assert peak[1, 0].item() == want_peak == np.nanmax(np.abs(x[1, 0]))


def _programme(seed: int, C: int, nseg: int, hop: int, levels) -> np.ndarray:
    rng = np.random.default_rng(seed)
    runs = rng.integers(31, 45, size=nseg // 31 + 1)                            # stretches longer than the longest block, the levels in turn
    level = np.repeat(np.resize(levels, len(runs)), runs)[:nseg]
    return hop * level[None, :] * rng.uniform(0.5, 1.5, (C, nseg))


def _gate_rows(C: int, nseg: int, hop: int) -> np.ndarray:
    """(5, C, nseg): all zero, below the absolute gate throughout, partly gated, cut by the relative gate only, holding a NaN."""
    rows = [np.zeros((C, nseg)), _programme(1, C, nseg, hop, [1e-9, 3e-9]), _programme(2, C, nseg, hop, [1e-9, 3e-5, 1e-3, 0.02, 0.3]),
            _programme(3, C, nseg, hop, [1e-4, 0.3]), _programme(4, C, nseg, hop, [1e-9, 1e-3, 0.3])]
    if nseg:
        rows[4][C - 1, nseg // 2] = np.nan
    return np.stack(rows)


@pytest.mark.parametrize("C", [1, 2, 5])
@pytest.mark.parametrize("win,rel", [(1, 0.1), (4, 0.1), (30, 0.01)])
def test_gate_bit_for_bit(win, rel, C):
    ops, hop = _ops(), 800
    weights = SURROUND if C == 5 else None
    seen = np.zeros(3, dtype=bool)
    for nseg in (0, win - 1, win, win + 1, 65, 300):
        seg = _gate_rows(C, nseg, hop)
        got = ops.loudness_gate(_dev(seg), hop, win=win, rel=rel, weights=weights, return_blocks=True, want_range=True)
        plain = ops.loudness_gate(_dev(seg), hop, win=win, rel=rel, weights=weights)               # the instantiation without the sort
        assert plain.blocks is None and plain.range is None
        nb = max(0, nseg - win + 1)
        assert got.blocks.shape == (5, nb) and got.range.shape == (5, 2)
        for b in range(5):
            want = o.restate_gate(seg[b], hop, win, rel, weights)
            for g in (got, plain):
                assert (g.n_abs[b].item(), g.n_rel[b].item()) == (want["n_abs"], want["n_rel"]), (nseg, b)
                assert g.power[b].item() == want["power"] and g.abs_power[b].item() == want["abs_power"], (nseg, b)
            assert _same(got.blocks[b].cpu().numpy(), want["blocks"])
            assert (got.range[b, 0].item(), got.range[b, 1].item()) == (want["lo"], want["hi"]), (nseg, b)
            if b < 2:
                assert want["n_rel"] == 0 and want["power"] == 0.0
            if nseg == 300:
                seen |= [b == 2 and 0 < want["n_abs"] < nb, b == 3 and want["n_rel"] < want["n_abs"] == nb,
                         b == 4 and np.isnan(want["blocks"]).any() and want["n_rel"] > 0]
    assert seen.all(), seen                                                     # the cases take the decisions they are named for


def test_gate_ranks_at_the_cap_and_refusal_above_it():
    ops, hop = _ops(), 800
    cap = ops.LOUDNESS_MAX_RANGE_BLOCKS
    seg = hop * np.random.default_rng(9).uniform(1e-4, 1.0, (2, 1, cap + 4))
    seg[1, 0, 5000:] = 0.0                                                     # the sort pads this example's gated-off blocks
    for win, rel in ((4, 0.01), (1, 0.5)):
        s = seg[:, :, :cap + win - 1]
        got = ops.loudness_gate(_dev(s), hop, win=win, rel=rel, want_range=True)
        for b in range(2):
            want = o.restate_gate(s[b], hop, win, rel)
            assert (got.n_abs[b].item(), got.n_rel[b].item()) == (want["n_abs"], want["n_rel"]) and want["n_rel"] > 1000
            assert got.power[b].item() == want["power"]
            assert (got.range[b, 0].item(), got.range[b, 1].item()) == (want["lo"], want["hi"]) and want["lo"] < want["hi"]
    with pytest.raises(ValueError):
        ops.loudness_gate(_dev(seg[:, :, :cap + 4]), hop, win=4, want_range=True)
    assert ops.loudness_gate(_dev(seg[:, :, :cap + 4]), hop, win=4).power.shape == (2,)          # without ranks there is no cap


@functools.lru_cache(maxsize=None)
def _examples(dtype) -> np.ndarray:
    """(6, 2, 12000) at 8 kHz: five levels and one silent example."""
    rng = np.random.default_rng(33)
    x = rng.uniform(-1.0, 1.0, (6, 2, 12000)) * np.array([0.5, 0.05, 0.0, 0.2, 0.01, 0.3])[:, None, None]
    return x.astype(np.float32) if dtype == "float32" else x


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_gain_bit_for_bit(dtype):
    ops, fs = _ops(), 8000
    x = _examples(dtype)
    xd = _dev(x)
    targets = np.array([2.0, -14.0, -20.0, -30.5, -16.0, 0.0])                 # the first and the last would leave above 0.9
    apply = [True, True, True, True, False, True]
    seg, peak = ops.loudness_segments(xd, _sos(fs), 800, return_peak=True)
    gated = ops.loudness_gate(seg, 800).power.cpu().numpy()
    assert gated[2] == 0.0 and np.all(gated[[0, 1, 3, 4, 5]] > 0)
    p_target = ops.loudness_power(targets)
    for limit in (None, 0.9):
        y, g = ops.loudness_normalize(xd, fs, targets, peak_limit=limit, apply=apply, return_gain=True)
        want_y, want_g = o.restate_gain(x, gated, p_target, peak.cpu().numpy(), limit, apply)
        assert y.dtype == xd.dtype and y.shape == xd.shape
        assert _same(g.cpu().numpy(), want_g) and _same(y.cpu().numpy(), want_y)
        assert torch.equal(y[2], xd[2]) and torch.equal(y[4], xd[4])           # silent, and gated off: the input itself
        free = np.sqrt(p_target / np.where(gated > 0, gated, 1.0))
        binds = want_g < free
        assert (binds[[0, 1, 3, 5]].any() and not binds[[0, 1, 3, 5]].all()) if limit else not binds[[0, 1, 3, 5]].any()
        if limit:
            assert y.abs().amax().item() <= limit * (1 + 1e-7)
    if dtype == "float32":                                                     # the float64 result rounded once
        y64 = ops.loudness_normalize(xd.double(), fs, targets, apply=apply)
        assert torch.equal(ops.loudness_normalize(xd, fs, targets, apply=apply), y64.float())


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_normalized_examples_read_their_targets(dtype):
    ops, fs = _ops(), 8000
    xd = _dev(_examples(dtype))
    targets = np.array([-23.0, -14.0, -20.0, -30.5, -16.0, -27.0])
    y = ops.loudness_normalize(xd, fs, targets)
    got = ops.loudness(y, fs).cpu().numpy()
    print(dtype, got - targets)
    live = [0, 1, 3, 4, 5]
    assert np.max(np.abs(got[live] - targets[live])) <= 1e-6 and got[2] == -np.inf
    one = ops.loudness_normalize(xd[:, 0], fs, -18.0)                          # (B, T) is one channel
    assert one.shape == xd[:, 0].shape and np.max(np.abs(ops.loudness(one, fs).cpu().numpy()[live] + 18.0)) <= 1e-6


def _f32(x: np.ndarray) -> torch.Tensor:
    return _dev(x.astype(np.float32)[None])


def test_bs1770_full_scale_sine_on_the_device():
    ops = _ops()
    for rate in (48000, 44100, 8000):
        got = ops.loudness(_f32(o.sine(997.0, rate, 20.0, 0.0)), rate).item()
        print(f"997 Hz, 0 dBFS, {rate} Hz: {got:.4f} LUFS")
        assert abs(got + 3.01) <= 0.05


def test_ebu_tech_3341_on_the_device():
    ops = _ops()
    for case, (parts, want) in sorted(o.TECH_3341.items()):
        got = ops.loudness(_f32(o.steps(48000, parts)), 48000).item()
        print(f"Tech 3341 case {case}: {got:.4f} LUFS")
        assert abs(got - want) <= 0.1


def test_ebu_tech_3342_on_the_device():
    ops = _ops()
    for case, (parts, want) in sorted(o.TECH_3342.items()):
        got = ops.loudness_range(_f32(o.steps(48000, parts)), 48000).item()
        print(f"Tech 3342 case {case}: {got:.4f} LU")
        assert abs(got - want) <= 1.0


def test_curves_and_short_inputs():
    ops, fs = _ops(), 8000
    x = _f32(o.sine(997.0, fs, 5.0, -20.0, channels=2))
    m, s = ops.loudness_curve(x, fs), ops.loudness_curve(x, fs, "short")
    assert m.shape == (1, 47) and s.shape == (1, 21) and m.dtype == torch.float64
    want = o.lufs_of(2 * 0.5 * 10.0 ** (-20.0 / 10.0)) + 20.0 * np.log10(abs(_k_gain(fs, 997.0)))
    assert torch.all((m[:, 2:] - want).abs() < 0.01) and torch.all((s - want).abs() < 0.01)
    short = ops.loudness(x[:, :, :3000], fs)                                   # less than one block: nothing to gate
    assert short.item() == -np.inf and ops.loudness_range(x[:, :, :3000], fs).item() == 0.0
    assert ops.loudness_curve(x[:, :, :3000], fs).shape == (1, 0)


def _k_gain(fs, f):
    import scipy.signal
    return scipy.signal.sosfreqz(_sos(fs), worN=[f], fs=fs)[1][0]


def test_true_peak_between_the_samples():
    ops, fs = _ops(), 48000
    n = np.arange(fs)
    x = _dev((0.5 * np.sin(2.0 * np.pi * (fs / 4) * n / fs + np.pi / 4)).astype(np.float32)[None])
    sample_peak = 20.0 * np.log10(x.abs().amax().item())
    tp = ops.true_peak(x)
    assert tp.shape == (1,)
    true_peak = 20.0 * np.log10(tp.item())
    print(f"sample peak {sample_peak:.3f} dBFS, true peak {true_peak:.3f} dBTP")
    assert abs(sample_peak + 9.03) < 0.01 and -6.0 - 0.4 <= true_peak <= -6.0 + 0.2
    assert ops.true_peak(x[:, None, :].expand(1, 2, fs)).shape == (1, 2)


def test_functional_fronts():
    from musicfpaugment_amd import functional as F
    ops, fs = _ops(), 8000
    x = torch.from_numpy(np.random.default_rng(4).uniform(-0.3, 0.3, (2, 3, 2, 9000)).astype(np.float32))
    got = F.loudness(x, fs)
    assert got.shape == (2, 3) and got.dtype == torch.float64 and not got.is_cuda
    want = ops.loudness(x.to(DEV).reshape(6, 2, 9000), fs).reshape(2, 3).cpu()
    assert torch.equal(got, want) and torch.all(torch.isfinite(got))
    assert torch.equal(F.loudness(x.to(DEV), fs).cpu(), want)
    y = F.loudness_normalize(x, fs, -23.0)
    assert y.shape == x.shape and y.dtype == x.dtype and torch.all((F.loudness(y, fs) + 23.0).abs() <= 1e-6)
    assert F.loudness_range(x, fs).shape == (2, 3)
    ta = ops.loudness(x.to(DEV).reshape(6, 2, 9000), fs, design="torchaudio").reshape(2, 3).cpu()
    assert torch.all((ta - want).abs() < 0.5) and not torch.equal(ta, want)
    w = ops.loudness(x.to(DEV).reshape(6, 2, 9000), fs, weights=[1.0, 0.0]).reshape(2, 3).cpu()
    assert torch.equal(w, ops.loudness(x.to(DEV).reshape(6, 2, 9000)[:, :1].contiguous(), fs).reshape(2, 3).cpu())


def test_loudness_normalization_transform_in_a_compose():
    from musicfpaugment_amd.augmentation.composition import Compose
    from musicfpaugment_amd.augmentation.transformations.loudness import LoudnessNormalization
    ops, fs = _ops(), 8000
    x = _dev(np.random.default_rng(6).uniform(-0.4, 0.4, (12, 1, 10000)).astype(np.float32))
    torch.manual_seed(3)
    t = LoudnessNormalization(p=0.5)
    out = Compose([t])(x, sample_rate=fs)
    y, should = out.samples, t.transform_parameters["should_apply"]
    assert out.sample_rate == fs and y.shape == x.shape and y.dtype == torch.float32
    assert 0 < int(should.sum()) < 12
    assert torch.equal(y[~should], x[~should])                                 # unselected examples: the input itself
    got = ops.loudness(y, fs).cpu().numpy()
    targets = t.targets()
    assert np.all(targets >= -31.0) and np.all(targets <= -13.0)
    assert np.max(np.abs(got[should.numpy()] - targets[should.numpy()])) <= 1e-6
    assert not torch.equal(y[should], x[should])
