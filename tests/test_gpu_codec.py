"""GPU: csrc/codec.hip (ops.transform_codec, ops.mu_law and its halves) against tests/_codec_oracle.py, and the fronts over it: the
functional entries and the LossyCodec / TelephoneChannel transforms.

The codec's output and its water line are held against the long-double truth with the float64 definition's own error as the
yardstick (D <= 8 E, and the reference's bits where E == 0); every accuracy case prints its D/E.  The counts of coded coefficients
and the mu-law codes are integers and must be equal.  Every coded case keeps every discrete decision at least 1e-9 from its
threshold (tests/test_codec_oracle.py::test_margin_condition_of_every_gpu_case), so no frame and no sample is left out.

Shapes: T of (1, 255, 256, 257, 513, G 256 - 1, G 256 + 1, 2 G 256 + 1), G = MFPA_CODEC_FRAMES: the fold's edges, the last
partial frame, the seam between two workgroups and a third workgroup.

Worst D/E on one MI355X: lossless 1.00 (T = 1; 0.21 to 0.58 elsewhere); coded output and water line 3.16
(the water line of the two-tone signal at 16 kbit/s, T = 257, E = 1.4e-16), 2.12 on the impulse, at most 1.69 elsewhere; other band
tables 1.12; the mu-law decoder 1.00."""
import functools
import math
import os
import random
import re

import numpy as np
import pytest
import torch

from tests import _codec_oracle as co

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = int(re.search(r"#define MFPA_CODEC_FRAMES (\d+)", open(os.path.join(ROOT, "include", "mfpa.h")).read()).group(1))
LENGTHS = co.lengths(G)


def _ops():
    from musicfpaugment_amd import ops
    return ops


def _dev(a: np.ndarray, dtype=torch.float64) -> torch.Tensor:
    return torch.from_numpy(np.array(a, order="C")).to(dtype).to(DEV)


def _ratio(D, E):
    return "exact" if E == 0.0 and D == 0.0 else "inf" if E == 0.0 else format(D / E, ".2f")


def _check(tag: str, got, t: np.ndarray, r: np.ndarray) -> float:
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    D, E = co.errors(got, (t, r))
    print(f"{tag}: D={D:.3e} E={E:.3e} D/E={_ratio(D, E)}")
    if E == 0.0:
        assert np.array_equal(got, r), tag
    assert D <= co.BOUND * E, (tag, D, E)
    return D / E if E else 0.0


@functools.lru_cache(maxsize=None)
def _case(T: int):
    """name -> (x, kbps, truth, reference) of every coded case of length T, computed once and shared."""
    out = {}
    for name, x, kbps in co.coded_cases(T):
        x.setflags(write=False)
        out[name] = (x, kbps, co.truth(x, co.budget(kbps)), co.reference(x, co.budget(kbps)))
    return out


def _finite_lambda(lam):
    """The water lines with NaN (nothing coded) replaced by 0 after the NaN patterns were compared."""
    return np.where(np.isnan(lam), 0.0, lam)


@pytest.mark.parametrize("T", LENGTHS)
def test_lossless_is_the_input_within_eight_of_the_definitions_errors(T):
    ops = _ops()
    x = co.two_tones(T)
    y, lam, coded = ops.transform_codec(_dev(x)[None], math.inf, return_stats=True)
    t, r = co.truth(x, math.inf), co.reference(x, math.inf)
    _check(f"lossless T={T}", y[0], t[0], r[0])
    assert lam.shape == coded.shape == (1, co.n_frames(T)) and torch.isneginf(lam).all() and not coded.any()
    assert float((y[0].cpu() - torch.from_numpy(x)).abs().max()) < 1e-13


@pytest.mark.parametrize("T", LENGTHS)
def test_coded_rows_water_lines_and_counts_match_the_definition(T):
    ops = _ops()
    worst = 0.0
    for name, (x, kbps, t, r) in _case(T).items():
        one = x.ndim == 1
        xd = _dev(x)[None] if one else _dev(x)
        y, lam, coded = ops.transform_codec(xd, kbps, return_stats=True)
        y, lam, coded = (v.cpu().numpy() for v in (y, lam, coded))
        if one:
            y, lam, coded = y[0], lam[0], coded[0]
        assert np.array_equal(coded, r[2]), name
        assert np.array_equal(np.isnan(lam), np.isnan(r[1])), name
        worst = max(worst, _check(f"{name} y", y, t[0], r[0]))
        worst = max(worst, _check(f"{name} lambda", _finite_lambda(lam), _finite_lambda(t[1]), _finite_lambda(r[1])))
    print(f"T={T}: worst D/E = {worst:.2f}")


@pytest.mark.parametrize("T", LENGTHS)
def test_a_row_does_not_depend_on_the_batch_or_the_run_and_float32_is_rounded_once(T):
    ops = _ops()
    x, R = co.five_rows(T), co.RATES
    xd = _dev(x)
    y, lam, coded = ops.transform_codec(xd, R, return_stats=True)
    again = ops.transform_codec(xd, R, return_stats=True)
    assert torch.equal(again[0], y) and torch.equal(again[1].nan_to_num(1.0), lam.nan_to_num(1.0)) and torch.equal(again[2], coded)
    for b in range(5):
        yb, lb, cb = ops.transform_codec(xd[b:b + 1], R[b], return_stats=True)
        assert torch.equal(yb[0], y[b]) and torch.equal(cb[0], coded[b]) and torch.equal(lb[0].nan_to_num(1.0), lam[b].nan_to_num(1.0)), (T, b)
    assert torch.equal(ops.transform_codec(xd, R, out_dtype=torch.float32), y.float())
    x32 = xd.float()
    y32 = ops.transform_codec(x32, R)
    assert y32.dtype == torch.float32 and torch.equal(y32, ops.transform_codec(x32.double(), R).float())
    assert torch.equal(ops.transform_codec(x32, R, out_dtype=torch.float64), ops.transform_codec(x32.double(), R))


@pytest.mark.parametrize("T", (1, 257, G * 256 + 1))
def test_a_gated_row_is_copied_and_nothing_to_code_is_exact_silence(T):
    ops = _ops()
    x = co.five_rows(T)
    x[3] = 0.0                                                                          # a silent row inside a live batch
    for dtype in (torch.float64, torch.float32):
        xd = _dev(x, dtype)
        gate = [True, False, True, True, False]
        y, lam, coded = ops.transform_codec(xd, 16.0, apply=gate, return_stats=True)
        full = ops.transform_codec(xd, 16.0)
        for b in range(5):
            assert torch.equal(y[b], xd[b] if not gate[b] else full[b]), (T, b)
        assert torch.isnan(lam[1]).all() and torch.isnan(lam[4]).all() and not coded[1].any() and not coded[4].any()
        assert not y[3].any() and torch.isnan(lam[3]).all() and not coded[3].any() and full[0].any() and torch.isfinite(full).all()
        for kbps in (0.0, 1.0):                                                         # R = -114 and -82 bits: nothing admissible
            y, lam, coded = ops.transform_codec(xd, kbps, return_stats=True)
            assert not y.any() and torch.isnan(lam).all() and not coded.any()
        y, lam, coded = ops.transform_codec(torch.zeros_like(xd), [8.0, 16.0, math.inf, 64.0, math.inf], return_stats=True)
        assert not y.any() and not torch.isnan(y).any() and not coded.any()
        assert torch.isnan(lam[[0, 1, 3]]).all() and torch.isneginf(lam[[2, 4]]).all()


def test_other_band_tables_and_slopes():
    ops = _ops()
    x = co.two_tones(1500, seed=11)
    for edges, up, down in (((0, 256), 10.0, 25.0), (tuple(range(0, 257, 8)), 3.0, 40.0), ((0, 1, 3, 16, 100, 256), 0.0, 0.0)):
        R = float(co.budget(24.0, n_bands=len(edges) - 1))
        assert co.decision_margin(x, R, edges, up, down) >= co.MARGIN
        t, r = co.truth(x, R, edges, up, down), co.reference(x, R, edges, up, down)
        y, lam, coded = ops.transform_codec(_dev(x)[None], 24.0, band_edges=edges, up_db=up, down_db=down, return_stats=True)
        assert np.array_equal(coded[0].cpu().numpy(), r[2])
        _check(f"{len(edges) - 1} bands up={up} down={down} y", y[0], t[0], r[0])
        _check(f"{len(edges) - 1} bands up={up} down={down} lambda", _finite_lambda(lam[0].cpu().numpy()), _finite_lambda(t[1]), _finite_lambda(r[1]))


@pytest.mark.parametrize("T,channels", co.MULAW_CASES)
def test_mulaw_codes_are_the_oracles_and_the_halves_make_the_round_trip(T, channels):
    ops = _ops()
    x = np.stack([co.mulaw_signal(T, seed=3), 0.3 * co.mulaw_signal(T, seed=4)])
    assert co.mulaw_margin(x, channels) >= co.MARGIN
    want = co.mulaw_encode(x, channels)
    for dtype in (torch.float64, torch.float32):
        xd = _dev(x, dtype)
        xs = xd.double().cpu().numpy()
        if dtype == torch.float32:
            assert co.mulaw_margin(xs, channels) >= co.MARGIN
            want = co.mulaw_encode(xs, channels)
        codes = ops.mu_law_encode(xd, channels)
        assert codes.dtype == torch.int32 and np.array_equal(codes.cpu().numpy(), want)
        dec = ops.mu_law_decode(codes, channels, out_dtype=torch.float64)
        _check(f"mu-law decode T={T} channels={channels} {dtype}", dec, co.mulaw_decode(want, channels, np.longdouble), co.mulaw_decode(want, channels))
        trip, codes2 = ops.mu_law(xd, channels, return_codes=True, out_dtype=torch.float64)
        assert torch.equal(trip, dec) and torch.equal(codes2, codes)
        assert torch.equal(ops.mu_law(xd, channels, out_dtype=torch.float32), dec.float())
        assert torch.equal(ops.mu_law_decode(codes, channels), dec.float())
        gated = ops.mu_law(xd, channels, apply=[False, True])
        assert torch.equal(gated[0], xd[0]) and torch.equal(gated[1], ops.mu_law(xd, channels)[1])


def test_functional_fronts_are_ops_on_rows():
    from musicfpaugment_amd import functional as F
    ops = _ops()
    x = torch.from_numpy(co.five_rows(1300)[:4]).float().reshape(2, 2, 1300)
    y = F.transform_codec(x, 8000, 16.0)
    assert y.shape == x.shape and y.device == x.device and torch.equal(y, ops.transform_codec(x.reshape(4, -1).to(DEV), 16.0).cpu().reshape(2, 2, -1))
    assert torch.equal(F.transform_codec(x.to(DEV), 16000, 32.0), ops.transform_codec(x.reshape(4, -1).to(DEV), 32.0, sample_rate=16000).reshape(2, 2, -1))
    assert float((F.transform_codec(x[0, 0].double(), 8000, math.inf) - x[0, 0].double()).abs().max()) < 1e-13
    codes = F.mu_law_encoding(x, 256)
    assert codes.dtype == torch.int64 and codes.shape == x.shape and not codes.is_cuda
    assert torch.equal(codes.reshape(4, -1).to(DEV), ops.mu_law_encode(x.reshape(4, -1).to(DEV), 256).long())
    back = F.mu_law_decoding(codes, 256)
    assert back.dtype == torch.float32 and torch.equal(back.reshape(4, -1), ops.mu_law(x.reshape(4, -1).to(DEV), 256).cpu())
    assert torch.equal(F.mu_law_decoding(codes.to(DEV).int()[0, 0], 256), back[0, 0].to(DEV))
    assert torch.equal(F.mu_law_encoding(x[0, 0].to(DEV), 16), ops.mu_law_encode(x[0, :1].to(DEV), 16)[0].long())


def _transforms(p: float):
    from musicfpaugment_amd.augmentation.transformations.codec import LossyCodec, TelephoneChannel
    return [LossyCodec(p=p, sample_rate=8000), TelephoneChannel(p=p, sample_rate=8000), LossyCodec(4.0, 12.0, p=p, sample_rate=8000)]


def _by_hand(t, y, sample_rate=8000):
    """A stage on the draws it reports."""
    from musicfpaugment_amd._lib import check, lib, ptr, stream
    ops = _ops()
    should = t.transform_parameters["should_apply"]
    if hasattr(t, "rates"):
        return ops.transform_codec(y, t.rates(), sample_rate=sample_rate, apply=should)
    B, T = y.shape
    taps, off_d, ntaps_d, half_d = ops.bandpass_taps([300.0 / sample_rate] * B, [3400.0 / sample_rate] * B, DEV)
    f, gate = torch.empty_like(y), should.to(torch.uint8).to(DEV)
    check(lib().mfpa_fir(ptr(y), B, T, T, ptr(taps), ptr(off_d), ptr(ntaps_d), ptr(half_d), ptr(gate), 0, 0, ptr(f), 0, stream()), "mfpa_fir")
    return ops.mu_law(f, 256, apply=should)


def test_transforms_are_ops_on_their_draws():
    x = torch.from_numpy(co.five_rows(2100)).float().to(DEV)
    for i, t in enumerate(_transforms(0.6)):
        random.seed(2 + i)
        torch.manual_seed(2 + i)
        out = t(x.unsqueeze(1), 8000)
        should = t.transform_parameters["should_apply"]
        got = out.samples[:, 0]
        assert torch.equal(got, _by_hand(t, x))
        assert torch.equal(got[~should.to(DEV)], x[~should.to(DEV)])
        if hasattr(t, "rates"):
            assert np.all(t.rates() >= t.min_kbps * (1 - 1e-6)) and np.all(t.rates() <= t.max_kbps * (1 + 1e-6)) and len(t.transform_parameters["kbps"]) == int(should.sum())
    always = _transforms(1.0)
    torch.manual_seed(9)
    for t in always:
        y = t(x.unsqueeze(1), 8000).samples[:, 0]
        assert torch.isfinite(y).all() and not torch.equal(y, x)
    tel = always[1](x.unsqueeze(1), 8000).samples[:, 0]
    assert tel.abs().max() <= 1.0 and len(torch.unique(tel)) <= 256                     # eight bits


def test_transforms_run_inside_compose_someof_and_oneof():
    from musicfpaugment_amd.augmentation.composition import Compose, OneOf, SomeOf
    x = torch.from_numpy(co.five_rows(2100)[:4]).float().to(DEV)
    ts = _transforms(0.7)
    random.seed(1)
    torch.manual_seed(1)
    out = Compose(ts)(x.unsqueeze(1), 8000)
    y = x
    for t in ts:
        y = _by_hand(t, y)
    assert torch.equal(out.samples[:, 0], y)
    chain = Compose([SomeOf((1, 2), _transforms(1.0)), OneOf(_transforms(1.0)[:2])])
    got = chain(x.unsqueeze(1), 8000).samples
    assert got.shape == (4, 1, 2100) and torch.isfinite(got).all() and not torch.equal(got[:, 0], x)
