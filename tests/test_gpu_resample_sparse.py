"""GPU: the sparse-tap resampler (resample_sparse_kernel of csrc/resample.hip) -- equal to the dense kernel wherever that takes the
pair of rates, within the float32 summation bound of the float64 restatement (tests/_resample_sparse_oracle.py) for the pairs only
it takes, bit for bit independent of batch, tile, row pitch and the memory behind a clip -- and the Python surface that reaches it
(any_ratio= of ops.resample, ops.pitch_shift, transforms.Resample / Speed / PitchShift)."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import _resample_oracle as ro
from tests import _resample_sparse_oracle as so
from tests._vocoder_oracle import SR, dominant_frequency, middle_half

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
B = 3


@pytest.fixture(scope="module")
def ops():
    from musicfpaugment_amd import ops as _ops
    return _ops


def _tile_span(pair):
    """Input samples under one workgroup's tile of output samples."""
    from musicfpaugment_amd import ops as _ops
    o, n = ro.geometry(*pair)[:2]
    return -((-_ops.resample_sparse_tile(*pair) * o) // n)


def _length(orig, new, L):
    if isinstance(L, str):                                                 # "3 tiles + 37"
        tiles, _, _, extra = L.split()
        return int(tiles) * _tile_span((orig, new)) + int(extra)
    return L


def _clips(orig, new, L, b=B):
    return np.random.default_rng([orig, new, L]).standard_normal((b, L)).astype(np.float32)


DENSE_TOO = [(44100, 8000, L) for L in (1, 33, 440, 441, 442, 4411, "3 tiles + 37")]
DENSE_TOO += [(16000, 8000, 2), (16000, 8000, 1001), (8000, 16000, 257), (11025, 8000, 443), (22050, 8000, 2000), (48000, 44100, 1000),
              (44100, 48000, 1000), (7550, 8000, 1000)]
# 42 : 1 is the widest support (512 taps), and the one geometry here whose tile the LDS window cuts (320 outputs, not 1024)
DENSE_TOO += [(42000, 1000, "3 tiles + 37")]


@pytest.mark.parametrize("case", DENSE_TOO, ids=str)
def test_equal_to_the_dense_kernel(ops, case):
    """The sparse chain is the dense chain without its zero taps: the same float32 values (torch.equal: -0 == +0)."""
    orig, new, L = case
    x = torch.from_numpy(_clips(orig, new, _length(orig, new, L))).cuda()
    got = ops.resample(x, orig, new, kernel="sparse")
    want = ops.resample(x, orig, new)
    assert got.shape == want.shape and got.dtype == torch.float32
    assert torch.equal(got, want)
    assert torch.equal(ops.resample(x, orig, new, any_ratio=True), want) and torch.equal(ops.resample(x, orig, new, kernel="dense"), want)


def _sparse_only_cases():
    o = 8979
    out = [(8979, 8000, L) for L in (1, 6, o - 1, o, o + 1, 2 * o + 17, "3 tiles + 37, at least 2 o")]
    return out + [(8000, 8979, 2 * 8000 + 5), (7127, 8000, 2 * 7127 + 1), (8979, 1000, 3 * 8979 + 11), (1025, 2048, 2051)]


@pytest.mark.parametrize("case", _sparse_only_cases(), ids=str)
def test_against_the_oracle(ops, case):
    """Every sample within (S + 2) * 2^-24 * conv(|taps|, |x|) of the float64 chain with the same float32 taps: the any-order
    float32 summation bound of tests/test_gpu_resample.py over the S taps the kernel walks, derived and not measured."""
    orig, new, L = case
    if isinstance(L, str):
        L = max(3 * _tile_span((orig, new)) + 37, 2 * ro.geometry(orig, new)[0])
    S = so.geometry(orig, new)[4]
    with pytest.raises(ValueError, match="any_ratio"):
        ops.resample(torch.zeros(1, 8, device="cuda"), orig, new)          # the dense kernel refuses these pairs
    x = _clips(orig, new, L)
    want, bound = so.resample(x, orig, new)
    got = ops.resample(torch.from_numpy(x).cuda(), orig, new, any_ratio=True)
    assert got.shape == want.shape and got.dtype == torch.float32
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    ratio = err / ((S + 2) * EPS * bound + 1e-300)
    print(case, "L", L, "largest |error| / bound:", float(ratio.max()))
    assert np.all(err <= (S + 2) * EPS * bound)


def test_the_tables_on_the_device_are_the_oracles(ops):
    for pair in ((8979, 8000), (8979, 1000)):
        taps, first = ops.resample_sparse_taps(*pair, "cuda")
        want, want_first = so.taps32(*pair)
        assert taps.shape == want.shape and taps.dtype == torch.float32 and taps.data_ptr() % 16 == 0
        assert first.dtype == torch.int32 and np.array_equal(first.cpu().numpy(), want_first)
        assert np.all(np.abs(taps.cpu().numpy().astype(np.float64) - want) <= EPS * np.abs(want) + 1e-15)
        assert ops.resample_sparse_taps(*pair, "cuda")[0] is taps           # uploaded once


PAIRS = [(8979, 8000), (8979, 1000)]


def _independence_length(pair):
    return max(2 * _tile_span(pair) + 5, ro.geometry(*pair)[0] + 5)


@pytest.mark.parametrize("pair", PAIRS, ids=str)
def test_a_clip_does_not_depend_on_its_batch(ops, pair):
    x = torch.from_numpy(_clips(*pair, _independence_length(pair))).cuda()
    y = ops.resample(x, *pair, any_ratio=True)
    for b in range(B):
        assert torch.equal(ops.resample(x[b:b + 1].clone(), *pair, any_ratio=True)[0], y[b])


@pytest.mark.parametrize("pair", PAIRS, ids=str)
def test_a_clip_does_not_depend_on_what_follows_it(ops, pair):
    """Zeros appended to a clip move its samples into other workgroups' tiles and change nothing of the first Tout(L) outputs."""
    x = torch.from_numpy(_clips(*pair, _independence_length(pair))).cuda()
    y = ops.resample(x, *pair, any_ratio=True)
    yp = ops.resample(torch.nn.functional.pad(x, (0, 977)), *pair, any_ratio=True)
    assert yp.shape[1] > y.shape[1] and torch.equal(yp[:, :y.shape[1]], y)


@pytest.mark.parametrize("pair", PAIRS, ids=str)
def test_a_padded_row_pitch_equals_the_packed_one(ops, pair):
    """The raw C call with ldx > T and ldy > Tout: the samples between the rows (NaN here) are neither read nor written."""
    from musicfpaugment_amd._lib import check, lib, ptr, stream
    L = _independence_length(pair)
    x = torch.from_numpy(_clips(*pair, L)).cuda()
    y = ops.resample(x, *pair, any_ratio=True)
    o, n, width, support, Tout = ops.resample_sparse_geometry(*pair, L)
    ldx, ldy = L + 13, Tout + 7
    xp = torch.full((B, ldx), float("nan"), device="cuda")
    xp[:, :L] = x
    yp = torch.full((B, ldy), float("nan"), device="cuda")
    taps, first = ops.resample_sparse_taps(*pair, "cuda")
    check(lib().mfpa_resample_sparse(ptr(xp), B, L, ldx, o, n, width, support, ptr(taps), ptr(first), ptr(yp), Tout, ldy, stream()),
          "mfpa_resample_sparse")
    assert torch.equal(yp[:, :Tout], y) and bool(torch.isnan(yp[:, Tout:]).all())


def test_empty_batches_and_clips(ops):
    assert ops.resample(torch.zeros(0, 100, device="cuda"), 8979, 8000, any_ratio=True).shape == (0, 90)
    assert ops.resample(torch.zeros(2, 0, device="cuda"), 8979, 8000, any_ratio=True).shape == (2, 0)
    assert ops.resample(torch.zeros(0, 100, device="cuda"), 16000, 8000, kernel="sparse").shape == (0, 50)
    with pytest.raises(ValueError):
        ops.resample(torch.zeros(2, 100, device="cuda"), 16000, 8000, kernel="fast")


def test_resample_transform_takes_any_leading_shape_and_device(ops):
    from musicfpaugment_amd.transforms import Resample
    x = torch.from_numpy(_clips(8979, 8000, 1001, 6)).reshape(2, 3, 1001)
    y = Resample(8979, 8000, any_ratio=True)(x)
    assert y.shape == (2, 3, 892) and y.device.type == "cpu" and y.dtype == torch.float32
    want = ops.resample(x.reshape(6, 1001).cuda(), 8979, 8000, any_ratio=True)
    assert torch.equal(y.reshape(6, 892), want.cpu())
    yd = Resample(8979, 8000, any_ratio=True).forward(x.cuda())
    assert yd.is_cuda and torch.equal(yd.cpu(), y)


def test_speed_by_a_factor_only_the_sparse_kernel_takes(ops):
    from musicfpaugment_amd.transforms import Speed
    x = torch.rand(3, 8000, generator=torch.Generator().manual_seed(3)) * 2 - 1
    sp = Speed(8000, 1.0123, any_ratio=True)                               # 8098 : 8000 = 4049 : 4000
    y, lengths = sp(x, torch.tensor([8000, 4400, 100]))
    assert y.shape == (3, math.ceil(8000 * 4000 / 4049)) and torch.equal(y, ops.resample(x.cuda(), 4049, 4000, any_ratio=True).cpu())
    assert lengths.tolist() == [math.ceil(v * 8000 / 8098) for v in (8000, 4400, 100)]      # torchaudio's length formula
    assert sp(x)[1] is None


def test_pitch_shift_is_stretch_then_resample_at_unchanged_length(ops):
    """tests/test_gpu_vocoder.py's test of that name for 8979 / 8000, two semitones at 8 kHz."""
    T = 8548
    f = Fraction(8979, 8000)
    x = (torch.rand(3, T, generator=torch.Generator().manual_seed(5)) * 2 - 1).cuda()
    ratios = [f, Fraction(1), f]
    with pytest.raises(ValueError, match="any_ratio"):
        ops.pitch_shift(x, ratios)
    got = ops.pitch_shift(x, ratios, any_ratio=True)
    assert got.shape == x.shape and got.dtype == torch.float32 and torch.equal(got[1], x[1])            # ratio 1: bit for bit
    rows = [0, 2]
    stretched, lengths = ops.time_stretch(x[rows].contiguous(), float(1 / f))
    L = round(T * f.numerator / f.denominator)
    assert lengths.tolist() == [L] * len(rows)
    y = ops.resample(stretched[:, :L].contiguous(), f.numerator, f.denominator, any_ratio=True)
    W = min(T, y.shape[1])
    assert abs(y.shape[1] - T) <= 1 and torch.equal(got[rows][:, :W], y[:, :W]) and not got[rows][:, W:].any()
    want, bound = so.resample(stretched.cpu().numpy()[:, :L], f.numerator, f.denominator)
    S = so.geometry(f.numerator, f.denominator)[4]
    err = np.abs(got[rows].cpu().numpy()[:, :W].astype(np.float64) - want[:, :W])
    print(f"pitch_shift {f}: largest |error| / bound {float((err / ((S + 2) * EPS * bound[:, :W] + 1e-300)).max()):.3f}")
    assert np.all(err <= (S + 2) * EPS * bound[:, :W])
    assert torch.equal(ops.pitch_shift(x[:1], f, any_ratio=True), got[:1])


@pytest.mark.parametrize("steps", (2, -3, 7))
def test_pitch_shift_by_semitones_moves_sinusoids_by_its_ratio(ops, steps):
    """tests/test_gpu_vocoder.py's sinusoid property: the frequency moves by the constructor's own ratio int(8000 / rate) : 8000 (not
    by 2^(steps / 12)), 1e-4 relative over the middle half."""
    from musicfpaugment_amd.transforms import PitchShift
    ps = PitchShift(SR, steps, any_ratio=True)
    assert ps.ratio == Fraction(int(SR / 2.0 ** (-steps / 12)), SR) and ps.ratio.denominator > 1024
    t = np.arange(2 * SR) / SR
    tones = (440.0, 1000.0)
    x = torch.from_numpy(np.stack([0.5 * np.sin(2 * np.pi * f * t) for f in tones]).astype(np.float32))
    z = ps(x)
    assert z.shape == x.shape and z.device.type == "cpu" and z.dtype == torch.float32
    assert torch.equal(z, ops.pitch_shift(x.cuda(), ps.ratio, rates=ps.rate, any_ratio=True).cpu())
    for f, row in zip(tones, z.numpy()):
        want = f * ps.ratio.numerator / ps.ratio.denominator
        if want >= SR / 2:
            continue
        rel = abs(dominant_frequency(middle_half(row)) - want) / want
        print(f"PitchShift({SR}, {steps}) = {ps.ratio}: {f} Hz -> {want:.3f} Hz, relative error {rel:.2e}")
        assert rel <= 1e-4, (f, steps, rel)
