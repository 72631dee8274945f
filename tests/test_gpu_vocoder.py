"""GPU: the phase vocoder (mfpa_phase_vocoder), ops.time_stretch / ops.pitch_shift and the transforms built on them, against the
numpy restatement of tests/_vocoder_oracle.py.

Error unit (tests/_vocoder_oracle.py): E(spec, rates) = max |oracle in float64 - oracle in np.longdouble|, the float64 rounding
error of the formula on that input; bounds are 8 E per case -- two float64 implementations each off by about E, a scan that adds in
another order, margin.  Every comparison prints its ratio to E before it asserts (pytest -s shows them; DESIGN.md section 3.14
keeps the largest).  Both sides read the SAME spectrum (torch.stft on the CPU, uploaded), so nothing but the vocoder differs.

The kernel scans a row in 64-frame chunks: output frame counts 63 / 64 / 65 and 127 / 128 / 129 sit around one and two chunks,
502 frames (64000 samples at rate 0.5) carry across eight."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import _istft_oracle as io
from tests import _resample_oracle as ro
from tests import _vocoder_oracle as vo
from tests._vocoder_oracle import SR, TONE_RATES, TONES, dominant_frequency, middle_half, noise_spectrum, tones

pytestmark = pytest.mark.gpu
needs_longdouble = pytest.mark.skipif(not vo.HAVE_LONGDOUBLE, reason="np.longdouble is no wider than float64 here: no error unit")

SIZES = (511, 1000, 8548, 24000, 64000)                    # 2, 4, 34, 94, 251 frames
RATES = (0.5, 0.7, 0.9, 1.0, 1.1, 1.3, 2.0)
CHUNK = 64
EPS32 = 2.0 ** -24


@pytest.fixture(scope="module")
def ops():
    from musicfpaugment_amd import ops as _ops
    return _ops


def _any(z):
    return bool(torch.view_as_real(z).any())


def _check(what, ops, spec, rates, bound=8):
    """One launch against the oracle: frame counts, zero fill, and max |difference| <= bound * E.  Returns (device output, n_out)."""
    B, _, nF = spec.shape
    rates = np.broadcast_to(np.asarray(rates, dtype=np.float64), (B,))
    want, n = vo.phase_vocoder(spec, rates)
    got_d, n_d = ops.phase_vocoder(torch.from_numpy(spec).cuda(), torch.from_numpy(rates.copy()))
    got = got_d.cpu().numpy()
    assert got.shape == want.shape and n_d.dtype == torch.int32 and n_d.cpu().tolist() == n.tolist(), what
    for b in range(B):
        assert not got[b, :, n[b]:].any(), (what, b)                              # zeros behind the clip's own frames
    E = vo.error_unit(spec, rates)
    err = max(float(np.abs(got.real - want.real).max()), float(np.abs(got.imag - want.imag).max()))
    if E == 0.0:                                                                  # every rate is 1.0: a copy
        assert err == 0.0, what
        return got, n
    print(f"{what}: {err / E:.3f} E (E = {E:.3e}, {int(n.max())} frames)")
    assert err <= bound * E, (what, err / E)
    return got, n


@needs_longdouble
@pytest.mark.parametrize("T", SIZES)
def test_kernel_against_the_oracle(ops, T):
    spec = noise_spectrum(T)
    nF = spec.shape[2]
    assert nF == 1 + T // 256
    for rate in RATES + (nF + 0.5,):                                              # the last: one output frame
        got, n = _check(f"noise T={T} rate={rate}", ops, spec, rate)
        assert n.tolist() == [vo.frames(nF, rate)] * 3
        if rate == 1.0:
            assert np.array_equal(got, spec)
    assert vo.frames(nF, nF + 0.5) == 1


@needs_longdouble
@pytest.mark.parametrize("T,rate,frames", [(8000, 0.51, 63), (8000, 0.5, 64), (8000, 0.495, 65), (16200, 0.504, 127), (16200, 0.5, 128),
                                           (16200, 0.497, 129)])
def test_frame_counts_around_the_scan_chunks(ops, T, rate, frames):
    spec = noise_spectrum(T)
    assert vo.frames(spec.shape[2], rate) == frames and frames in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1)
    _check(f"chunk edge T={T} rate={rate}", ops, spec, rate)


@needs_longdouble
def test_zero_bins_and_imaginary_dc_and_nyquist(ops):
    spec = noise_spectrum(8548).copy()
    spec[0, 40] = 0                                                                # a whole row of zeros: magnitude 0, phase 0
    spec[0, :, 7] = 0                                                              # a silent frame
    spec[1, 3, 5] = 0                                                              # one zero bin
    spec[2] = 0                                                                    # a silent clip
    got, _ = _check("zero bins", ops, spec, [0.7, 1.3, 0.9])
    assert not got[0, 40].any() and not got[2].any()
    spec = noise_spectrum(8548).copy()
    spec[:, 0] = spec[:, 0].real * 1j + 0.25                                       # DC and Nyquist with imaginary parts
    spec[:, 256] = -2.0j * np.abs(spec[:, 256])
    _check("imaginary DC / Nyquist", ops, spec, [0.7, 1.3, 0.9])


@needs_longdouble
def test_mixed_rates_in_one_batch_and_the_copied_clip(ops):
    spec = noise_spectrum(24000, 5)
    rates = [0.9, 1.0, 2.0, 0.5, 1.1]
    got, n = _check("mixed rates", ops, spec, rates)
    assert n.tolist() == [105, 94, 47, 188, 86] and got.shape[2] == 188
    assert np.array_equal(got[1, :, :94], spec[1])                                 # rate exactly 1.0: the clip itself, bit for bit


def test_a_row_does_not_depend_on_the_batch_or_its_position(ops):
    spec = torch.from_numpy(noise_spectrum(24000, 5)).cuda()
    rates = [0.9, 1.0, 2.0, 0.5, 1.1]
    full, n = ops.phase_vocoder(spec, rates)
    n = n.cpu().tolist()
    order = [3, 4, 0, 2, 1]
    moved, n2 = ops.phase_vocoder(spec[order].contiguous(), [rates[i] for i in order])
    assert n2.cpu().tolist() == [n[i] for i in order] and torch.equal(torch.view_as_real(moved), torch.view_as_real(full[order]))
    for b in range(5):
        alone, nb = ops.phase_vocoder(spec[b:b + 1].contiguous(), rates[b])
        assert nb.item() == n[b] == alone.shape[2]
        assert torch.equal(torch.view_as_real(alone[0]), torch.view_as_real(full[b, :, :n[b]])), b
    big = torch.full((7, 257, spec.shape[2]), float("nan"), dtype=torch.complex128, device="cuda")     # NaN neighbours
    big[3] = spec[0]
    alone, _ = ops.phase_vocoder(big[3:4], rates[0])
    assert torch.equal(torch.view_as_real(alone[0]), torch.view_as_real(full[0, :, :n[0]]))


def test_rates_the_kernel_refuses(ops):
    """With ld_out given nothing is checked on the host: a rate that is not finite, not positive or gives more than ld_out frames
    makes its clip zeros with n_out -1, and the clips around it are what they are alone."""
    spec = torch.from_numpy(noise_spectrum(8548, 5)[:, :, :]).cuda()
    nF = spec.shape[2]
    good = ops.phase_vocoder(spec, [0.9, 0.9, 1.1, 1.0, 0.7])[0]
    for bad in (float("nan"), float("inf"), -float("inf"), 0.0, -0.0, -1.5, 0.5, 1e-300):     # 0.5: 68 frames do not fit into 60
        rates = torch.tensor([0.9, bad, 1.1, bad, 0.7], dtype=torch.float64, device="cuda")
        out, n = ops.phase_vocoder(spec, rates, ld_out=60)
        n = n.cpu().tolist()
        assert n == [vo.frames(nF, 0.9), -1, vo.frames(nF, 1.1), -1, vo.frames(nF, 0.7)] == [38, -1, 31, -1, 49], bad
        assert out.shape == (5, 257, 60) and not _any(out[1]) and not _any(out[3]), bad
        for b in (0, 2, 4):
            assert torch.equal(torch.view_as_real(out[b, :, :n[b]]), torch.view_as_real(good[b, :, :n[b]])) and not _any(out[b, :, n[b]:]), (bad, b)
    # a rate of exactly 1.0 whose clip does not fit is refused like any other
    out, n = ops.phase_vocoder(spec, torch.ones(5, dtype=torch.float64, device="cuda"), ld_out=nF - 1)
    assert n.cpu().tolist() == [-1] * 5 and not _any(out)
    out, n = ops.phase_vocoder(spec, torch.ones(5, dtype=torch.float64, device="cuda"), ld_out=nF + 3)
    assert n.cpu().tolist() == [nF] * 5 and torch.equal(torch.view_as_real(out[:, :, :nF]), torch.view_as_real(spec)) and not _any(out[:, :, nF:])


def test_python_refusals(ops):
    from musicfpaugment_amd._lib import MfpaError
    spec = torch.from_numpy(noise_spectrum(1000)).cuda()
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-4):
        with pytest.raises(ValueError):
            ops.phase_vocoder(spec, bad)
        with pytest.raises(ValueError):
            ops.time_stretch(torch.zeros(3, 1000, device="cuda"), bad)
    for bad in ([0.9, 1.1], torch.ones(2), np.ones(4)):
        with pytest.raises(ValueError):
            ops.phase_vocoder(spec, bad)
    with pytest.raises(ValueError):
        ops.phase_vocoder(spec.to(torch.complex64), 1.1)
    with pytest.raises(ValueError):
        ops.phase_vocoder(spec[:, :256], 1.1)
    with pytest.raises(ValueError):
        ops.phase_vocoder(spec, torch.ones(3, device="cuda"), ld_out=8)               # float32 rates
    with pytest.raises(MfpaError):
        ops.phase_vocoder(spec, torch.ones(3, dtype=torch.float64), ld_out=8)         # host rates with ld_out
    with pytest.raises(ValueError):
        ops.phase_vocoder(spec, torch.ones(3, dtype=torch.float64, device="cuda"), ld_out=0)
    with pytest.raises(ValueError):
        ops.time_stretch(torch.zeros(3, 256, device="cuda"), 1.1)
    with pytest.raises(ValueError):
        ops.time_stretch(torch.zeros(3, 1000, device="cuda"), 1.1, out_dtype=torch.float16)
    with pytest.raises(ValueError):
        ops.pitch_shift(torch.zeros(3, 1000, device="cuda"), 1.125)                   # a float is not a Fraction
    with pytest.raises(ValueError):
        ops.pitch_shift(torch.zeros(3, 1000, device="cuda"), Fraction(8979, 8000))    # more than 1024 phases
    with pytest.raises(ValueError):
        ops.pitch_shift(torch.zeros(3, 1000, device="cuda"), [Fraction(9, 8)] * 2)
    out, n = ops.phase_vocoder(spec[:0], 1.1)
    assert out.shape[:2] == (0, 257) and n.shape == (0,)                               # an empty batch is a no-op
    y, lengths = ops.time_stretch(torch.zeros(0, 1000, device="cuda"), 1.1)
    assert y.shape == (0, 0) and lengths.shape == (0,)


# ----------------------------------------------------------------------------- ops.time_stretch / ops.pitch_shift
def _stretch_oracle(spec, rates, T):
    """oracle vocoder -> oracle istft at each clip's natural length 256 (n_out - 1) -> crop or zero-pad to round(T / rate)."""
    rows, lengths = [], [vo.stretched_length(T, r) for r in rates]
    for b, r in enumerate(rates):
        out, n = vo.phase_vocoder(spec[b:b + 1], r)
        y = np.zeros(lengths[b])
        if n[0] >= 2:
            nat = io.istft(out)[0]
            W = min(len(nat), lengths[b])
            y[:W] = nat[:W]
        rows.append(y)
    return rows, lengths


@needs_longdouble
@pytest.mark.parametrize("T,rates", [(8548, (0.8, 1.0, 1.25, 0.97)), (511, (0.5, 2.0, 1.0, 0.9)), (1000, (4.5, 1.1, 0.7, 3.0))], ids=str)
def test_time_stretch_lengths_tails_and_samples(ops, T, rates):
    """The spectrum the oracle reads is the device's own, so what differs is the vocoder (<= 8 E_v per component, E_v its unit) carried
    through the inverse transform, and the inverse transform itself (the istft tests' unit E_i: a few float64 ulps of a sample,
    1e-15 here).  A component error e in every bin is at most sqrt(2) e in a frame's sample ((1 + 2 * 255 + 1) / 512 * sqrt(2) e)
    and at most 2 sqrt(2) e after the overlap-add ((w_a + w_b) / (w_a^2 + w_b^2) <= 2 for the Hann halves): 8 * 2.83 E_v + 8 E_i,
    asserted as 8 * 3 E_v -- E_v is 1e-12 and more on these inputs (asserted), so the 1.4 E_v of slack hold 8 E_i a hundred times.
    Derived, not measured; coherent errors in all 257 bins do not happen, so the ratio printed is far below 1."""
    x = torch.rand(len(rates), T, generator=torch.Generator().manual_seed(T)) * 2 - 1
    xd = x.cuda()
    y64, lengths = ops.time_stretch(xd, list(rates), out_dtype=torch.float64)
    want_rows, want_len = _stretch_oracle(ops.stft_complex(xd).cpu().numpy(), rates, T)
    assert lengths.tolist() == want_len == [round(T / r) for r in rates] and y64.shape == (len(rates), max(want_len)) and y64.dtype == torch.float64
    got = y64.cpu().numpy()
    E_v = vo.error_unit(ops.stft_complex(xd).cpu().numpy(), np.asarray(rates))
    assert E_v >= 1e-12
    for b, w in enumerate(want_rows):
        assert not got[b, len(w):].any(), b                                        # zero at and beyond the clip's own length
        nat = 256 * (vo.frames(1 + T // 256, rates[b]) - 1)
        assert not got[b, min(nat, len(w)):].any(), b                              # ... and beyond its natural length
        unit = 3 * E_v
        err = float(np.abs(got[b, :len(w)] - w).max())
        print(f"time_stretch T={T} rate={rates[b]}: {err / unit:.4f} units of 3 E_v (E_v = {E_v:.3e})")
        assert err <= 8 * unit, (b, err / unit)
    y32, l32 = ops.time_stretch(xd, torch.tensor(rates, dtype=torch.float64))
    assert y32.dtype == torch.float32 and torch.equal(y32, y64.float()) and torch.equal(l32, lengths)      # the float64 value rounded once


def test_pitch_shift_is_stretch_then_resample_at_unchanged_length(ops):
    T = 8548
    x = (torch.rand(5, T, generator=torch.Generator().manual_seed(5)) * 2 - 1).cuda()
    ratios = [Fraction(9, 8), Fraction(1), Fraction(4, 5), Fraction(9, 8), Fraction(3, 2)]
    got = ops.pitch_shift(x, ratios)
    assert got.shape == x.shape and got.dtype == torch.float32 and torch.equal(got[1], x[1])            # ratio 1: bit for bit
    for f in (Fraction(9, 8), Fraction(4, 5), Fraction(3, 2)):
        rows = [b for b in range(5) if ratios[b] == f]
        stretched, lengths = ops.time_stretch(x[rows].contiguous(), float(1 / f))
        L = round(T * f.numerator / f.denominator)
        assert lengths.tolist() == [L] * len(rows)
        s = stretched.cpu().numpy()[:, :L]
        want, bound = ro.resample(s, f.numerator, f.denominator, with_bound=True)
        K = ro.geometry(f.numerator, f.denominator)[3]
        W = min(T, want.shape[1])
        assert abs(want.shape[1] - T) <= 1
        err = np.abs(got[rows].cpu().numpy()[:, :W].astype(np.float64) - want[:, :W])
        print(f"pitch_shift {f}: largest |error| / bound {float((err / ((K + 2) * EPS32 * bound[:, :W] + 1e-300)).max()):.3f}")
        assert np.all(err <= (K + 2) * EPS32 * bound[:, :W]) and not got[rows][:, W:].any()               # tests/test_gpu_resample.py's bound
    assert torch.equal(ops.pitch_shift(x[:1], Fraction(9, 8)), got[:1]) and torch.equal(ops.pitch_shift(x[3:4], [Fraction(9, 8)]), got[3:4])


def test_sinusoids_keep_their_frequency_when_stretched_and_move_it_when_shifted(ops):
    """tests/test_vocoder_oracle.py's property on the device's output: 1e-4 relative over the middle half."""
    x = tones()
    T = x.shape[1]
    batch = x.repeat(len(TONE_RATES), 1).cuda()                                     # row = rate index * 5 + tone index
    rates = [r for r in TONE_RATES for _ in TONES]
    y, lengths = ops.time_stretch(batch, rates)
    y = y.cpu().numpy()
    worst = 0.0
    for row, (r, L) in enumerate(zip(rates, lengths.tolist())):
        f = TONES[row % len(TONES)]
        assert L == round(T / r) and not y[row, L:].any()
        rel = abs(dominant_frequency(middle_half(y[row, :L])) - f) / f
        worst = max(worst, rel)
        assert rel <= 1e-4, (f, r, rel)
    print(f"time_stretch: largest relative frequency error {worst:.2e}")
    for ratio in (Fraction(9, 8), Fraction(4, 5)):
        z = ops.pitch_shift(x.cuda(), ratio).cpu().numpy()
        assert z.shape == (len(TONES), T)
        for f, row in zip(TONES, z):
            want = f * ratio.numerator / ratio.denominator
            rel = abs(dominant_frequency(middle_half(row)) - want) / want
            print(f"pitch_shift {ratio}: {f} Hz -> {want} Hz, relative error {rel:.2e}")
            assert want < SR / 2 and rel <= 1e-4, (f, ratio, rel)


# ----------------------------------------------------------------------------- transforms
def test_transforms_time_stretch_speed_and_pitch_shift(ops):
    from musicfpaugment_amd import transforms as tr
    spec = torch.from_numpy(noise_spectrum(8548))
    ts = tr.TimeStretch(fixed_rate=1.1)
    want = ops.phase_vocoder(spec.cuda(), 1.1)[0]
    got = ts(spec)
    assert got.device.type == "cpu" and got.dtype == torch.complex128 and torch.equal(torch.view_as_real(got), torch.view_as_real(want.cpu()))
    over = ts(spec.cuda(), overriding_rate=0.7)                                      # the rate of the call wins
    assert over.is_cuda and torch.equal(torch.view_as_real(over), torch.view_as_real(ops.phase_vocoder(spec.cuda(), 0.7)[0]))
    lead = tr.TimeStretch()(spec.reshape(3, 1, 257, -1).repeat(1, 2, 1, 1), 1.1)     # any leading shape
    assert lead.shape == (3, 2, 257, want.shape[2]) and torch.equal(torch.view_as_real(lead[:, 1]), torch.view_as_real(want.cpu()))
    c64 = ts(spec.to(torch.complex64))
    assert c64.dtype == torch.complex64 and c64.shape == want.shape
    with pytest.raises(ValueError, match="If no fixed_rate is specified"):
        tr.TimeStretch()(spec)
    with pytest.raises(NotImplementedError):
        tr.TimeStretch(n_freq=201)
    x = torch.rand(3, 8000, generator=torch.Generator().manual_seed(3)) * 2 - 1
    sp = tr.Speed(8000, 1.1)
    y, lengths = sp(x, torch.tensor([8000, 4400, 100]))
    assert torch.equal(y, ops.resample(x.cuda(), 11, 10).cpu()) and y.shape == (3, 7273) and lengths.tolist() == [7273, 4000, 91]
    assert sp(x)[1] is None
    for steps, ratio in ((12, Fraction(2)), (-1, Fraction(151, 160))):
        ps = tr.PitchShift(8000, steps)
        y = ps(x)
        assert y.shape == x.shape and y.device.type == "cpu" and ps.ratio == ratio
        assert torch.equal(y, ops.pitch_shift(x.cuda(), ratio, rates=2.0 ** (-steps / 12)).cpu())
    with pytest.raises(ValueError):
        tr.PitchShift(8000, 2)


def _augmentations():
    from musicfpaugment_amd.augmentation.transformations.pitch_shift import PitchShift
    from musicfpaugment_amd.augmentation.transformations.time_stretch import TimeStretch
    return PitchShift, TimeStretch


@pytest.mark.parametrize("which", (0, 1), ids=("PitchShift", "TimeStretch"))
def test_augmentation_gate_parameters_and_freezing(ops, which):
    cls = _augmentations()[which]
    key = ("transpositions", "rates")[which]
    x = (torch.rand(4, 1, 8000, generator=torch.Generator().manual_seed(11)) * 2 - 1).cuda()
    off = cls(p=0.0, sample_rate=8000)
    out = off(x)
    assert torch.equal(out.samples, x) and out.sample_rate == 8000 and len(off.transform_parameters[key]) == 0
    on = cls(p=1.0, sample_rate=8000)
    on.freeze_parameters(seed=7)
    first = on(x).samples
    params = on.transform_parameters[key]
    assert first.shape == x.shape and first.dtype == torch.float32 and len(params) == 4 and on.transform_parameters["should_apply"].all()
    assert all(not torch.equal(first[b], x[b]) for b in range(4))
    if which == 0:
        assert all(isinstance(f, Fraction) and f in on.candidates for f in params)
        assert torch.equal(first[:, 0], ops.pitch_shift(x[:, 0].contiguous(), list(params)))
    else:
        assert params.shape == (4,) and bool(((params >= 0.8) & (params <= 1.25)).all())
        for b, r in enumerate(params.tolist()):
            L = round(8000 / r)
            assert L >= 8000 or not first[b, 0, L:].any()                             # a faster clip is zero-padded at its end
    on.freeze_parameters(seed=7)
    again = on(x).samples
    assert torch.equal(again, first) and list(on.transform_parameters[key]) == list(params)
    half = cls(p=0.5, sample_rate=8000)
    half.freeze_parameters(seed=7)
    mixed = half(x).samples
    should = half.transform_parameters["should_apply"]
    assert 0 < int(should.sum()) < 4 and len(half.transform_parameters[key]) == int(should.sum())
    for b in range(4):
        assert torch.equal(mixed[b], x[b]) != bool(should[b]), b                     # unselected examples come back bit for bit


def test_augmentations_inside_compositions_and_the_base_class_errors():
    from musicfpaugment_amd.augmentation.composition import Compose, OneOf, SomeOf
    from musicfpaugment_amd.augmentation.transform import MultichannelAudioNotSupportedException
    from musicfpaugment_amd.augmentation.transformations.gain import Gain
    PitchShift, TimeStretch = _augmentations()
    x = (torch.rand(3, 1, 8000, generator=torch.Generator().manual_seed(12)) * 2 - 1).cuda()
    chain = Compose([Gain(p=1.0), PitchShift(p=1.0), TimeStretch(p=1.0)])
    chain.freeze_parameters(seed=5)
    out = chain(x, sample_rate=8000)
    assert out.samples.shape == x.shape and out.sample_rate == 8000 and bool(torch.isfinite(out.samples).all())
    g, ps, st = chain.transforms
    chain.freeze_parameters(seed=5)
    assert torch.equal(chain(x, sample_rate=8000).samples, out.samples)
    assert len(ps.transform_parameters["transpositions"]) == 3 and st.transform_parameters["rates"].shape == (3,)
    for comp in (OneOf([PitchShift(p=1.0), TimeStretch(p=1.0)]), SomeOf((1, 2), [PitchShift(p=1.0), TimeStretch(p=1.0), Gain(p=1.0)])):
        res = comp(x, sample_rate=8000)
        assert res.samples.shape == x.shape and not torch.equal(res.samples, x)
    for t in (PitchShift(p=1.0), TimeStretch(p=1.0)):
        with pytest.raises(RuntimeError, match="sample_rate is required"):
            t(x)
        with pytest.raises(MultichannelAudioNotSupportedException):
            t(x.repeat(1, 2, 1), 8000)
