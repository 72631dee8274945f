"""GPU: the composable transforms (csrc/transforms.hip and the augmentation.transformations / augmentation.composition classes)
against the float64 restatements of tests/_transforms_oracle.py, golden g19 (the real _gen_noise) and AugmentFP itself.

Tolerance of the coloured noise (measured, not assumed): golden g19 holds the reference's own float32 result, so
err_ref = max|golden - oracle| is what float32 costs the REFERENCE; the device (another factorisation order, a float32 powf) must
stay within 4 x err_ref.  Sizes without a golden case take the largest err_ref of a golden size at least as large; sizes above
every golden one (16000 and the cap) take the error of the same float32 formula evaluated by torch on the CPU on the test's own
white noise -- which is how the reference would compute them.  The ratios measured on an MI355X are in NOTES.md."""
import math
import random

import numpy as np
import pytest
import torch

from musicfpaugment_amd import synth
from tests import _transforms_oracle as to

pytestmark = pytest.mark.gpu

CAP = 16384
DECAYS = (-2.0, -1.0, 0.0, 1.0, 2.0)


def _lib():
    from musicfpaugment_amd._lib import check, lib, ptr, stream
    return check, lib(), ptr, stream


@pytest.fixture(scope="module")
def g19(golden):
    return golden("g19_colored_noise")


@pytest.fixture(scope="module")
def ref_err(g19):
    return to.reference_error(g19)


def _formula_f32(white: np.ndarray, fd: float, T: int) -> np.ndarray:
    """colored_noise.py:30-38 in float32 with torch on the CPU, for given white noise."""
    w = torch.from_numpy(white)
    N = w.shape[0]
    spec = torch.fft.rfft(w)
    spec = spec * (1 / (torch.linspace(1, (N / 2) ** 0.5, spec.shape[0]) ** torch.tensor(fd, dtype=torch.float32)))
    x = torch.fft.irfft(spec)
    x = x / (x.square().mean().sqrt() + 1e-8)
    return torch.cat([x] * int(math.ceil(T / N)))[:T].numpy()


def _white(N: int, B: int = 5) -> np.ndarray:
    return np.random.default_rng(1900 + N).standard_normal((B, N)).astype(np.float32)


def test_colored_noise_against_the_golden_cases(g19):
    from musicfpaugment_amd import ops
    worst = {}
    for sr, white, fd, T, y in to.g19_cases(g19):
        want = to.colored_noise(white, fd, T)
        err_ref = np.abs(y.astype(np.float64) - want).max()
        got = ops.colored_noise(torch.from_numpy(white)[None].cuda(), torch.tensor([fd], device="cuda"), T).cpu().numpy()[0]
        err = np.abs(got.astype(np.float64) - want).max()
        print(f"g19 N={sr} f_decay={fd:+.0f} T={T}: device {err:.3e}  reference {err_ref:.3e}  ratio {err / err_ref:.2f}")
        worst[sr] = max(worst.get(sr, 0.0), err / err_ref)
        assert err <= 4 * err_ref, (sr, fd, T, err, err_ref)
    print("worst ratio per size:", {k: round(v, 2) for k, v in worst.items()})


@pytest.mark.parametrize("N", [8, 12, 20, 30, 600, 1000, 8000, 16000, CAP])
def test_colored_noise_every_radix_and_length(N, ref_err):
    """Every radix alone (8: 4, 12: 3 2, 20: 5 2 -- and 4, 6, 10 below), every pair, the two real sizes and the largest; f_decay
    mixed within the batch; T below, at and above one period."""
    from musicfpaugment_amd import ops
    white = _white(N)
    fd = np.array(DECAYS, dtype=np.float32)
    at_least = [e for sr, e in ref_err.items() if sr >= N]
    if at_least:
        err_ref = max(at_least)
    else:
        err_ref = max(np.abs(_formula_f32(white[b], float(fd[b]), N).astype(np.float64) - to.colored_noise(white[b], fd[b], N)).max()
                      for b in range(5))
    wd, fdd = torch.from_numpy(white).cuda(), torch.from_numpy(fd).cuda()
    full = to.colored_noise(white, fd, 3 * N + 1)
    for T in (1, N - 1, N, N + 1, 3 * N + 1):
        got = ops.colored_noise(wd, fdd, T)
        assert got.shape == (5, T) and got.dtype == torch.float32
        err = np.abs(got.cpu().numpy().astype(np.float64) - full[:, :T]).max(axis=1)
        if T == 3 * N + 1:
            print(f"N={N}: device {err.max():.3e}  reference {err_ref:.3e}  ratio {err.max() / err_ref:.2f}  per f_decay {np.round(err / err_ref, 2)}")
        assert err.max() <= 4 * err_ref, (N, T, err, err_ref)


@pytest.mark.parametrize("N", [4, 6, 10])
def test_colored_noise_single_pass_sizes(N, ref_err):
    from musicfpaugment_amd import ops
    white = _white(N)
    fd = np.array(DECAYS, dtype=np.float32)
    got = ops.colored_noise(torch.from_numpy(white).cuda(), torch.from_numpy(fd).cuda(), 2 * N + 1).cpu().numpy()
    assert np.abs(got.astype(np.float64) - to.colored_noise(white, fd, 2 * N + 1)).max() <= 4 * max(ref_err.values())


@pytest.mark.parametrize("N", [30, 8000, CAP])
def test_colored_noise_is_independent_of_batch_row_and_length(N):
    from musicfpaugment_amd import ops
    white, fd = torch.from_numpy(_white(N)).cuda(), torch.tensor(DECAYS, device="cuda")
    batch = ops.colored_noise(white, fd, N)
    long = ops.colored_noise(white, fd, 3 * N + 1)
    assert torch.equal(long[:, :N], batch) and torch.equal(long[:, N:2 * N], batch) and torch.equal(long[:, 3 * N], batch[:, 0])
    assert torch.equal(ops.colored_noise(white, fd, N - 1), batch[:, :N - 1])
    big_w, big_f = torch.randn(64, N, device="cuda"), torch.zeros(64, device="cuda")
    for b in range(5):
        alone = ops.colored_noise(white[b:b + 1].clone(), fd[b:b + 1].clone(), N)
        assert torch.equal(alone[0], batch[b]), b
        big_w[0], big_f[0] = white[b], fd[b]
        assert torch.equal(ops.colored_noise(big_w, big_f, N)[0], batch[b]), b
    assert torch.equal(ops.colored_noise(white, fd, N + 3), torch.cat([batch, batch[:, :3]], dim=1))


def test_colored_noise_rows_off_a_16_byte_boundary():
    """T = 4k+1, 4k+2, 4k+3: every row but the first starts 4, 8 or 12 bytes past a 16-byte boundary (scalar head, float4 body, tail)."""
    from musicfpaugment_amd import ops
    N = 600
    white, fd = torch.from_numpy(_white(N)).cuda(), torch.tensor(DECAYS, device="cuda")
    one = ops.colored_noise(white, fd, N)
    for T in (1, 2, 3, 5, 6, 7, 1201, 1202, 1203):
        got = ops.colored_noise(white, fd, T)
        assert torch.equal(got, one.repeat(1, 3)[:, :T]), T


@pytest.mark.parametrize("lo,hi", [(0.02, 0.3), (0.1, 0.5), (1.25e-4, 0.2), (0.249, 0.251)])
def test_bandpass_taps_and_fir_against_the_oracle(lo, hi):
    """The tolerances tests/test_gpu_augment.py uses for the pass filters: 2e-7 on the taps, 2e-5 on the outputs."""
    check, L, ptr, stream = _lib()
    from musicfpaugment_amd import ops
    T = 16000
    x = torch.from_numpy(synth.batch(2, seed=1900, n=T))
    taps, off_d, ntaps_d, half_d = ops.bandpass_taps([lo, lo], [hi, hi])
    n = 2 * int(8 / lo / 2) + 1
    assert ntaps_d.tolist() == [n, n] and off_d.tolist() == [0, n] and half_d.tolist() == [n // 2] * 2 and taps.shape == (2 * n,)
    if lo == 1.25e-4:
        assert n == 64001
    want_taps = to.bandpass_taps(lo, hi)
    got_taps = taps.cpu().numpy()
    assert np.array_equal(got_taps[:n], got_taps[n:])
    print(f"band ({lo}, {hi}): {n} taps, max |taps - oracle| {np.abs(got_taps[:n] - want_taps).max():.3e}, sum {got_taps[:n].astype(np.float64).sum():.3e}")
    np.testing.assert_allclose(got_taps[:n], want_taps, rtol=0, atol=2e-7)
    xd, on = x.cuda(), torch.tensor([1, 1], dtype=torch.uint8, device="cuda")
    want = np.stack([to.bandpass(x[b].numpy(), lo, hi) for b in range(2)])
    for mode in (0, 1):
        y = torch.empty_like(xd)
        check(L.mfpa_fir(ptr(xd), 2, T, T, ptr(taps), ptr(off_d), ptr(ntaps_d), ptr(half_d), ptr(on), 0, mode, ptr(y), 0, stream()), "fir")
        ref = want if mode == 0 else x.numpy().astype(np.float64) - want
        print(f"  out_mode {mode}: max |y - oracle| {np.abs(y.cpu().numpy() - ref).max():.3e}")
        np.testing.assert_allclose(y.cpu().numpy(), ref, rtol=0, atol=2e-5)


def _chain(scope, irs, noises):
    from musicfpaugment_amd.augmentation.composition import Compose
    from musicfpaugment_amd.augmentation.constants import DEFAULT_PARAMETERS as P
    from musicfpaugment_amd.augmentation.transformations.background_noise import AddBackgroundNoise
    from musicfpaugment_amd.augmentation.transformations.clipping import Clipping
    from musicfpaugment_amd.augmentation.transformations.gain import Gain
    from musicfpaugment_amd.augmentation.transformations.impulse_response import ApplyImpulseResponse
    from musicfpaugment_amd.augmentation.transformations.pass_filters import HighPassFilter, LowPassFilter
    from musicfpaugment_amd.augmentation.transformations.peak_normalization import PeakNormalization
    return Compose([
        HighPassFilter(P["min_cutoff_freq1"], P["max_cutoff_freq1"], p=P["proba_cutoff_freq1"], sample_rate=8000),
        ApplyImpulseResponse(None, 8000, p=P["proba_ir_response"], ir_bank=irs),
        AddBackgroundNoise(None, P["min_snr_in_db"], P["max_snr_in_db"], p=P["proba_snr_in_db"], sample_rate=8000, noise_bank=noises),
        Gain(P["min_gain_in_db"], P["max_gain_in_db"], p=P["proba_gain_in_db"]),
        Clipping(0.0, P["max_percentile_threshold"], p=P["proba_percentile_threshold"], scope=scope),
        LowPassFilter(P["min_cutoff_freq2"], P["max_cutoff_freq2"], p=P["proba_cutoff_freq2"], sample_rate=8000),
        HighPassFilter(P["min_cutoff_freq3"], P["max_cutoff_freq3"], p=P["proba_cutoff_freq3"], sample_rate=8000),
        PeakNormalization(p=1.0)])


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu())
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))
    return a == b


@pytest.mark.parametrize("scope", ["example", "batch"])
@pytest.mark.parametrize("seed", [14, 16])
def test_compose_of_the_eight_stages_is_augmentfp_bit_for_bit(seed, scope):
    from musicfpaugment_amd.augmentation import AugmentFP, synthetic_banks
    irs, noises = synthetic_banks(0)
    wav = torch.from_numpy(synth.batch(6, seed=1910, n=16000))[:, None, :].cuda()
    af = AugmentFP(None, 8000, ir_bank=irs, noise_bank=noises, clipping_scope=scope)
    chain = _chain(scope, irs, noises)
    random.seed(seed)
    torch.manual_seed(seed)
    want = af.batch_augment(wav)
    state = (random.getstate(), torch.get_rng_state())
    random.seed(seed)
    torch.manual_seed(seed)
    got = chain(wav, sample_rate=8000)
    assert random.getstate() == state[0] and torch.equal(torch.get_rng_state(), state[1])     # the same draws, no more, no fewer
    assert got.sample_rate == 8000 and got.samples.shape == want.shape == (6, 1, 16000)
    assert torch.equal(got.samples, want)
    stages = af.augmentation_pipeline.transforms
    assert len(stages) == len(chain.transforms) == 8
    for old, new in zip(stages, chain.transforms):
        assert type(new).__name__ == old.name
        assert set(new.transform_parameters) == set(old.transform_parameters), old.name
        for k, v in old.transform_parameters.items():
            assert _same(v, new.transform_parameters[k]), (old.name, k)
    for old in stages[:7]:                                      # the seeds were chosen so: every gate is on somewhere and off somewhere
        g = old.transform_parameters["should_apply"]
        assert bool(g.any()) and not bool(g.all()), (old.name, g)
    assert bool(stages[7].transform_parameters["should_apply"].all())


def test_add_colored_noise_is_the_mix_of_the_oracle_noise():
    from musicfpaugment_amd.augmentation.transformations.colored_noise import AddColoredNoise
    from oracle import augment as oau
    wav = torch.from_numpy(synth.batch(4, seed=1920, n=12001))[:, None, :]
    t = AddColoredNoise(min_snr_in_db=3.0, max_snr_in_db=30.0, p=1.0, sample_rate=8000)
    torch.manual_seed(3)
    out = t(wav.cuda())
    assert out.sample_rate == 8000 and out.samples.shape == wav.shape and out.samples.is_cuda
    par = t.transform_parameters
    assert set(par) == {"should_apply", "snr_in_db", "f_decay"} and par["should_apply"].all()
    assert par["snr_in_db"].shape == par["f_decay"].shape == (4,) and t.white.shape == (4, 8000)
    assert bool(((par["snr_in_db"] >= 3) & (par["snr_in_db"] <= 30) & (par["f_decay"] >= -2) & (par["f_decay"] <= 2)).all())
    noise = to.colored_noise(t.white.cpu().numpy(), par["f_decay"].numpy(), 12001)
    want = oau.add_background(wav, torch.from_numpy(noise.astype(np.float32)), par["snr_in_db"])
    got = out.samples.cpu()
    print(f"AddColoredNoise: max |y - mix(oracle noise)| {float((got - want).abs().max()):.3e}")
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=2e-6)        # the mix tolerance tests/test_gpu_augment.py uses
    assert torch.equal(got.abs().amax(dim=2), torch.ones(4, 1))
    torch.manual_seed(3)                                        # the draws: gate, snr, f_decay (host), then one normal (device)
    gate = torch.distributions.Bernoulli(1.0).sample((4,))
    snr = torch.distributions.Uniform(torch.tensor(3.0), torch.tensor(30.0)).sample((4,))
    f_decay = torch.distributions.Uniform(torch.tensor(-2.0), torch.tensor(2.0)).sample((4,))
    assert gate.all() and torch.equal(snr, par["snr_in_db"]) and torch.equal(f_decay, par["f_decay"])
    assert torch.equal(torch.normal(0.0, 1.0, (4, 8000), device="cuda"), t.white)


def test_band_stop_plus_band_pass_is_the_input():
    from musicfpaugment_amd.augmentation.transformations.band_filters import BandPassFilter, BandStopFilter
    wav = torch.from_numpy(synth.batch(5, seed=1930, n=9000))[:, None, :].cuda()
    bp, bs = BandPassFilter(p=1.0, sample_rate=8000, max_center_frequency=2000), BandStopFilter(p=1.0, sample_rate=8000, max_center_frequency=2000)
    torch.manual_seed(11)
    a = bp(wav).samples
    torch.manual_seed(11)
    b = bs(wav).samples
    for k in ("should_apply", "center_freq", "bandwidth"):
        assert torch.equal(bp.transform_parameters[k], bs.transform_parameters[k])
    assert set(bp.transform_parameters) == {"should_apply", "center_freq", "bandwidth"}
    c, w = bp.transform_parameters["center_freq"], bp.transform_parameters["bandwidth"]
    assert bool(((c >= 199.9) & (c <= 2000.1) & (w >= 0.5) & (w <= 1.99)).all())
    np.testing.assert_allclose((a + b).cpu().numpy(), wav.cpu().numpy(), rtol=0, atol=2e-5)
    assert float(a.abs().max()) > 0.01 and float(b.abs().max()) > 0.01
    b0 = to.bandpass(wav[0, 0].cpu().numpy(), float(c[0] * (1 - 0.5 * w[0]) / 8000), float(c[0] * (1 + 0.5 * w[0]) / 8000))
    np.testing.assert_allclose(a[0, 0].cpu().numpy(), b0, rtol=0, atol=2e-5)


def _every_transform(irs, noises):
    from musicfpaugment_amd.augmentation.transformations.band_filters import BandPassFilter, BandStopFilter
    from musicfpaugment_amd.augmentation.transformations.colored_noise import AddColoredNoise
    chain = _chain("example", irs, noises)
    return list(chain.transforms) + [BandPassFilter(sample_rate=8000, max_center_frequency=2000),
                                     BandStopFilter(sample_rate=8000, max_center_frequency=2000), AddColoredNoise(sample_rate=8000)]


def test_p_zero_copies_through_and_frozen_parameters_repeat():
    from musicfpaugment_amd.augmentation import synthetic_banks
    from musicfpaugment_amd.augmentation.composition import Compose, OneOf, SomeOf
    irs, noises = synthetic_banks(0)
    wav = torch.from_numpy(synth.batch(3, seed=1940, n=8000))[:, None, :].cuda()
    keep = wav.clone()
    ts = _every_transform(irs, noises)
    assert len(ts) == 11
    for t in ts:
        t.p = 0.0
        out = t(wav, 8000)
        assert torch.equal(out.samples, keep) and not t.transform_parameters["should_apply"].any(), type(t).__name__
        t.p = 1.0
        t.freeze_parameters(5)
        a = t(wav, 8000).samples.clone()
        t.freeze_parameters(5)
        b = t(wav, 8000).samples
        assert torch.equal(a, b) and torch.isfinite(a).all() and a.shape == wav.shape, type(t).__name__
        assert type(t).__name__ == "PeakNormalization" or not torch.equal(a, keep), type(t).__name__
        t.p = 0.5
    assert torch.equal(wav, keep)                               # no transform writes into its input
    chain = Compose([SomeOf((1, 3), ts[:4]), OneOf(ts[8:]), ts[7]], shuffle=True)
    chain.freeze_parameters(9)
    a = chain(wav, 8000).samples.clone()
    chain.freeze_parameters(9)
    assert torch.equal(chain(wav, 8000).samples, a) and a.is_cuda and torch.isfinite(a).all()


def test_error_cases():
    from musicfpaugment_amd.augmentation.transform import MultichannelAudioNotSupportedException
    from musicfpaugment_amd.augmentation.transformations.band_filters import BandPassFilter
    from musicfpaugment_amd.augmentation.transformations.colored_noise import AddColoredNoise
    from musicfpaugment_amd.augmentation.transformations.gain import Gain
    wav = torch.from_numpy(synth.batch(2, seed=1950, n=4000))[:, None, :].cuda()
    high = BandPassFilter(min_center_frequency=3800, max_center_frequency=3900, min_bandwidth_fraction=0.5, max_bandwidth_fraction=0.6,
                          p=1.0, sample_rate=8000)                  # upper cut-off >= 3800 * 1.25 / 8000 = 0.59
    with pytest.raises(ValueError, match="A cutoff above 0.5 does not make sense."):
        high(wav)
    high.p = 0.0
    assert torch.equal(high(wav).samples, wav)                  # ... but a band nobody applies is not an error
    with pytest.raises(ValueError, match="2\\^a 3\\^b 5\\^c"):
        AddColoredNoise(sample_rate=44100)
    with pytest.raises(MultichannelAudioNotSupportedException):
        Gain(p=1.0)(torch.cat([wav, wav], dim=1))
    with pytest.raises(RuntimeError, match="three-dimensional"):
        Gain(p=1.0)(wav[:, 0])
    with pytest.warns(UserWarning, match="empty"):
        empty = wav[:0]
        assert Gain(p=1.0)(empty).samples is empty
