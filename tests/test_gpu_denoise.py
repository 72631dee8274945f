"""GPU: csrc/denoise.hip (ops.spectral_suppress) against tests/_denoise_oracle.py BIT FOR BIT -- y, g and n -- and the fronts over
it: SpectralDenoiser in the UNet's slot of both fingerprinters and as a waveform denoiser, functional.spectral_denoise, the
NoiseSuppression transform.

The definition is a serial chain of correctly rounded float64 operations around a minimum that selects and never rounds, so there
is no tolerance anywhere in the kernel's tests: a differing bit is a contraction, a reordered sum or a scan in the kernel.

Shapes: F of (1, 63, 64, 65, 257): one partial workgroup of 16 bins, the last full one, one bin spilling into the next.  nF of
(1, 2, ahead, ahead + 1, W - 1, W, W + 1, 63, 64, 65, 251, 2 W + 3, 1500) and the kernel's own edges (15, 16, 17: the minimum's
frame groups; 127, 128, 129: two tiles of 64 frames), crossed at F = 65 with the windows (0,0), (0,5), (5,0), (48,48) and (63,64),
the largest (W = 128 = MFPA_DENOISE_MAX_WINDOW): windows below 16 frames take the direct minimum, the others the block scheme; the
gain walk lags the s walk by ceil(ahead / 64) tiles -- none for (0, 0) and (5, 0), one for the others; test_two_tiles_of_lag adds
(20, 100)."""
import functools
import random

import numpy as np
import pytest
import torch

from tests import _denoise_oracle as o

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
T64, T32 = torch.float64, torch.float32


def _ops():
    from musicfpaugment_amd import ops
    return ops


def _dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def _compare(tag, m, *, in_dtype=T64, out_dtype=None, noise=None, denom=None, apply=None, **kw):
    """ops.spectral_suppress on m (B, F, nF) float64 (rounded to float32 first when in_dtype says so) against the oracle: all bits."""
    ops = _ops()
    m_in = m.astype(np.float32) if in_dtype == T32 else m
    okw = {k: v for k, v in kw.items() if k in ("alpha", "back", "ahead", "bias")}
    if "dd" in kw:
        okw["a"] = kw["dd"]
    okw["xi_min"], okw["g_floor"] = ops.suppress_thresholds(kw.get("xi_min_db", -25.0), kw.get("floor_db", -20.0))
    want_y, want_g, want_n = o.suppress(m_in, noise=noise, denom=denom, apply=apply, **okw)
    y, g, n = ops.spectral_suppress(_dev(m_in), noise_psd=None if noise is None else _dev(noise), denom=None if denom is None else _dev(denom),
                                    apply=apply, out_dtype=out_dtype, return_gain=True, return_noise=True, **kw)
    want_dtype = out_dtype or in_dtype
    assert y.dtype == want_dtype and g.dtype == T64 and n.dtype == T64 and y.shape == g.shape == n.shape == m.shape
    if want_dtype == T32:
        want_y = want_y.astype(np.float32)                                    # the float64 value rounded once
    for name, got, want in (("n", n, want_n), ("g", g, want_g), ("y", y, want_y)):
        got = got.cpu().numpy()
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            pytest.fail(f"{tag}: {name} differs in {len(bad)} of {want.size} elements, first at (b, k, t) = {bad[0].tolist()}: "
                        f"{got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}")
    return y, g, n


@pytest.mark.parametrize("F", o.F_LIST)
def test_bins(F):
    _compare(f"F={F}", o.magnitudes(F, 251))


@pytest.mark.parametrize("back,ahead", o.WINDOWS, ids=lambda v: str(v))
def test_windows_crossed_with_frame_counts(back, ahead):
    for nF in o.frames_list(back, ahead):
        _compare(f"window ({back}, {ahead}) nF={nF}", o.magnitudes(65, nF), back=back, ahead=ahead)


def test_two_tiles_of_lag():
    for nF in (1, 64, 100, 101, 121, 129, 300):
        _compare(f"window (20, 100) nF={nF}", o.magnitudes(33, nF), back=20, ahead=100)


def test_one_clip():
    _compare("B=1", o.magnitudes(65, 251)[4:5])
    _compare("B=1, the zeros-then-signal row", o.magnitudes(65, 251)[1:2])


@pytest.mark.parametrize("in_dtype,out_dtype", [(T32, None), (T32, T64), (T64, T32), (T64, T64), (T32, T32)], ids=str)
def test_dtypes(in_dtype, out_dtype):
    _compare(f"{in_dtype} -> {out_dtype}", o.magnitudes(65, 251), in_dtype=in_dtype, out_dtype=out_dtype)


@pytest.mark.parametrize("with_noise", [False, True])
@pytest.mark.parametrize("with_denom", [False, True])
@pytest.mark.parametrize("with_apply", [False, True])
def test_noise_psd_denominator_and_gate(with_noise, with_denom, with_apply):
    m = o.magnitudes(65, 131)
    rng = np.random.default_rng(11)
    noise = 10.0 ** rng.uniform(-4.0, 2.0, (5, 65))
    noise[0, 0] = 0.0                                                         # the DBL_MIN floor
    denom = m.reshape(5, -1).max(axis=1)
    denom[2] = 1.0                                                            # the all-zero row
    gate = [True, False, True, True, False]
    y, g, n = _compare(f"noise={with_noise} denom={with_denom} apply={with_apply}", m, noise=noise if with_noise else None,
                       denom=denom if with_denom else None, apply=gate if with_apply else None, out_dtype=T32 if with_denom else None)
    if with_apply:                                                            # a gated row is its input, or its input over denom
        off = [1, 4]
        want = m[off] / denom[off, None, None] if with_denom else m[off]
        assert np.array_equal(y[off].cpu().numpy(), want.astype(np.float32) if with_denom else want)
        assert bool((g[off] == 1.0).all()) and bool((g[[0, 2, 3]] < 1.0).any())


def test_other_parameters_and_floors_per_clip():
    m = o.magnitudes(40, 200)
    _compare("alpha 0, dd 0", m, alpha=0.0, dd=0.0, bias=1.0)
    _compare("alpha 0.95, dd 0.98, deep floor", m, alpha=0.95, dd=0.98, bias=1.5, xi_min_db=-40.0, floor_db=-60.0)
    _compare("no floor at all", m, floor_db=0.0)
    ops = _ops()
    floors = [-30.0, -10.0, -20.0, 0.0, -3.5]
    y = ops.spectral_suppress(_dev(m), floor_db=floors)
    for b, f in enumerate(floors):
        assert torch.equal(y[b:b + 1], ops.spectral_suppress(_dev(m[b:b + 1]), floor_db=f)), b


def test_rows_do_not_depend_on_the_batch_and_flags_do_not_change_y():
    ops = _ops()
    m = _dev(o.magnitudes(257, 251))
    y, g, n = ops.spectral_suppress(m, return_gain=True, return_noise=True)
    for b in range(5):
        yb, gb, nb = ops.spectral_suppress(m[b:b + 1].contiguous(), return_gain=True, return_noise=True)
        assert torch.equal(yb[0], y[b]) and torch.equal(gb[0], g[b]) and torch.equal(nb[0], n[b]), b
    assert torch.equal(ops.spectral_suppress(m), y)
    y1, g1 = ops.spectral_suppress(m, return_gain=True)
    y2, n2 = ops.spectral_suppress(m, return_noise=True)
    assert torch.equal(y1, y) and torch.equal(y2, y) and torch.equal(g1, g) and torch.equal(n2, n)
    big = m.repeat(13, 1, 1)                                                  # 65 clips: the rows again, wherever they stand
    assert torch.equal(ops.spectral_suppress(big).reshape(13, 5, 257, 251), y.expand(13, 5, 257, 251))


# ----------------------------------------------------------------------------- the fronts
@functools.lru_cache(maxsize=None)
def _chain_case(kind, snr_in):
    """(clean, noisy, the oracle chain's output SNR): the inputs of tests/test_denoise_oracle.py, computed once."""
    clean = o.tonal()
    x = o.noisy(clean, kind, snr_in)
    return clean, x, o.snr_db(clean, o.chain(x))


def _noisy_batch():
    return torch.from_numpy(np.stack([_chain_case(k, s)[1] for k, s in o.CHAIN_CASES])).float().to(DEV)


def test_denoise_spectrogram_is_the_op_with_the_maxima_as_denominator():
    from musicfpaugment_amd.denoisers import SpectralDenoiser
    ops = _ops()
    net = SpectralDenoiser().to(DEV).eval()
    mag, cmax = ops.stft_mag(_noisy_batch(), T64)
    got = net.denoise_spectrogram(mag, cmax, per_clip=True)
    assert got.dtype == T32 and torch.equal(got, ops.spectral_suppress(mag, denom=cmax, out_dtype=T32))
    both = net.denoise_spectrogram(mag, cmax, per_clip=False)
    assert torch.equal(both, ops.spectral_suppress(mag, denom=cmax.max().expand(4).contiguous(), out_dtype=T32))
    other = SpectralDenoiser(floor_db=-6.0, dd=0.5, back=10, ahead=3)
    assert torch.equal(other.denoise_spectrogram(mag, cmax, True),
                       ops.spectral_suppress(mag, denom=cmax, out_dtype=T32, floor_db=-6.0, dd=0.5, back=10, ahead=3))


def test_denoise_waveform_is_the_three_ops_and_matches_the_oracle_chain_snr():
    from musicfpaugment_amd import functional as F
    from musicfpaugment_amd.denoisers import SpectralDenoiser
    ops = _ops()
    net = SpectralDenoiser().to(DEV).eval()
    x = _noisy_batch()
    y = net.denoise_waveform(x)
    spec, mag, _ = ops.stft_complex(x, want_mag=True)
    assert y.dtype == T32 and torch.equal(y, ops.istft(spec, x.shape[1], mag=ops.spectral_suppress(mag)))
    out = net(x)
    assert out.shape == (4, 1, x.shape[1]) and torch.equal(out[:, 0], y) and torch.equal(net(x[:, None, :]), out)
    assert torch.equal(F.spectral_denoise(x.reshape(2, 2, -1), 8000), y.reshape(2, 2, -1))
    assert torch.equal(F.spectral_denoise(x[0].cpu(), 8000), y[0].cpu())
    for i, (kind, snr_in) in enumerate(o.CHAIN_CASES):
        clean, _, want = _chain_case(kind, snr_in)
        got = o.snr_db(clean, y[i].double().cpu().numpy())
        print(f"{kind} noise at {snr_in} dB: device {got:.3f} dB, oracle chain {want:.3f} dB")
        assert abs(got - want) < 0.1 and got > snr_in + 3.0


def test_audfprint_takes_it_in_the_unet_slot():
    from musicfpaugment_amd.afp.audfprint.peak_extractor import Audfprint_peaks
    from musicfpaugment_amd.denoisers import SpectralDenoiser
    ops = _ops()
    x = _noisy_batch()
    ext = Audfprint_peaks(None, denoising=True, denoising_model="unet", unet=SpectralDenoiser(), device=DEV)
    mask, npk, spec = ext.find_peaks_batch(x)
    mag, cmax = ops.stft_mag(x, T64)
    want_spec = ops.spectral_suppress(mag, denom=cmax, out_dtype=T32)
    filtered = ops.audfprint_prepare(want_spec, None, mean_order=0, float32_log=ext.float32_log)
    want_mask, want_npk = ops.audfprint_prune(filtered, ops.audfprint_a_dec(ext.density, ext.n_hop), ext.maxpksperframe, float(ext.f_sd))
    assert torch.equal(spec, want_spec) and torch.equal(mask, want_mask) and torch.equal(npk, want_npk) and int(npk.min()) > 0


def test_dejavu_takes_it_in_the_unet_slot_in_the_power_domain():
    from musicfpaugment_amd.afp.dejavu import fingerprint as fp
    from musicfpaugment_amd.denoisers import SpectralDenoiser
    ops = _ops()
    x = _noisy_batch()
    net = SpectralDenoiser(domain="power")
    mask, npk, spec = fp.fingerprint_peaks_batch(x, denoising=True, denoising_model="unet", unet=net)
    psd, cmax = ops.specgram_psd(x, scale_in=32767.0)
    _, g = ops.spectral_suppress(torch.sqrt(psd), return_gain=True)
    want = (g * g * psd / cmax[:, None, None]).cpu().numpy()
    # spec = y * y in float32 with y = float32(g sqrt(psd) / sqrt(cmax)): 2^-24 on y doubles in the square, 2^-24 for the product
    np.testing.assert_allclose(spec.cpu().numpy(), want, rtol=2.0 ** -22, atol=1e-30)
    assert spec.dtype == T32 and mask.shape == spec.shape and int(npk.min()) > 0
    old = dict(fp._DENOISERS)
    try:
        fp.set_denoisers(unet=net)
        assert fp._DENOISERS["unet"] is net
    finally:
        fp._DENOISERS.update(old)


def test_noise_suppression_keeps_unselected_rows_and_composes():
    from musicfpaugment_amd.augmentation.composition import Compose, OneOf, SomeOf
    from musicfpaugment_amd.augmentation.transformations.noise_suppression import NoiseSuppression
    ops = _ops()
    x = _noisy_batch()[:, :8000].contiguous()
    t = NoiseSuppression(p=0.5)
    random.seed(1)
    torch.manual_seed(1)
    out = t(x.unsqueeze(1), 8000).samples[:, 0]
    should = t.transform_parameters["should_apply"]
    assert 0 < int(should.sum()) < 4, "the seed must select some rows and leave some"
    on, off = should.to(DEV), ~should.to(DEV)
    assert torch.equal(out[off], x[off]) and not torch.equal(out[on], x[on])
    spec, mag, _ = ops.stft_complex(x, want_mag=True)
    by_hand = ops.istft(spec, 8000, mag=ops.spectral_suppress(mag, floor_db=t.floors()))
    assert torch.equal(out[on], by_hand[on])
    random.seed(1)
    torch.manual_seed(1)
    chain = Compose([NoiseSuppression(p=1.0), SomeOf((1, 2), [NoiseSuppression(p=1.0), NoiseSuppression(p=1.0)]), OneOf([NoiseSuppression(p=1.0)])])
    got = chain(x.unsqueeze(1), 8000).samples
    assert got.shape == (4, 1, 8000) and torch.isfinite(got).all() and not torch.equal(got[:, 0], x)
