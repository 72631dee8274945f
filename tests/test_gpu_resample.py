"""GPU: the device resampler (csrc/resample.hip) against the float64 restatement of torchaudio's Resample
(tests/_resample_oracle.py), its bit-for-bit independence of batch, tile, row pitch and the memory behind a clip, and the Python
surface built on it (ops.resample, transforms.Resample, the .wav readers, AugmentFP's resample_banks)."""
import numpy as np
import pytest
import torch

from musicfpaugment_amd import synth
from tests import _resample_oracle as ro

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
B = 3


@pytest.fixture(scope="module")
def ops():
    from musicfpaugment_amd import ops as _ops
    return _ops


def _tile(pair):
    from musicfpaugment_amd import ops as _ops
    return _ops.resample_tile(*pair)


def _cases():
    """(orig, new, L): lengths around one frame, shorter than the filter's half width, and over several workgroups."""
    out = [(44100, 8000, L) for L in (1, 33, 440, 441, 442, 4411)]
    out.append((44100, 8000, "3 tiles + 37"))
    out += [(16000, 8000, 2), (16000, 8000, 1001), (16000, 8000, "3 tiles + 1")]
    out += [(48000, 8000, 613), (22050, 8000, 2000), (11025, 8000, 443), (8000, 16000, 257), (44100, 48000, 1000), (48000, 44100, 1000)]
    return out


def _length(orig, new, L):
    if isinstance(L, str):
        o = ro.geometry(orig, new)[0]
        return 3 * _tile((orig, new)) * o + int(L.rsplit(" ", 1)[1])
    return L


def _clips(orig, new, L, b=B):
    return np.random.default_rng([orig, new, L]).standard_normal((b, L)).astype(np.float32)


@pytest.mark.parametrize("case", _cases(), ids=str)
def test_against_the_oracle(ops, case):
    """Every sample within (K + 2) * 2^-24 * conv(|taps|, |x|) of the float64 result with the same float32 taps: the any-order
    float32 summation bound (K products, K - 1 additions, one rounding each), derived and not measured."""
    orig, new, L = case
    L = _length(orig, new, L)
    K = ro.geometry(orig, new)[3]
    x = _clips(orig, new, L)
    want, bound = ro.resample(x, orig, new, with_bound=True)
    got = ops.resample(torch.from_numpy(x).cuda(), orig, new)
    assert got.shape == want.shape and got.dtype == torch.float32
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    ratio = err / ((K + 2) * EPS * bound + 1e-300)
    print(case, "L", L, "largest |error| / bound:", float(ratio.max()))
    assert np.all(err <= (K + 2) * EPS * bound)


def test_the_taps_on_the_device_are_the_oracles(ops):
    for pair in sorted(ro.TABLE):
        taps = ops.resample_taps(*pair, "cuda")
        want = ro.taps64(*pair)                                           # phase-major
        K = want.shape[1]
        assert taps.shape == (want.shape[0], ops.resample_tap_pitch(K)) and taps.data_ptr() % 64 == 0
        assert np.all(np.abs(taps[:, :K].cpu().numpy().astype(np.float64) - want) <= EPS * np.abs(want) + 1e-15)
        assert not bool(taps[:, K:].any())


PAIRS = [(44100, 8000), (16000, 8000), (8000, 16000), (48000, 44100)]


@pytest.mark.parametrize("pair", PAIRS, ids=str)
def test_a_clip_does_not_depend_on_its_batch(ops, pair):
    L = 2 * _tile(pair) * ro.geometry(*pair)[0] + 5
    x = torch.from_numpy(_clips(*pair, L)).cuda()
    y = ops.resample(x, *pair)
    for b in range(B):
        assert torch.equal(ops.resample(x[b:b + 1].clone(), *pair)[0], y[b])


@pytest.mark.parametrize("pair", PAIRS, ids=str)
def test_a_clip_does_not_depend_on_what_follows_it(ops, pair):
    """Zeros appended to a clip move its samples into other workgroups' tiles and change nothing of the first Tout(L) outputs."""
    L = _tile(pair) * ro.geometry(*pair)[0] + 3
    x = torch.from_numpy(_clips(*pair, L)).cuda()
    y = ops.resample(x, *pair)
    yp = ops.resample(torch.nn.functional.pad(x, (0, 977)), *pair)
    assert yp.shape[1] > y.shape[1] and torch.equal(yp[:, :y.shape[1]], y)


@pytest.mark.parametrize("pair", PAIRS, ids=str)
def test_a_padded_row_pitch_equals_the_packed_one(ops, pair):
    """The raw C call with ldx > T and ldy > Tout: the samples between the rows (NaN here) are neither read nor written."""
    from musicfpaugment_amd._lib import check, lib, ptr, stream
    L = _tile(pair) * ro.geometry(*pair)[0] + 3
    x = torch.from_numpy(_clips(*pair, L)).cuda()
    y = ops.resample(x, *pair)
    o, n, width, _, Tout = ops.resample_geometry(*pair, L)
    ldx, ldy = L + 13, Tout + 7
    xp = torch.full((B, ldx), float("nan"), device="cuda")
    xp[:, :L] = x
    yp = torch.full((B, ldy), float("nan"), device="cuda")
    check(lib().mfpa_resample(ptr(xp), B, L, ldx, o, n, width, ptr(ops.resample_taps(*pair, "cuda")), ptr(yp), Tout, ldy, stream()),
          "mfpa_resample")
    assert torch.equal(yp[:, :Tout], y) and bool(torch.isnan(yp[:, Tout:]).all())


def test_equal_rates_return_the_very_tensor(ops):
    from musicfpaugment_amd.transforms import Resample
    x = torch.zeros(2, 100, device="cuda")
    assert ops.resample(x, 8000, 8000) is x
    assert Resample(8000, 8000)(x) is x and Resample()(x) is x


def test_empty_batches_and_clips(ops):
    assert ops.resample(torch.zeros(0, 100, device="cuda"), 16000, 8000).shape == (0, 50)
    assert ops.resample(torch.zeros(2, 0, device="cuda"), 16000, 8000).shape == (2, 0)


def test_resample_transform_takes_any_leading_shape_and_device(ops):
    from musicfpaugment_amd.transforms import Resample
    x = torch.from_numpy(_clips(16000, 8000, 1001, 6)).reshape(2, 3, 1001)
    y = Resample(16000, 8000)(x)
    assert y.shape == (2, 3, 501) and y.device.type == "cpu" and y.dtype == torch.float32
    want = ops.resample(x.reshape(6, 1001).cuda(), 16000, 8000)
    assert torch.equal(y.reshape(6, 501), want.cpu())
    yd = Resample(16000, 8000).forward(x.cuda())
    assert yd.is_cuda and torch.equal(yd.cpu(), y)
    assert Resample(16000, 8000)(x[0, 0]).shape == (501,)
    with pytest.raises(ValueError):
        Resample(16000, 8000)(x.double())
    with pytest.raises(ValueError):
        Resample(44101, 8000)                                             # more phases than the kernel takes


@pytest.fixture(scope="module")
def wav_files(tmp_path_factory):
    """A 16 kHz int16 mono file and a 44.1 kHz float32 stereo file, 2 s each, with their decoded mono samples."""
    from scipy.io import wavfile
    d = tmp_path_factory.mktemp("resample_wavs")
    a = (synth.batch(1, seed=3100, n=32000)[0] * 32767).astype(np.int16)
    wavfile.write(d / "a16k.wav", 16000, a)
    s = np.stack([synth.batch(1, seed=3101, n=88200)[0], synth.batch(1, seed=3102, n=88200, tonal=False)[0]], axis=1).astype(np.float32) * 0.5
    wavfile.write(d / "s44k.wav", 44100, s)
    return {"a": (str(d / "a16k.wav"), 16000, a.astype(np.float32) / 32768.0), "s": (str(d / "s44k.wav"), 44100, s.mean(axis=1))}


def test_wav_files_at_other_rates_are_resampled_on_the_device(ops, wav_files):
    from musicfpaugment_amd.afp.audfprint.peak_extractor import Audfprint_peaks
    from musicfpaugment_amd.afp.dejavu import dejavu
    for path, sr, decoded in wav_files.values():
        got = Audfprint_peaks._read_waveform(path, 8000)
        want = ops.resample(torch.from_numpy(np.ascontiguousarray(decoded, dtype=np.float32))[None].cuda(), sr, 8000)[0]
        assert got.device.type == "cpu" and got.shape == (16000,) and torch.equal(got, want.cpu())
    path, sr, _ = wav_files["a"]
    wav = Audfprint_peaks._read_waveform(path, 8000)
    ext = Audfprint_peaks(None)
    h = ext.wavfile2hashes(path)
    uq, n = ext.hashes_batch(wav[None].cuda())
    assert len(h) > 0 and np.array_equal(h, uq[0, : int(n[0])].cpu().numpy())
    assert abs(ext.soundfiledur - 2.0) < 1e-9
    channels, rate, _ = dejavu.read(path)
    assert rate == 8000 and len(channels) == 1 and torch.equal(channels[0].cpu(), wav * 32767)
    with pytest.raises(NotImplementedError):
        Audfprint_peaks._read_waveform("x.mp3", 8000)                     # decoding stays outside


def test_augmentfp_resamples_its_banks_when_asked(ops, tmp_path):
    import random
    from scipy.io import wavfile
    from musicfpaugment_amd.augmentation import AugmentFP, synthetic_banks
    irs, noises = synthetic_banks(3, sample_rate=32000, n_ir=2, n_noise=2, noise_seconds=1.0)
    ir = (irs[1].numpy() / np.abs(irs[1].numpy()).max() * 32767).astype(np.int16)
    ir_dir = tmp_path / "irs"
    ir_dir.mkdir()
    wavfile.write(ir_dir / "ir.wav", 32000, ir)
    noise = noises["scene0"][0].numpy()[::2].astype(np.float32) * 0.1      # any 16 kHz signal
    wavfile.write(tmp_path / "n.wav", 16000, noise)
    paths = {"street": [str(tmp_path / "n.wav")]}
    with pytest.raises(NotImplementedError):
        AugmentFP(paths, 8000, impulse_response_dir=str(ir_dir))          # the default still refuses
    af = AugmentFP(paths, 8000, impulse_response_dir=str(ir_dir), resample_banks=True)
    want_ir = ops.resample(torch.from_numpy(ir.astype(np.float32) / 32768.0)[None].cuda(), 32000, 8000)[0].cpu()
    want_noise = ops.resample(torch.from_numpy(noise)[None].cuda(), 16000, 8000)[0].cpu()
    assert len(af.ir_bank) == 1 and torch.equal(af.ir_bank[0], want_ir)
    assert torch.equal(af.noise_bank["street"][0], want_noise)
    random.seed(5); torch.manual_seed(5)
    out = af.batch_augment(torch.from_numpy(synth.batch(4, seed=3200, n=16000))[:, None, :])
    assert out.shape == (4, 1, 16000) and bool(torch.isfinite(out).all())
