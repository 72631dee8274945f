"""GPU: the complex STFT (mfpa_stft_complex), the inverse STFT (mfpa_istft) and UNet.denoise_waveform against torch.stft / torch.istft
on the CPU and the numpy restatement of tests/_istft_oracle.py.

Error unit (tests/_istft_oracle.py): E(x) = max |torch.istft(torch.stft(x.double())) - x| on the CPU, bounds 8 E.  Every
comparison prints its ratio to E before it asserts (pytest -s shows them; NOTES.md keeps the measured ones).

T_w = 8548 is 33 hops + 100 samples: it crosses the edge of the 15-hop workgroups twice and ends in a partial hop that lies under
one frame only; 257 and 511 are the shortest and the longest clip of 2 frames, 512 the shortest of 3, 769 is 3 hops + 1 sample;
64000 is the pipeline's clip."""
import functools

import numpy as np
import pytest
import torch

from tests import _istft_oracle as io
from tests._istft_oracle import error_unit, torch_istft, torch_stft

pytestmark = pytest.mark.gpu

SIZES = (257, 511, 512, 769, 8548, 64000)
CASES = [(T, B) for T in SIZES for B in (1, 3)]


@pytest.fixture(scope="module")
def ops():
    from musicfpaugment_amd import ops as _ops
    return _ops


@functools.lru_cache(maxsize=None)
def _case(T, B):
    """x (B, T) uniform in [-1, 1] on the CPU, its error unit E, torch's spectrum, and the device's (computed once, never modified)."""
    from musicfpaugment_amd import ops as _ops
    x = torch.rand(B, T, generator=torch.Generator().manual_seed(1000 * B + T)) * 2 - 1
    spec = _ops.stft_complex(x.cuda())
    return x, error_unit(x), torch_stft(x), spec


def _ratio(what, got, want, E):
    r = float((torch.as_tensor(got).double().cpu() - torch.as_tensor(want).double().cpu()).abs().max()) / E
    print(f"{what}: {r:.3f} E (E = {E:.3e})")
    return r


@pytest.mark.parametrize("T,B", CASES)
def test_stft_complex_against_torch_and_its_magnitudes_against_stft_mag(ops, T, B):
    x, E, Zt, spec = _case(T, B)
    assert spec.dtype == torch.complex128 and spec.shape == (B, 257, 1 + T // 256)
    # a bin is a sum of 512 windowed samples: the window's sum (256) scales the unit
    assert _ratio(f"stft_complex T={T} B={B}", torch.view_as_real(spec), torch.view_as_real(Zt), 256 * E) <= 8
    xd = x.cuda()
    for dt in (torch.float32, torch.float64):
        s2, mag, cmax = ops.stft_complex(xd, want_mag=True, mag_dtype=dt)
        want_mag, want_max = ops.stft_mag(xd, dt)
        assert mag.dtype == dt and torch.equal(mag, want_mag) and torch.equal(cmax, want_max)
        assert torch.equal(torch.view_as_real(s2), torch.view_as_real(spec))


@pytest.mark.parametrize("T,B", CASES)
def test_round_trip_and_float32_output(ops, T, B):
    x, E, _, spec = _case(T, B)
    y64 = ops.istft(spec, T, out_dtype=torch.float64)
    assert y64.dtype == torch.float64 and y64.shape == (B, T)
    assert _ratio(f"round trip T={T} B={B}", y64, x, E) <= 8
    y32 = ops.istft(spec, T)
    assert y32.dtype == torch.float32 and torch.equal(y32, y64.float())           # the float64 value rounded once
    if T % 256 == 0:
        assert torch.equal(ops.istft(spec, out_dtype=torch.float64), y64)           # length=None: 256 (n_frames - 1), as in torch


@pytest.mark.parametrize("T,B", CASES)
def test_device_spectrum_through_torch_istft_with_imaginary_dc_and_nyquist(ops, T, B):
    x, E, _, spec = _case(T, B)
    s = spec.clone()
    s[:, 0] += 3.0j
    s[:, 256] -= 2.0j
    want = torch_istft(s.cpu(), T)
    assert _ratio(f"device spectrum vs torch.istft T={T} B={B}", ops.istft(s, T, out_dtype=torch.float64), want, E) <= 8
    assert _ratio(f"... and the input T={T} B={B}", want, x, E) <= 8                # torch ignored those imaginary parts too


@pytest.mark.parametrize("T,B", CASES)
def test_magnitude_path(ops, T, B):
    x, E, _, spec = _case(T, B)
    S = spec.cpu().numpy()
    g = np.random.default_rng(T + B)
    gain = g.uniform(0.25, 1.0, size=S.shape)
    d = g.uniform(0.5, 4.0, size=B)
    dd = torch.from_numpy(d).cuda()
    for dt in (np.float32, np.float64):
        for denom, ddev in ((None, None), (d, dd)):
            # m = gain * |spec| both times: with a denominator the magnitudes come divided by it
            mag = (gain * np.abs(S) / (1.0 if denom is None else d[:, None, None])).astype(dt)
            want = torch_istft(torch.from_numpy(io.apply_magnitude(S, mag, denom)), T)
            got = ops.istft(spec, T, mag=torch.from_numpy(mag).cuda(), denom=ddev, out_dtype=torch.float64)
            assert _ratio(f"magnitudes {np.dtype(dt).name} denom={denom is not None} T={T} B={B}", got, want, E) <= 8
    # |spec| / d with denom = d gives the input back
    back = ops.istft(spec, T, mag=torch.from_numpy(np.abs(S) / d[:, None, None]).cuda(), denom=dd, out_dtype=torch.float64)
    assert _ratio(f"|spec| / d * d T={T} B={B}", back, x, E) <= 8
    # a zeroed bin takes phase 0
    s0 = spec.clone()
    s0[:, 40, 1] = 0
    m2 = torch.full(S.shape, 2.0, dtype=torch.float64).cuda()
    want = torch_istft(torch.from_numpy(io.apply_magnitude(s0.cpu().numpy(), m2.cpu().numpy())), T)
    assert _ratio(f"zeroed bin T={T} B={B}", ops.istft(s0, T, mag=m2, out_dtype=torch.float64), want, E) <= 8
    # negative magnitudes: flipped without the clamp, zero with it
    signed = (gain * np.abs(S) * np.where(g.uniform(size=S.shape) < 0.3, -1.0, 1.0)).astype(np.float32)
    sd = torch.from_numpy(signed).cuda()
    for clamp in (False, True):
        want = io.istft(S, T, mag=signed, clamp=clamp)
        assert _ratio(f"negative magnitudes clamp={clamp} T={T} B={B}", ops.istft(spec, T, mag=sd, clamp=clamp, out_dtype=torch.float64),
                      want, E) <= 8
    assert not torch.equal(ops.istft(spec, T, mag=sd, clamp=True), ops.istft(spec, T, mag=sd))


@pytest.mark.parametrize("T", SIZES)
def test_a_row_does_not_depend_on_the_batch_its_position_or_its_surroundings(ops, T):
    _, _, _, spec = _case(T, 3)
    nF = spec.shape[2]
    mag = torch.rand(3, 257, nF, device="cuda") + 0.1
    den = torch.tensor([2.0, 0.5, 3.0], dtype=torch.float64, device="cuda")
    for kw in (dict(), dict(mag=mag, denom=den)):
        def run(s, rows):
            k = {n: v[rows].contiguous() for n, v in kw.items()}
            return ops.istft(s, T, out_dtype=torch.float64, **k)
        full = run(spec, slice(0, 3))
        for b in range(3):
            alone = run(spec[b:b + 1].contiguous(), slice(b, b + 1))
            assert torch.equal(alone[0], full[b]), b
        order = [2, 1, 0]                                                             # clip 1 stays the middle row, clips 0 and 2 trade places
        assert torch.equal(run(spec[order].contiguous(), order), full[order])
        mid = [0, 2, 1]
        assert torch.equal(run(spec[mid].contiguous(), mid)[1], full[2])              # clip 2 as a middle row
        big = torch.full((5, 257, nF), float("nan"), dtype=torch.complex128, device="cuda")
        big[2] = spec[1]
        assert torch.equal(run(big[2:3], slice(1, 2))[0], full[1])                    # a slice of a larger buffer, NaN around it


def test_python_refusals(ops):
    from musicfpaugment_amd._lib import MfpaError
    _, _, _, spec = _case(769, 3)                                                     # 4 frames: lengths 768 .. 1023
    for length in (767, 1024, 0, -5):
        with pytest.raises(ValueError):
            ops.istft(spec, length)
    assert ops.istft(spec, 1023).shape == (3, 1023) and ops.istft(spec).shape == (3, 768)
    with pytest.raises(ValueError):
        ops.istft(spec.to(torch.complex64), 769)
    with pytest.raises(ValueError):
        ops.istft(torch.view_as_real(spec), 769)
    with pytest.raises(ValueError):
        ops.istft(spec[:, :256], 769)
    with pytest.raises(ValueError):
        ops.istft(spec[:, :, :1], 100)
    with pytest.raises(ValueError):
        ops.istft(spec, 769, out_dtype=torch.float16)
    with pytest.raises(ValueError):
        ops.istft(spec, 769, mag=torch.ones(3, 257, 4, dtype=torch.float16, device="cuda"))
    with pytest.raises(ValueError):
        ops.istft(spec, 769, mag=torch.ones(3, 257, 3, device="cuda"))
    with pytest.raises(ValueError):
        ops.istft(spec, 769, mag=torch.ones(3, 257, 4, device="cuda"), denom=torch.ones(3, device="cuda"))      # float32 denominator
    with pytest.raises(ValueError):
        ops.istft(spec, 769, denom=torch.ones(3, dtype=torch.float64, device="cuda"))                          # denom without mag
    with pytest.raises(MfpaError):
        ops.istft(spec.cpu(), 769)
    with pytest.raises(MfpaError):
        ops.istft(spec, 769, mag=torch.ones(3, 257, 4))
    with pytest.raises(MfpaError):
        ops.stft_complex(torch.zeros(2, 1000))
    with pytest.raises(ValueError):
        ops.stft_complex(torch.zeros(2, 256, device="cuda"))
    with pytest.raises(ValueError):
        ops.stft_complex(torch.zeros(2, 1000, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        ops.stft_complex(torch.zeros(2, 1000, device="cuda"), want_mag=True, mag_dtype=torch.float16)
    zero = ops.stft_tables(np.zeros(512), "cuda")
    with pytest.raises(RuntimeError, match="window overlap add min"):
        ops.istft(spec, 769, tables=zero)
    assert ops.istft(spec[:0], 769).shape == (0, 769)                                 # an empty batch is a no-op


@pytest.fixture(scope="module")
def net():
    from musicfpaugment_amd.training.unet import UNet
    from musicfpaugment_amd.training.weights import formula_state_dict
    m = UNet(1, 1, rate=0.05)
    m.load_state_dict(formula_state_dict(0))
    return m.cuda().eval()


@pytest.mark.parametrize("per_clip", (False, True))
def test_unet_denoise_waveform(ops, net, per_clip):
    """denoise_waveform is the chain stft_complex -> denoise_spectrogram -> istft, bit for bit.  Its float32 samples cannot lie within
    8 E of anything (one float32 rounding is 2^-25 of a sample, E some 2^-51): the float64 output of the same chain is held to
    8 E s of torch.istft built on the CPU from the device's own network output, s = max |y_ref| / max |x|, and the float32 output to
    that float64 output rounded once."""
    x, E, _, _ = _case(24000, 2)
    xd = x.cuda()
    y = net.denoise_waveform(xd, per_clip=per_clip)
    assert y.dtype == torch.float32 and y.shape == (2, 24000)
    spec, mag, cmax = ops.stft_complex(xd, want_mag=True)
    den = net.denoise_spectrogram(mag, cmax, per_clip)
    denom = cmax if per_clip else cmax.max().expand(2).contiguous()
    assert torch.equal(y, ops.istft(spec, 24000, mag=den, denom=denom, clamp=True))
    y64 = ops.istft(spec, 24000, mag=den, denom=denom, clamp=True, out_dtype=torch.float64)
    assert torch.equal(y, y64.float())
    Z = io.apply_magnitude(spec.cpu().numpy(), den.cpu().numpy(), denom.cpu().numpy(), clamp=True)
    y_ref = torch_istft(torch.from_numpy(Z), 24000)
    s = float(y_ref.abs().max()) / float(x.abs().max())
    assert _ratio(f"denoise_waveform per_clip={per_clip} (s = {s:.3e})", y64, y_ref, E * s) <= 8


def test_unet_denoise_waveform_is_eval_only(net):
    from musicfpaugment_amd._lib import MfpaError
    net.train()
    try:
        with pytest.raises(MfpaError):
            net.denoise_waveform(torch.zeros(2, 24000, device="cuda"))
    finally:
        net.eval()
