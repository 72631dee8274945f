"""GPU: every form of `apply` gives the same bits in every wrapper that takes one.  The mask goes to the device through one
function (ops/_args.py); this is the test that crosses all of its callers: a list, a host bool tensor, a device bool tensor and
a device uint8 tensor with values other than 0 and 1 select the same rows, a row that is not selected comes back bit for bit
(the denoiser: with gain exactly 1), and no mask equals a mask of ones.

T = 700 spans more than one 256-sample block of the codec and more than one tile of the variable delay.  At T = 700 no sample rate
the K-weighting takes leaves loudness_normalize a 400 ms block, so there it returns every row unchanged and the comparison says
little; the same wrapper is therefore also run at T = 2000 and 4 kHz, where the gain acts."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
B, T = 3, 700
MASK = [True, False, True]


def _wave(t=T):
    g = torch.Generator().manual_seed(20240 + t)
    return (0.3 * torch.randn(B, t, generator=g, dtype=torch.float64)).to(DEV)


def _mags():
    g = torch.Generator().manual_seed(77)
    return torch.rand(B, 5, 40, generator=g, dtype=torch.float64).add_(0.05).to(DEV)


def _lfo():
    n = torch.arange(T, dtype=torch.float64)
    return (5.5 + 3.0 * torch.sin(2.0 * np.pi * n / 97.0)).expand(B, T).contiguous().to(DEV)


def _cases():
    from musicfpaugment_amd import ops
    sos = [[0.2, 0.3, 0.1, 1.0, -0.5, 0.2]]
    comp = [-30.0, 0.75, 6.0, 0.9, 0.99, 3.0]
    # name -> (input, call(x, apply) -> (y, gain or None), whether a selected row must differ from the input)
    return {
        "sosfilt": (_wave(), lambda x, a: (ops.sosfilt(x, sos, apply=a), None), True),
        "compressor": (_wave(), lambda x, a: (ops.compressor(x, comp, apply=a), None), True),
        "variable_delay": (_wave(), lambda x, a: (ops.variable_delay(x, _lfo(), 0.7, dry=0.2, apply=a), None), True),
        "comb": (_wave(), lambda x, a: (ops.comb(x, 7, 1.0, 0.0, 0.5, apply=a), None), True),
        "transform_codec": (_wave(), lambda x, a: (ops.transform_codec(x, 16.0, apply=a), None), True),
        "mu_law": (_wave(), lambda x, a: (ops.mu_law(x, apply=a), None), True),
        "loudness_normalize": (_wave(), lambda x, a: (ops.loudness_normalize(x, 8000, -23.0, apply=a), None), False),
        "loudness_normalize_gated": (_wave(2000), lambda x, a: (ops.loudness_normalize(x, 4000, -23.0, apply=a), None), True),
        "spectral_suppress": (_mags(), lambda x, a: ops.spectral_suppress(x, back=4, ahead=4, apply=a, return_gain=True), True),
    }


NAMES = ("sosfilt", "compressor", "variable_delay", "comb", "transform_codec", "mu_law", "loudness_normalize", "loudness_normalize_gated",
         "spectral_suppress")


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.dtype == b.dtype == torch.float64 and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64),
                                                                                       b.contiguous().view(torch.int64))


@pytest.mark.parametrize("name", NAMES)
def test_every_form_of_apply_gives_the_same_bits(name):
    x, call, acts = _cases()[name]
    x0 = x.clone()
    y, g = call(x, MASK)
    forms = {"host bool tensor": torch.tensor(MASK), "device bool tensor": torch.tensor(MASK, device=DEV),
             "device uint8 tensor": torch.tensor([2, 0, 255], dtype=torch.uint8, device=DEV)}
    for form, a in forms.items():
        y2, g2 = call(x, a)
        assert _same_bits(y, y2), (name, form)
        assert g is None or _same_bits(g, g2), (name, form)
    assert _same_bits(x, x0), name                                           # the input is not written
    if g is None:
        assert _same_bits(y[1], x[1]), name                                  # the row that is not selected: bit for bit
    else:
        assert bool((g[1] == 1.0).all()), name                               # the denoiser: gain exactly 1
    if acts:
        assert not torch.equal(y[0], x[0]) and not torch.equal(y[2], x[2]), name
    y_none, g_none = call(x, None)
    y_ones, g_ones = call(x, [True] * B)
    assert _same_bits(y_none, y_ones), name
    assert g_none is None or _same_bits(g_none, g_ones), name
    if acts:
        assert not torch.equal(y_none[1], x[1]), name
