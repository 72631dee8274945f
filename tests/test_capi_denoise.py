"""CPU: the spectral suppressor's entry point (mfpa_spectral_suppress) through ctypes.  It checks its arguments before any launch and
dereferences no device pointer on the host, so all of this runs without a GPU (the style of tests/test_capi_codec.py).  The Python
refusals of ops.spectral_suppress, functional.spectral_denoise, SpectralDenoiser and NoiseSuppression need none either."""
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 1 << 12          # a non-null, 16-byte aligned value for pointers that are never dereferenced


@pytest.fixture(scope="module")
def lib():
    from musicfpaugment_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from musicfpaugment_amd.csrc.build import build
        build(verbose=False)
    return _lib


def _suppress(h, **kw):
    a = dict(m=P, m_f64=0, B=2, F=257, nF=100, alpha=0.7, back=48, ahead=48, bias=3.0, a=0.9, xi_min=10.0 ** -2.5, g_floor=0.1, floors=None,
             noise=None, denom=None, apply=None, y=P, y_f64=0, g=None, n=None, stream=None)
    a.update(kw)
    return h.mfpa_spectral_suppress(a["m"], a["m_f64"], a["B"], a["F"], a["nF"], a["alpha"], a["back"], a["ahead"], a["bias"], a["a"], a["xi_min"],
                                    a["g_floor"], a["floors"], a["noise"], a["denom"], a["apply"], a["y"], a["y_f64"], a["g"], a["n"], a["stream"])


def test_symbol_header_constant_and_abi_version(lib):
    from musicfpaugment_amd import ops
    h = lib.lib()
    header = open(os.path.join(ROOT, "include", "mfpa.h")).read()
    declared = set(re.findall(r"^int\s+(mfpa_\w+)\s*\(", header, flags=re.M))
    name = "mfpa_spectral_suppress"
    assert name in lib.exported_symbols() and name in declared and hasattr(h, name)
    assert len(lib._SIGNATURES[name][0]) == 21
    assert int(re.search(r"#define MFPA_DENOISE_MAX_WINDOW (\d+)", header).group(1)) == ops.DENOISE_MAX_WINDOW >= 128
    assert lib.ABI_VERSION == 47 and h.mfpa_version() == 47              # the new symbol is additive
    from musicfpaugment_amd.csrc import build as b
    assert b.PER_FILE["denoise.hip"] == ["-ffp-contract=off"]


nan, inf = math.nan, math.inf
ERRORS = [dict(alpha=-0.1), dict(alpha=1.0), dict(alpha=1.5), dict(alpha=nan), dict(a=-0.1), dict(a=1.0), dict(a=nan), dict(xi_min=0.0),
          dict(xi_min=-1.0), dict(xi_min=inf), dict(xi_min=nan), dict(g_floor=-0.1), dict(g_floor=1.1), dict(g_floor=nan), dict(bias=0.0),
          dict(bias=-3.0), dict(bias=nan), dict(bias=inf), dict(back=-1), dict(ahead=-1), dict(back=64, ahead=64), dict(back=128, ahead=0),
          dict(back=0, ahead=128), dict(back=2 ** 31 - 1, ahead=2 ** 31 - 1), dict(B=0), dict(B=-1), dict(B=65536), dict(F=0), dict(F=-3),
          dict(nF=0), dict(nF=-1), dict(nF=16385), dict(m_f64=2), dict(y_f64=-1), dict(m=None), dict(y=None), dict(m=P + 2), dict(y=P + 2),
          dict(m=P + 4, m_f64=1), dict(y=P + 4, y_f64=1), dict(noise=P + 4), dict(denom=P + 4), dict(floors=P + 4), dict(g=P + 4), dict(n=P + 4)]


@pytest.mark.parametrize("change", ERRORS, ids=[str(i) + "-" + ",".join(c) for i, c in enumerate(ERRORS)])
def test_argument_errors_do_not_touch_the_gpu(lib, change):
    assert _suppress(lib.lib(), **change) == lib.EINVAL


def test_python_refusals_need_no_gpu():
    from musicfpaugment_amd import functional as F
    from musicfpaugment_amd import ops
    from musicfpaugment_amd.augmentation.transformations.noise_suppression import NoiseSuppression
    from musicfpaugment_amd.denoisers import SpectralDenoiser
    m = torch.zeros(2, 5, 20, dtype=torch.float64)
    for bad in (torch.zeros(5, 20), torch.zeros(2, 5, 20, dtype=torch.float16), np.zeros((2, 5, 20)), torch.zeros(2, 0, 20), torch.zeros(2, 5, 0),
                torch.zeros(0, 5, 20), torch.zeros(1, 1, 16385)):
        with pytest.raises(ValueError):
            ops.spectral_suppress(bad)
    for kw in (dict(alpha=1.0), dict(alpha=-0.5), dict(alpha=nan), dict(dd=1.0), dict(dd=-1e-3), dict(dd="x"), dict(bias=0.0), dict(bias=-1.0),
               dict(bias=inf), dict(back=-1), dict(ahead=-2), dict(back=1.5), dict(back=64, ahead=64), dict(xi_min_db=nan), dict(xi_min_db=inf),
               dict(floor_db=1.0), dict(floor_db=nan), dict(floor_db=[-10.0]), dict(floor_db=[-10.0, 3.0]), dict(floor_db=[-10.0, nan]),
               dict(noise_psd=torch.zeros(2, 5)), dict(noise_psd=torch.zeros(2, 4, dtype=torch.float64)), dict(denom=torch.zeros(2)),
               dict(denom=torch.zeros(3, dtype=torch.float64)), dict(apply=[True]), dict(out_dtype=torch.float16)):
        with pytest.raises(ValueError):
            ops.spectral_suppress(m, **kw)
    xi_min, g_floor = ops.suppress_thresholds()
    assert xi_min == 10.0 ** -2.5 and g_floor == 10.0 ** -1.0 and ops.suppress_thresholds(-10.0, -6.0) == (10.0 ** -1.0, 10.0 ** (-6.0 / 20.0))
    for bad in (dict(domain="log"), dict(gamma=1.0), dict(floor_db=2.0), dict(xi_min_db=nan)):
        with pytest.raises(ValueError):
            SpectralDenoiser(**bad)
    for bad in (dict(min_floor_db=-5.0, max_floor_db=-10.0), dict(max_floor_db=1.0), dict(min_floor_db=-inf)):
        with pytest.raises(ValueError):
            NoiseSuppression(**bad)
    x = torch.zeros(2, 1000)
    for call in (lambda: F.spectral_denoise(x, 0), lambda: F.spectral_denoise(x.double(), 8000), lambda: F.spectral_denoise(x, 8000, gamma=2.0),
                 lambda: F.spectral_denoise(np.zeros(1000, dtype=np.float32), 8000)):
        with pytest.raises(ValueError):
            call()


def test_no_cpu_fallback():
    from musicfpaugment_amd import functional as F
    from musicfpaugment_amd import ops
    from musicfpaugment_amd._lib import MfpaError
    from musicfpaugment_amd.augmentation.transformations.noise_suppression import NoiseSuppression
    from musicfpaugment_amd.denoisers import SpectralDenoiser
    m = torch.zeros(2, 5, 20)
    with pytest.raises(MfpaError):
        ops.spectral_suppress(m, floor_db=[-10.0, -20.0], apply=[True, False], return_gain=True, return_noise=True)
    net = SpectralDenoiser().to("cpu").eval()                            # no parameters: .to() and .eval() work
    assert list(net.parameters()) == [] and not net.training
    with pytest.raises(MfpaError):
        net.denoise_spectrogram(m.double(), torch.ones(2, dtype=torch.float64), True)
    with pytest.raises(MfpaError):
        net(torch.zeros(2, 1, 1000))
    with pytest.raises(MfpaError):
        NoiseSuppression(p=1.0)(torch.zeros(2, 1, 1000))
    if not torch.cuda.is_available():
        with pytest.raises(MfpaError):
            F.spectral_denoise(torch.zeros(3, 1, 1000), 8000)


def test_transform_constructs_names_its_parameters_and_composes():
    from musicfpaugment_amd.augmentation.composition import Compose, OneOf, SomeOf
    from musicfpaugment_amd.augmentation.transformations.noise_suppression import NoiseSuppression
    t = NoiseSuppression()
    assert (t.min_floor_db, t.max_floor_db, t.p) == (-30.0, -10.0, 0.5)
    torch.manual_seed(5)
    t.transform_parameters = {"should_apply": torch.tensor([True, False, True, True, False, True])}
    t.randomize_parameters(torch.zeros(6, 2000), 8000)                   # the draw is host work
    assert sorted(k for k in t.transform_parameters if k != "should_apply") == ["floor_db"] and len(t.transform_parameters["floor_db"]) == 4
    f = t.floors()
    assert f.shape == (6,) and f.dtype == np.float64 and np.all(f >= -30.0 - 1e-5) and np.all(f <= -10.0 + 1e-5) and len(set(f.tolist())) == 6
    chain = Compose([NoiseSuppression(p=1.0), SomeOf((1, 2), [NoiseSuppression(p=1.0), NoiseSuppression()]), OneOf([NoiseSuppression(), NoiseSuppression()])])
    assert len(chain.transforms) == 3
