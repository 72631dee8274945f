"""CPU: the compressor's entry point (mfpa_dynamics) through ctypes.  It checks its arguments before any launch and never
dereferences a pointer on the host, so all of this runs without a GPU (the style of tests/test_capi_iir.py).  The Python refusals
of ops.compressor / envelope_follow / time_coef, functional.compressor / limiter and the Compressor / Limiter transforms need none
either."""
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


def _dynamics(h, **kw):
    a = dict(x=P, x_f64=0, B=2, T=100, params=P, params_per_row=0, apply=None, zi=None, zf=None, level_in=0, y=P, gr=None, stream=None)
    a.update(kw)
    return h.mfpa_dynamics(a["x"], a["x_f64"], a["B"], a["T"], a["params"], a["params_per_row"], a["apply"], a["zi"], a["zf"], a["level_in"],
                           a["y"], a["gr"], a["stream"])


def test_symbol_header_and_abi_version(lib):
    h = lib.lib()
    header = open(os.path.join(ROOT, "include", "mfpa.h")).read()
    declared = set(re.findall(r"^int\s+(mfpa_\w+)\s*\(", header, flags=re.M))
    assert "mfpa_dynamics" in lib.exported_symbols() and "mfpa_dynamics" in declared and hasattr(h, "mfpa_dynamics")
    assert "mfpa_dynamics" in lib._SIGNATURES and len(lib._SIGNATURES["mfpa_dynamics"][0]) == 13
    assert lib.ABI_VERSION == 47 and h.mfpa_version() == 47              # the new symbol is additive


@pytest.mark.parametrize("change", [dict(x=None), dict(y=None), dict(params=None), dict(x=P + 2), dict(y=P + 2), dict(gr=P + 2),
                                    dict(x=P + 4, x_f64=1), dict(y=P + 4, x_f64=1), dict(gr=P + 4, x_f64=1), dict(params=P + 4),
                                    dict(zi=P + 4), dict(zf=P + 4), dict(T=0), dict(T=-5), dict(T=(1 << 30) + 1), dict(B=-1),
                                    dict(B=65536), dict(x_f64=2), dict(x_f64=-1), dict(params_per_row=2), dict(params_per_row=-1),
                                    dict(level_in=2), dict(level_in=-1), dict(level_in=1, gr=P)], ids=str)
def test_dynamics_rejects_before_any_launch(lib, change):
    assert _dynamics(lib.lib(), **change) == lib.EINVAL


def test_empty_batch_is_a_no_op_but_a_bad_shape_is_still_an_error(lib):
    h = lib.lib()
    assert _dynamics(h, B=0) == 0 and _dynamics(h, B=0, x=None, y=None, params=None) == 0
    assert _dynamics(h, B=0, T=1 << 30, params_per_row=1, x_f64=1, level_in=1) == 0
    for bad in (dict(T=0), dict(T=(1 << 30) + 1), dict(x_f64=2), dict(params_per_row=2), dict(level_in=3), dict(level_in=1, gr=P)):
        assert _dynamics(h, B=0, **bad) == lib.EINVAL, bad


def test_python_refusals_need_no_gpu():
    from musicfpaugment_amd import functional as F
    from musicfpaugment_amd import ops
    from musicfpaugment_amd.augmentation.transformations.dynamics import Compressor, Limiter
    x = torch.zeros(2, 100)
    ok = [-20.0, 0.75, 6.0, 0.9, 0.99, 0.0]
    nan, inf = float("nan"), float("inf")
    for bad in ([-20.0, 1.5, 6.0, 0.9, 0.99, 0.0], [-20.0, -0.1, 6.0, 0.9, 0.99, 0.0], [-20.0, 0.75, -1.0, 0.9, 0.99, 0.0],
                [-20.0, 0.75, 6.0, 1.0, 0.99, 0.0], [-20.0, 0.75, 6.0, 0.9, 1.0, 0.0], [-20.0, 0.75, 6.0, -0.1, 0.99, 0.0],
                [-20.0, 0.75, 6.0, 0.9, -0.1, 0.0], [nan, 0.75, 6.0, 0.9, 0.99, 0.0], [-20.0, 0.75, 6.0, 0.9, nan, 0.0],
                [-20.0, 0.75, 6.0, 0.9, 0.99, inf], ok[:5], [ok] * 3, [[ok]], np.zeros((0, 6))):
        with pytest.raises(ValueError):
            ops.compressor(x, bad)
    for wav in (torch.zeros(100), torch.zeros(1, 2, 100), x.to(torch.float16), x.to(torch.int32)):
        with pytest.raises(ValueError):
            ops.compressor(wav, ok)
        with pytest.raises(ValueError):
            ops.envelope_follow(wav, 0.9, 0.99)
    with pytest.raises(ValueError):
        ops.compressor(x, ok, apply=torch.ones(3, dtype=torch.bool))
    with pytest.raises(ValueError):
        ops.compressor(x, ok, zi=torch.zeros(2, 3, dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.envelope_follow(x, 0.9, 0.99, zi=torch.zeros(3, 2, dtype=torch.float64))
    for a, r in ((1.0, 0.5), (0.5, 1.0), (-0.1, 0.5), (0.5, nan), ([0.5, 0.5, 0.5], 0.5), (0.5, [[0.5, 0.5]])):
        with pytest.raises(ValueError):
            ops.envelope_follow(x, a, r)
    for seconds, rate in ((-1.0, 8000), (nan, 8000), (inf, 8000), (0.1, 0), (0.1, -8000), (0.1, nan)):
        with pytest.raises(ValueError):
            ops.time_coef(seconds, rate)
    for bad in (dict(ratio=0.5), dict(ratio=nan), dict(knee_db=-1.0), dict(attack_ms=-1.0), dict(release_ms=-1.0), dict(threshold_db=nan),
                dict(makeup_db=inf), dict(threshold_db=[-20.0, -10.0, -5.0]), dict(threshold_db=[-20.0, -10.0], ratio=[2.0, 3.0, 4.0])):
        with pytest.raises(ValueError):
            F.compressor(x, 8000, **bad)
    with pytest.raises(ValueError):
        F.compressor(x, 0)
    with pytest.raises(ValueError):
        F.compressor(x.to(torch.float16), 8000)
    for bad in (dict(threshold_db=nan), dict(release_ms=-1.0), dict(threshold_db=[-1.0, -2.0, -3.0])):
        with pytest.raises(ValueError):
            F.limiter(x, 8000, **bad)
    assert F.compressor_params(8000, ratio=inf)[1] == 1.0 and F.compressor_params(8000, ratio=1.0)[1] == 0.0
    Compressor()
    Limiter()
    for bad in (dict(min_threshold_db=-5.0, max_threshold_db=-10.0), dict(min_ratio=0.5), dict(min_ratio=5.0, max_ratio=2.0),
                dict(min_attack_ms=-1.0), dict(min_attack_ms=30.0), dict(min_release_ms=-1.0), dict(min_release_ms=500.0), dict(knee_db=-1.0)):
        with pytest.raises(ValueError):
            Compressor(**bad)
    for bad in (dict(min_threshold_db=0.0, max_threshold_db=-10.0), dict(min_release_ms=-1.0), dict(min_release_ms=500.0)):
        with pytest.raises(ValueError):
            Limiter(**bad)


def test_no_cpu_fallback():
    from musicfpaugment_amd import functional as F
    from musicfpaugment_amd import ops
    from musicfpaugment_amd._lib import MfpaError
    from musicfpaugment_amd.augmentation.transformations.dynamics import Compressor, Limiter
    ok = [-20.0, 0.75, 6.0, 0.9, 0.99, 0.0]
    with pytest.raises(MfpaError):
        ops.compressor(torch.zeros(2, 100), ok)
    with pytest.raises(MfpaError):
        ops.compressor(torch.zeros(2, 100, dtype=torch.float64), [ok, ok], apply=[True, False], zi=torch.zeros(2, 2, dtype=torch.float64),
                       return_gain_reduction=True, return_state=True)
    with pytest.raises(MfpaError):
        ops.envelope_follow(torch.zeros(2, 100), 0.9, [0.99, 0.5], return_state=True)
    for t in (Compressor(p=1.0, sample_rate=8000), Limiter(p=1.0, sample_rate=8000)):
        with pytest.raises(MfpaError):
            t(torch.zeros(2, 1, 8000))
    if not torch.cuda.is_available():
        x = torch.zeros(3, 100)
        for call in (lambda: F.compressor(x, 8000), lambda: F.compressor(x, 8000, ratio=[2.0, 4.0, float("inf")]),
                     lambda: F.limiter(x, 8000), lambda: F.limiter(x.reshape(3, 1, 100), 8000, threshold_db=[-1.0, -2.0, -3.0])):
            with pytest.raises(MfpaError):
                call()
