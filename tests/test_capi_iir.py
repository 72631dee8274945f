"""CPU: the recursive-filter entry points (mfpa_sosfilt, mfpa_sosfilt_work) through ctypes.  mfpa_sosfilt_work is a host function;
mfpa_sosfilt checks its arguments before any launch and never dereferences a pointer on the host, so all of this runs without a GPU
(the style of tests/test_capi_vocoder.py).  The Python refusals of ops.sosfilt, functional and the equaliser transforms need none
either."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mfpa_sosfilt", "mfpa_sosfilt_work")
P = 1 << 12          # a non-null, 16-byte aligned value for pointers that are never dereferenced
BIG = 1 << 40        # a work_len that is never too short


@pytest.fixture(scope="module")
def lib():
    from musicfpaugment_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from musicfpaugment_amd.csrc.build import build
        build(verbose=False)
    return _lib


def _sosfilt(h, **kw):
    a = dict(x=P, x_f64=0, B=2, T=100, sos=P, S=1, sos_per_row=0, apply=None, zi=None, zf=None, clamp=0, work=P, work_len=BIG, y=P,
             stream=None)
    a.update(kw)
    return h.mfpa_sosfilt(a["x"], a["x_f64"], a["B"], a["T"], a["sos"], a["S"], a["sos_per_row"], a["apply"], a["zi"], a["zf"], a["clamp"],
                          a["work"], a["work_len"], a["y"], a["stream"])


def _work(h, B, S, per_row):
    out = ctypes.c_longlong(-7)
    return h.mfpa_sosfilt_work(B, S, per_row, ctypes.addressof(out)), out.value


def test_symbols_header_and_abi_version(lib):
    h = lib.lib()
    header = open(os.path.join(ROOT, "include", "mfpa.h")).read()
    declared = set(re.findall(r"^int\s+(mfpa_\w+)\s*\(", header, flags=re.M))
    for name in NEW:
        assert name in lib.exported_symbols() and name in declared and hasattr(h, name), name
    assert lib.ABI_VERSION == 47 and h.mfpa_version() == 47              # the new symbols are additive
    from musicfpaugment_amd import ops
    assert int(re.search(r"#define MFPA_SOS_MAX_SECTIONS (\d+)", header).group(1)) == ops.SOS_MAX_SECTIONS == 8


def test_work_length(lib):
    """64 powers of a 2x2 matrix per filter and section; one filter with shared coefficients, none for an empty batch."""
    h = lib.lib()
    for B in (0, 1, 5, 65535):
        for S in (1, 2, 8):
            assert _work(h, B, S, 0) == (0, (1 if B else 0) * S * 256) and _work(h, B, S, 1) == (0, B * S * 256), (B, S)
    assert h.mfpa_sosfilt_work(1, 1, 0, None) == lib.EINVAL
    for B, S, per_row in ((-1, 1, 0), (65536, 1, 0), (1, 0, 0), (1, 9, 0), (1, 1, 2), (1, 1, -1)):
        assert _work(h, B, S, per_row) == (lib.EINVAL, -7), (B, S, per_row)


@pytest.mark.parametrize("change", [dict(x=None), dict(y=None), dict(sos=None), dict(work=None), dict(x=P + 2), dict(y=P + 2),
                                    dict(x=P + 4, x_f64=1), dict(y=P + 4, x_f64=1), dict(sos=P + 4), dict(work=P + 4), dict(zi=P + 4),
                                    dict(zf=P + 4), dict(S=0), dict(S=9), dict(S=-1), dict(T=0), dict(T=-5), dict(T=(1 << 30) + 1),
                                    dict(B=-1), dict(B=65536), dict(work_len=255), dict(S=8, work_len=8 * 256 - 1),
                                    dict(sos_per_row=1, work_len=2 * 256 - 1), dict(work_len=-1), dict(x_f64=2), dict(x_f64=-1), dict(clamp=2),
                                    dict(clamp=-1), dict(sos_per_row=2), dict(sos_per_row=-1)], ids=str)
def test_sosfilt_rejects_before_any_launch(lib, change):
    assert _sosfilt(lib.lib(), **change) == lib.EINVAL


def test_empty_batch_is_a_no_op_but_a_bad_shape_is_still_an_error(lib):
    h = lib.lib()
    assert _sosfilt(h, B=0) == 0 and _sosfilt(h, B=0, x=None, y=None, sos=None, work=None, work_len=0) == 0
    assert _sosfilt(h, B=0, T=1 << 30, S=8, sos_per_row=1, x_f64=1, clamp=1, work_len=0) == 0
    for bad in (dict(T=0), dict(S=9), dict(S=0), dict(x_f64=2), dict(clamp=3), dict(sos_per_row=2), dict(T=(1 << 30) + 1)):
        assert _sosfilt(h, B=0, **bad) == lib.EINVAL, bad


def test_python_refusals_need_no_gpu():
    from musicfpaugment_amd import functional as F
    from musicfpaugment_amd import ops
    from musicfpaugment_amd.augmentation.transformations.equalizer import HighShelfFilter, LowShelfFilter, ParametricEQ, PeakingFilter
    x = torch.zeros(2, 100)
    ok = [1.0, 0.0, 0.0, 1.0, 0.0, 0.0]
    for bad in ([[1.0, 0.0, 0.0, 0.0, 0.0, 0.0]], [[float("nan"), 0.0, 0.0, 1.0, 0.0, 0.0]], [[1.0, 0.0, 0.0, 1.0, float("inf"), 0.0]],
                [ok] * 9, [ok[:5]], ok, [[ok], [ok], [ok]], np.zeros((0, 6))):
        with pytest.raises(ValueError):
            ops.sosfilt(x, bad)
    with pytest.raises(ValueError):
        ops.sosfilt(torch.zeros(100), [ok])
    with pytest.raises(ValueError):
        ops.sosfilt(x.to(torch.float16), [ok])
    with pytest.raises(ValueError):
        ops.sosfilt(x, [ok], apply=torch.ones(3, dtype=torch.bool))
    with pytest.raises(ValueError):
        ops.sosfilt(x, [ok], zi=torch.zeros(2, 2, 2, dtype=torch.float64))
    np.testing.assert_array_equal(ops.sos_normalized([[2.0, 4.0, 6.0, 2.0, 1.0, -1.0]]), [[1.0, 2.0, 3.0, 1.0, 0.5, -0.5]])
    with pytest.raises(NotImplementedError, match="ops.sosfilt"):
        F.lfilter(x, [1.0, 0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0])                       # order 3
    with pytest.raises(ValueError):
        F.lfilter(x, [1.0, 0.0], [1.0, 0.0, 0.0])
    with pytest.raises(ValueError):
        F.lfilter(x, [0.0, 1.0], [1.0, 0.0])                                           # a0 == 0
    with pytest.raises(ValueError):
        F.biquad(x, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    with pytest.raises(ValueError):
        F.biquad(x, float("nan"), 0.0, 0.0, 1.0, 0.0, 0.0)
    for f in (4000.0, 5000.0, 0.0, -1.0):                                              # at or above the Nyquist frequency, or not positive
        with pytest.raises(ValueError):
            F.biquad_coefficients("peaking", 8000, f, 1.0, 3.0)
        with pytest.raises(ValueError):
            F.equalizer_biquad(x, 8000, f, 3.0)
        with pytest.raises(ValueError):
            F.lowpass_biquad(x, 8000, f)
    with pytest.raises(ValueError):
        F.biquad_coefficients("peaking", 8000, 100.0, 1.0)                             # no gain
    with pytest.raises(ValueError):
        F.biquad_coefficients("peaking", 8000, 100.0, 0.0, 3.0)
    with pytest.raises(ValueError):
        F.biquad_coefficients("notch", 8000, 100.0, 1.0)
    for cls in (PeakingFilter, LowShelfFilter, HighShelfFilter):
        cls()
        for bad in (dict(min_center_freq=500.0, max_center_freq=400.0), dict(min_gain_db=3.0, max_gain_db=-3.0), dict(min_q=2.0, max_q=0.05),
                    dict(min_q=0.0), dict(min_center_freq=0.0)):
            with pytest.raises(ValueError):
                cls(**bad)
    assert ParametricEQ().n_bands == 7 and ParametricEQ(n_bands=2).n_bands == 2 and ParametricEQ(n_bands=8).n_bands == 8
    for bad in (dict(n_bands=1), dict(n_bands=9), dict(n_bands=2.5), dict(min_gain_db=1.0, max_gain_db=-1.0), dict(min_freq=0.0),
                dict(max_freq_fraction=0.5), dict(max_freq_fraction=0.0)):
        with pytest.raises(ValueError):
            ParametricEQ(**bad)
    with pytest.raises(ValueError):
        ParametricEQ(min_freq=4000.0).band_centers(8000)
    c = ParametricEQ().band_centers(8000)
    np.testing.assert_allclose(c, np.geomspace(60.0, 3200.0, 7), rtol=0, atol=0)
    sec = ParametricEQ().band_sections(8000, [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0])
    assert sec.shape == (7, 6)
    np.testing.assert_array_equal(sec[0], F.biquad_coefficients("lowshelf", 8000, c[0], 0.707, 1.0))
    np.testing.assert_array_equal(sec[3], F.biquad_coefficients("peaking", 8000, c[3], 1.0, 4.0))
    np.testing.assert_array_equal(sec[6], F.biquad_coefficients("highshelf", 8000, c[6], 0.707, 7.0))


def test_no_cpu_fallback():
    from musicfpaugment_amd import functional as F
    from musicfpaugment_amd import ops
    from musicfpaugment_amd._lib import MfpaError
    from musicfpaugment_amd.augmentation.transformations.equalizer import HighShelfFilter, LowShelfFilter, ParametricEQ, PeakingFilter
    ok = [[1.0, 0.0, 0.0, 1.0, 0.0, 0.0]]
    with pytest.raises(MfpaError):
        ops.sosfilt(torch.zeros(2, 100), ok)
    with pytest.raises(MfpaError):
        ops.sosfilt(torch.zeros(2, 100, dtype=torch.float64), [ok, ok], zi=torch.zeros(2, 1, 2, dtype=torch.float64))
    for t in (PeakingFilter(p=1.0, sample_rate=8000), LowShelfFilter(p=1.0, sample_rate=8000), HighShelfFilter(p=1.0, sample_rate=8000),
              ParametricEQ(p=1.0, sample_rate=8000)):
        with pytest.raises(MfpaError):
            t(torch.zeros(2, 1, 8000))
    if not torch.cuda.is_available():
        x = torch.zeros(3, 100)
        calls = [lambda: F.lfilter(x, [1.0, -0.5], [1.0, 0.0]), lambda: F.lfilter(x, [[1.0, -0.5]] * 3, [[1.0, 0.0]] * 3),
                 lambda: F.lfilter(x, [[1.0, -0.5]] * 2, [[1.0, 0.0]] * 2, batching=False), lambda: F.biquad(x, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0),
                 lambda: F.lowpass_biquad(x, 8000, 1000.0), lambda: F.highpass_biquad(x, 8000, 1000.0),
                 lambda: F.bandpass_biquad(x, 8000, 1000.0), lambda: F.bandpass_biquad(x, 8000, 1000.0, const_skirt_gain=True),
                 lambda: F.bandreject_biquad(x, 8000, 1000.0), lambda: F.allpass_biquad(x, 8000, 1000.0),
                 lambda: F.equalizer_biquad(x, 8000, 1000.0, 6.0), lambda: F.bass_biquad(x, 8000, 6.0), lambda: F.treble_biquad(x, 8000, 6.0)]
        for call in calls:
            with pytest.raises(MfpaError):
                call()
