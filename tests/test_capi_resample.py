"""CPU: the resampling entry points (mfpa_resample_geometry, mfpa_resample_tile, mfpa_resample_taps, mfpa_resample) through
ctypes.  The first three are host functions; mfpa_resample checks its arguments before any launch and never dereferences a
pointer on the host, so all of this runs without a GPU (the style of tests/test_capi_maintain.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import _resample_oracle as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mfpa_resample_geometry", "mfpa_resample_taps", "mfpa_resample", "mfpa_resample_tile")


@pytest.fixture(scope="module")
def lib():
    from musicfpaugment_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from musicfpaugment_amd.csrc.build import build
        build(verbose=False)
    return _lib


def _geometry(h, orig, new, T=0, lpw=6, rolloff=0.99):
    o, n, w, k = (ctypes.c_int(-1) for _ in range(4))
    tout = ctypes.c_longlong(-1)
    rc = h.mfpa_resample_geometry(orig, new, lpw, rolloff, T, *(ctypes.addressof(v) for v in (o, n, w, k, tout)))
    return rc, (o.value, n.value, w.value, k.value), tout.value


def _resample(h, **kw):
    a = dict(x=8, B=3, T=1001, ldx=1001, o=2, n=1, width=13, taps=8, y=8, Tout=501, ldy=501, stream=None)
    a.update(kw)
    return h.mfpa_resample(a["x"], a["B"], a["T"], a["ldx"], a["o"], a["n"], a["width"], a["taps"], a["y"], a["Tout"], a["ldy"],
                           a["stream"])


def test_symbols_header_and_abi_version(lib):
    h = lib.lib()
    header = open(os.path.join(ROOT, "include", "mfpa.h")).read()
    declared = set(re.findall(r"^int\s+(mfpa_\w+)\s*\(", header, flags=re.M))
    for name in NEW:
        assert name in lib.exported_symbols() and name in declared and hasattr(h, name), name
    assert lib.ABI_VERSION == 47 and h.mfpa_version() == 47              # the new symbols are additive


@pytest.mark.parametrize("pair", sorted(ro.TABLE), ids=str)
def test_geometry_table(lib, pair):
    rc, geo, tout = _geometry(lib.lib(), *pair)
    assert rc == 0 and geo == ro.TABLE[pair] and tout == 0
    assert lib.lib().mfpa_resample_tile(*geo[:3]) >= 1                   # every pair of the table is within the kernel's limits


@pytest.mark.parametrize("case", sorted(ro.LENGTHS), ids=str)
def test_geometry_output_lengths(lib, case):
    rc, _, tout = _geometry(lib.lib(), case[0], case[1], case[2])
    assert rc == 0 and tout == ro.LENGTHS[case]


def test_geometry_rejects(lib):
    h = lib.lib()
    for bad in (dict(orig=0), dict(orig=-8000), dict(new=0), dict(new=-1), dict(lpw=0), dict(lpw=-6), dict(rolloff=0.0),
                dict(rolloff=-0.5), dict(rolloff=1.01), dict(rolloff=float("nan")), dict(T=-1), dict(T=(1 << 40) + 1),
                dict(orig=44101, new=8000),            # coprime: o = 44101, n = 8000, more phases and taps than the kernel takes
                dict(orig=8000, new=1025 * 8000)):     # n = 1025 phases
        a = dict(orig=44100, new=8000, T=10, lpw=6, rolloff=0.99)
        a.update(bad)
        assert _geometry(h, **a)[0] == lib.EINVAL, bad
    assert h.mfpa_resample_geometry(44100, 8000, 6, 0.99, 10, None, None, None, None, None) == 0     # every output is optional
    assert _geometry(h, 8000, 8000, 77) == (0, (1, 1, 7, 15), 77)
    assert _geometry(h, 44100, 8000, 1 << 40)[0] == 0
    assert h.mfpa_resample_tile(0, 1, 13) == lib.EINVAL and h.mfpa_resample_tile(2, 1025, 13) == lib.EINVAL
    assert h.mfpa_resample_tile(441, 80, 34) == 64 and h.mfpa_resample_tile(160, 147, 7) == 64    # one frame per lane of a wave
    assert h.mfpa_resample_tile(2, 1, 13) == 1792 and h.mfpa_resample_tile(1, 2, 7) == 2048       # four waves of frames, 7 and 8 rounds
    assert h.mfpa_resample_tile(6, 1, 37) == 512
    assert h.mfpa_resample_tile(4000, 1, 2000) == (36864 - 8000) // 4000 + 1            # the LDS window caps the tile


@pytest.mark.parametrize("pair", sorted(ro.TABLE), ids=str)
def test_taps_against_the_oracle(lib, pair):
    """One float32 rounding of a float64 value good to a few ulp: |tap - oracle| <= 2^-24 |tap| + 1e-15; phase-major rows at the
    header's pitch, zeros behind the taps of a row and nothing written behind the bank."""
    from musicfpaugment_amd import ops
    o, n, width, K = ro.TABLE[pair]
    header = open(os.path.join(ROOT, "include", "mfpa.h")).read()
    assert int(re.search(r"#define MFPA_RESAMPLE_TAP_ALIGN (\d+)", header).group(1)) == ops.RESAMPLE_TAP_ALIGN
    pitch = ops.resample_tap_pitch(K)
    assert pitch % 16 == 0 and K <= pitch < K + 16
    buf = np.full(n * pitch + 8, np.nan, dtype=np.float32)
    assert lib.lib().mfpa_resample_taps(o, n, width, 6, 0.99, buf.ctypes.data_as(ctypes.c_void_p)) == 0
    taps = buf[:n * pitch].reshape(n, pitch)
    want = ro.taps64(*pair)                                              # (n, K)
    assert np.all(np.abs(taps[:, :K].astype(np.float64) - want) <= 2.0 ** -24 * np.abs(want) + 1e-15)
    assert np.all(taps[:, K:] == 0) and np.all(np.isnan(buf[n * pitch:]))


def test_taps_rejects(lib):
    h = lib.lib()
    buf = np.zeros(64, dtype=np.float32).ctypes.data_as(ctypes.c_void_p)
    assert h.mfpa_resample_taps(2, 1, 13, 6, 0.99, None) == lib.EINVAL
    for bad in ((0, 1, 13, 6, 0.99), (2, 0, 13, 6, 0.99), (2, 1, 0, 6, 0.99), (2, 1, 13, 0, 0.99), (2, 1, 13, 6, 0.0), (2, 1, 13, 6, 1.5),
                (2, 1025, 13, 6, 0.99), (2, 1, 4096, 6, 0.99)):
        assert h.mfpa_resample_taps(*bad, buf) == lib.EINVAL, bad


@pytest.mark.parametrize("change", [dict(x=None), dict(taps=None), dict(y=None), dict(ldx=1000), dict(ldy=500), dict(Tout=502, ldy=502),
                                    dict(B=-1), dict(T=-1), dict(Tout=-1), dict(o=0), dict(n=0), dict(width=0), dict(n=1025),
                                    dict(width=4096), dict(B=65536), dict(T=(1 << 40) + 1, ldx=(1 << 40) + 1)], ids=str)
def test_resample_rejects_before_any_launch(lib, change):
    assert _resample(lib.lib(), **change) == lib.EINVAL


def test_empty_calls_are_no_ops(lib):
    h = lib.lib()
    assert _resample(h, B=0) == 0 and _resample(h, B=0, x=None, taps=None, y=None) == 0
    assert _resample(h, Tout=0, ldy=0) == 0 and _resample(h, Tout=0, ldy=0, T=0, ldx=0, x=None, y=None) == 0
    assert _resample(h, B=0, o=0) == lib.EINVAL                         # ... but a bad shape is still an error


def test_no_cpu_fallback():
    import torch
    from musicfpaugment_amd import ops
    from musicfpaugment_amd._lib import MfpaError
    with pytest.raises(MfpaError):
        ops.resample(torch.zeros(1, 100), 16000, 8000)
    assert ops.resample_geometry(44100, 8000, 4411) == (441, 80, 34, 509, 801)
    assert ops.resample_tile(44100, 8000) == 64
    if not torch.cuda.is_available():
        from musicfpaugment_amd.transforms import Resample
        with pytest.raises(MfpaError):
            Resample(16000, 8000)(torch.zeros(2, 100))
