"""csrc/mfpa_nplog.h (numpy's float32 logarithm restated: the `float32_log="numpy"` mode of the pickers' denoised branch) compiled for
the HOST with gcc -- the very header the device kernels include -- and compared bit for bit with the committed fixture and with live
np.log (the reference's arithmetic, afp/audfprint/peak_extractor.py:265-276, afp/dejavu/fingerprint.py:70-79); plus the CPU-side
checks of the mode's C ABI and Python keyword."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = r"""
#define MFPA_NPLOG_HOST
#include "mfpa_nplog.h"
void nplog(const float* x, float* y, long n) { for (long i = 0; i < n; ++i) y[i] = mfpa_nplogf(x[i]); }
"""


def _numpy_simd_log():
    """np.log of a float32 array is numpy's own SIMD kernel only where AVX512F or AVX2 + FMA3 is enabled (libm's logf elsewhere)."""
    from numpy._core._multiarray_umath import __cpu_features__ as f
    return bool(f.get("AVX512F") or (f.get("AVX2") and f.get("FMA3")))


needs_simd_log = pytest.mark.skipif(not _numpy_simd_log(), reason="this numpy has neither AVX512F nor AVX2+FMA3 enabled: its float32 log "
                                    "is libm's logf, not the SIMD kernel mfpa_nplog.h restates -- live comparison skipped (the fixture still holds)")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    d = tmp_path_factory.mktemp("nplog")
    c = d / "nplog_host.c"
    c.write_text(SRC)
    so = d / "libnplog_host.so"
    subprocess.run([gcc, "-O2", "-mfma", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "musicfpaugment_amd", "csrc"),
                    "-o", str(so), str(c), "-lm"], check=True)
    h = ctypes.CDLL(str(so))
    h.nplog.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long]
    h.nplog.restype = None

    def log_bits(bits):
        x = np.ascontiguousarray(bits, dtype=np.uint32)
        y = np.empty_like(x)
        h.nplog(x.ctypes.data_as(ctypes.c_void_p), y.ctypes.data_as(ctypes.c_void_p), x.size)
        return y
    return log_bits


def _np_log_bits(bits):
    with np.errstate(all="ignore"):
        return np.log(np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32)).view(np.uint32)


def test_header_equals_the_fixture_on_every_pair(host, golden):
    g = golden("g16_nplog_f32")
    x, want = g["x_bits"], g["log_bits"]
    assert x.dtype == np.uint32 and want.dtype == np.uint32 and 20000 < x.size <= 32768
    feats = set(g["cpu_features"].tolist())
    assert "AVX512F" in feats or {"AVX2", "FMA3"} <= feats              # written where np.log was numpy's SIMD kernel
    # what the fixture must cover: denormals, 0, +inf, FLT_MIN, FLT_MAX, both sides of the mantissa switch at sqrt(1/2), every binade
    assert np.count_nonzero((x > 0) & (x < 0x00800000)) == 256
    for v in (0x00000000, 0x7f800000, 0x00800000, 0x7f7fffff, 0x3f800000, 0x3f3504f3, 0x3f3504f4):
        assert v in x, hex(v)
    assert len(np.unique(x[(x >= 0x00800000) & (x < 0x7f800000)] >> 23)) == 254
    got = host(x)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(hex(int(x[i])), hex(int(got[i])), hex(int(want[i]))) for i in bad[:5]]


@needs_simd_log
def test_header_equals_live_numpy_log(host):
    """Bit-equal to np.log on every float32 in [0.25, 4) (2^25 values: both sides of the mantissa switch in four binades, the zone
    around 1), on every denormal, and on a stride-37 walk of all normal values.  (tools/make_nplog_golden.py --exhaustive covers
    all 2^31; NOTES.md has its result.)"""
    ranges = [(0x3e800000, 0x40800000, 1), (0x00000001, 0x00800000, 1), (0x00800000, 0x7f800000, 37)]
    for lo, hi, step in ranges:
        chunk = (1 << 24) * step
        for a in range(lo, hi, chunk):
            bits = np.arange(a, min(a + chunk, hi), step, dtype=np.uint32)
            got, want = host(bits), _np_log_bits(bits)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (hex(lo), [(hex(int(bits[i])), hex(int(got[i])), hex(int(want[i]))) for i in bad[:5]])


def test_special_values(host):
    x = np.array([0.0, np.inf, np.nan, -1.0, -0.0, -np.inf, -1e-45, 1.0, 1e-45], dtype=np.float32)
    got = host(x.view(np.uint32)).view(np.float32)
    with np.errstate(all="ignore"):
        want = np.log(x)
    assert got[0] == -np.inf and got[1] == np.inf and np.isnan(got[2]) and np.isnan(got[3]) and got[4] == -np.inf
    assert np.isnan(got[5]) and np.isnan(got[6]) and got[7] == 0.0 and not np.signbit(got[7])
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    if _numpy_simd_log():
        np.testing.assert_array_equal(got[~np.isnan(got)], want[~np.isnan(want)])


def test_build_flags_keep_the_division_correctly_rounded_and_contraction_off():
    """mfpa_nplogf needs an IEEE correctly rounded float32 division and no contraction beyond its explicit fmaf calls."""
    from musicfpaugment_amd.csrc import build as b
    for src in ("audfprint.hip", "dejavu.hip", "nplog.hip"):
        flags = b.COMMON + b.PER_FILE.get(src, [])
        assert "-ffp-contract=off" in flags, src
        assert not any(re.search(r"fast-math|unsafe-math|reciprocal-math|no-hip-fp32-correctly-rounded|approx-func|Ofast", f) for f in flags), flags
    hdr = open(os.path.join(ROOT, "musicfpaugment_amd", "csrc", "mfpa_nplog.h")).read()
    assert "__fdiv_rn" in hdr and "#pragma clang fp contract(off)" in hdr and hdr.count("__builtin_fmaf") == 11


@pytest.fixture(scope="module")
def lib():
    from musicfpaugment_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from musicfpaugment_amd.csrc.build import build
        build(verbose=False)
    return _lib


def test_abi_symbols_and_flag_errors(lib):
    header = open(os.path.join(ROOT, "include", "mfpa.h")).read()
    h = lib.lib()
    for name in ("mfpa_nplog_f32", "mfpa_dejavu_prepare_f32_ex"):
        assert re.search(r"^int\s+%s\s*\(" % name, header, flags=re.M), name
        assert name in lib.exported_symbols() and hasattr(h, name)
    assert int(re.search(r"#define MFPA_LOG_NUMPY_F32 (\d+)", header).group(1)) == 4
    assert int(re.search(r"#define MFPA_F32LOG_NUMPY (\d+)", header).group(1)) == 1
    assert h.mfpa_version() == lib.ABI_VERSION >= 43
    # the numpy float32 log has no meaning for float64 spectrograms or for caller-made log values: rejected before any launch
    assert h.mfpa_audfprint_prepare(1, lib.F64, 1, 257, 10, None, 0, 4, 0.98, 1, 1, None) == lib.EINVAL
    assert h.mfpa_audfprint_prepare(1, lib.F64, 1, 257, 10, None, 0, 6, 0.98, 1, 1, None) == lib.EINVAL
    assert h.mfpa_audfprint_prepare(1, lib.F32, 1, 257, 10, None, 0, 5, 0.98, 1, 1, None) == lib.EINVAL
    assert h.mfpa_audfprint_prepare(1, lib.F32, 0, 257, 10, None, 0, 4, 0.98, 1, 1, None) == 0      # empty batch
    assert h.mfpa_dejavu_prepare_f32_ex(1, 1, 257, 10, 1, 10.0, 0, 2, 1, None) == lib.EINVAL      # no such logarithm
    assert h.mfpa_dejavu_prepare_f32_ex(1, 1, 257, 10, 1, 10.0, 0, -1, 1, None) == lib.EINVAL
    assert h.mfpa_dejavu_prepare_f32_ex(None, 1, 257, 10, 1, 10.0, 0, 1, 1, None) == lib.EINVAL
    assert h.mfpa_dejavu_prepare_f32_ex(1, 0, 257, 10, 1, 10.0, 0, 1, 1, None) == 0               # empty batch
    assert h.mfpa_nplog_f32(None, 1, 5, None) == lib.EINVAL and h.mfpa_nplog_f32(1, None, 5, None) == lib.EINVAL
    assert h.mfpa_nplog_f32(1, 1, -1, None) == lib.EINVAL and h.mfpa_nplog_f32(None, None, 0, None) == 0
    assert h.mfpa_nplog_f32(64, 64, 4, None) == lib.EINVAL                                       # in place: the ranges must not overlap
    assert h.mfpa_nplog_f32(64, 76, 4, None) == lib.EINVAL and h.mfpa_nplog_f32(76, 64, 4, None) == lib.EINVAL


def test_bad_float32_log_string_raises_value_error(lib):
    from musicfpaugment_amd import ops
    from musicfpaugment_amd.afp.audfprint.peak_extractor import Audfprint_peaks
    from musicfpaugment_amd.afp.dejavu.fingerprint import fingerprint, fingerprint_batch, fingerprint_peaks_batch
    from musicfpaugment_amd.pipeline import HotPath
    spec = torch.zeros((1, 257, 8), dtype=torch.float32)
    wav = torch.zeros((1, 2048), dtype=torch.float32)
    for bad in ("Numpy", "", "float64", None, 1):
        with pytest.raises(ValueError):
            ops.audfprint_prepare(spec, float32_log=bad)
        with pytest.raises(ValueError):
            ops.dejavu_prepare_f32(spec, float32_log=bad)
        with pytest.raises(ValueError):
            Audfprint_peaks(None, float32_log=bad)
        with pytest.raises(ValueError):
            HotPath(None, float32_log=bad)
        with pytest.raises(ValueError):
            HotPath(None, picker="dejavu", float32_log=bad)
        with pytest.raises(ValueError):
            fingerprint_peaks_batch(wav, float32_log=bad)
        with pytest.raises(ValueError):
            fingerprint_batch(wav, float32_log=bad)
        with pytest.raises(ValueError):
            fingerprint(wav[0].numpy(), float32_log=bad)
    for ok in ("rounded", "numpy"):                         # accepted: construction does no device work
        assert Audfprint_peaks(None, float32_log=ok).float32_log == ok
        assert HotPath(None, float32_log=ok).float32_log == ok
