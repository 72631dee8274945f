#!/usr/bin/env python
"""Write tests/golden/g16_nplog_f32.npz: (float32 bit pattern, bit pattern of numpy's float32 log of it) pairs that pin the function
csrc/mfpa_nplog.h restates -- np.log of a float32 array as numpy's SIMD kernel computes it (the reference's arithmetic on the denoised
branch, afp/audfprint/peak_extractor.py:265-276, afp/dejavu/fingerprint.py:70-79).  Needs numpy only.

    python tools/make_nplog_golden.py                write the fixture
    python tools/make_nplog_golden.py --exhaustive   compile csrc/mfpa_nplog.h with gcc and compare it with np.log on EVERY
                                                     non-negative float32 (2^31 values, well under a minute); writes nothing

numpy takes its SIMD float32 log only where AVX512F or AVX2 + FMA3 is enabled; elsewhere it calls libm's logf, another function.  The
tool refuses to write a fixture there."""
import argparse
import ctypes
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g16_nplog_f32.npz")
INV_SQRT2 = np.float32(0.70710678)

HOST_SRC = r"""
#define MFPA_NPLOG_HOST
#include "mfpa_nplog.h"
void nplog(const float* x, float* y, long n) { for (long i = 0; i < n; ++i) y[i] = mfpa_nplogf(x[i]); }
"""


def numpy_simd_log() -> bool:
    """True where np.log of a float32 array is numpy's own SIMD kernel (the function the fixture pins)."""
    from numpy._core._multiarray_umath import __cpu_features__ as f
    return bool(f.get("AVX512F") or (f.get("AVX2") and f.get("FMA3")))


def cpu_features():
    from numpy._core._multiarray_umath import __cpu_features__ as f
    return sorted(k for k, v in f.items() if v)


def build_host(workdir: str) -> ctypes.CDLL:
    """csrc/mfpa_nplog.h compiled for the host (gcc, -ffp-contract=off: only the marked multiply-adds are fused)."""
    gcc = shutil.which("gcc")
    if gcc is None:
        raise RuntimeError("no gcc")
    c = os.path.join(workdir, "nplog_host.c")
    with open(c, "w") as fh:
        fh.write(HOST_SRC)
    so = os.path.join(workdir, "libnplog_host.so")
    subprocess.run([gcc, "-O2", "-mfma", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "musicfpaugment_amd", "csrc"),
                    "-o", so, c, "-lm"], check=True)
    h = ctypes.CDLL(so)
    h.nplog.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long]
    h.nplog.restype = None
    return h


def host_log_bits(h: ctypes.CDLL, bits: np.ndarray) -> np.ndarray:
    x = np.ascontiguousarray(bits, dtype=np.uint32)
    y = np.empty_like(x)
    h.nplog(x.ctypes.data_as(ctypes.c_void_p), y.ctypes.data_as(ctypes.c_void_p), x.size)
    return y


def numpy_log_bits(bits: np.ndarray) -> np.ndarray:
    with np.errstate(all="ignore"):
        return np.log(np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32)).view(np.uint32)


def inputs(seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    parts = []
    # random normals over the whole exponent range
    n = 24000
    parts.append((rng.integers(1, 255, n).astype(np.uint32) << 23) | rng.integers(0, 1 << 23, n).astype(np.uint32))
    # +-64 ulps around the mantissa switch 0.70710678f * 2^k, and around 1
    d = np.arange(-64, 65).astype(np.int64)
    for k in (-125, -100, -40, -20, -6, -3, -2, -1, 0, 1, 2, 3, 6, 20, 40, 100, 127):
        c = np.ldexp(INV_SQRT2, k).astype(np.float32)
        parts.append((np.int64(c.view(np.uint32)) + d).astype(np.uint32))
    parts.append((np.int64(np.float32(1.0).view(np.uint32)) + d).astype(np.uint32))
    # FLT_MIN, FLT_MAX
    parts.append(np.array([0x00800000, 0x7f7fffff], dtype=np.uint32))
    # 256 denormals: both ends, the powers of two and random ones
    den = np.concatenate([np.array([1, 2, 3, 0x007fffff, 0x007ffffe, 0x00400000], dtype=np.uint32),
                          (np.uint32(1) << np.arange(2, 22, dtype=np.uint32)),
                          rng.integers(1, 1 << 23, 230).astype(np.uint32)])
    assert den.size == 256 and den.max() < 0x00800000 and den.min() > 0
    parts.append(den)
    # 0 and +inf
    parts.append(np.array([0x00000000, 0x7f800000], dtype=np.uint32))
    x = np.concatenate(parts)
    assert x.size <= 32768
    return x


def exhaustive() -> int:
    with tempfile.TemporaryDirectory() as d:
        h = build_host(d)
        t0 = time.time()
        bad = 0
        step = 1 << 24
        for lo in range(0, 0x7f800000 + 1, step):
            bits = np.arange(lo, min(lo + step, 0x7f800000 + 1), dtype=np.uint32)
            diff = host_log_bits(h, bits) != numpy_log_bits(bits)
            if diff.any():
                bad += int(diff.sum())
                i = int(np.flatnonzero(diff)[0])
                print(f"first difference in [{lo:#010x}, ...): x bits {int(bits[i]):#010x}")
        print(f"numpy {np.__version__}, {'AVX512F' if 'AVX512F' in cpu_features() else 'AVX2+FMA3'} dispatch: "
              f"{bad} differences on all {0x7f800000 + 1} non-negative float32 values (0, denormals, normals, +inf) in {time.time() - t0:.0f} s")
        return bad


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--exhaustive", action="store_true", help="compare the header with np.log on every non-negative float32; write nothing")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if not numpy_simd_log():
        print("neither AVX512F nor AVX2+FMA3 is enabled in this numpy: np.log(float32) is libm's logf here, not the SIMD kernel the "
              "fixture pins -- refusing to write", file=sys.stderr)
        return 2
    if args.exhaustive:
        return 1 if exhaustive() else 0
    x = inputs()
    np.savez_compressed(args.out, x_bits=x, log_bits=numpy_log_bits(x), numpy_version=np.array(np.__version__),
                        cpu_features=np.array(cpu_features()))
    print(f"{args.out}: {x.size} pairs, {os.path.getsize(args.out)} bytes, numpy {np.__version__}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
