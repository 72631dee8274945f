"""CPU: the sparse-tap resampling entry points (mfpa_resample_sparse_geometry, mfpa_resample_sparse_tile, mfpa_resample_sparse_taps,
mfpa_resample_sparse) through ctypes, and the host side of the Python surface built on them.  The first three are host functions;
mfpa_resample_sparse checks its arguments before any launch and never dereferences a pointer on the host, so all of this runs
without a GPU (the style of tests/test_capi_resample.py)."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import _resample_oracle as ro
from tests import _resample_sparse_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mfpa_resample_sparse_geometry", "mfpa_resample_sparse_taps", "mfpa_resample_sparse", "mfpa_resample_sparse_tile")
# (orig, new) -> (o, n, width, S), output samples per workgroup (1024 while their input span stays within 16384 floats)
LARGE = {
    (8979, 8000): ((8979, 8000, 7, 16), 1024),
    (7127, 8000): ((7127, 8000, 7, 16), 1024),
    (11313, 8000): ((11313, 8000, 9, 20), 1024),
    (8979, 1000): ((8979, 1000, 55, 112), 1024),
    (1025, 2048): ((1025, 2048, 7, 16), 1024),
}


@pytest.fixture(scope="module")
def lib():
    from musicfpaugment_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from musicfpaugment_amd.csrc.build import build
        build(verbose=False)
    return _lib


def _geometry(h, orig, new, T=0, lpw=6, rolloff=0.99):
    o, n, w, s = (ctypes.c_int(-1) for _ in range(4))
    tout = ctypes.c_longlong(-1)
    rc = h.mfpa_resample_sparse_geometry(orig, new, lpw, rolloff, T, *(ctypes.addressof(v) for v in (o, n, w, s, tout)))
    return rc, (o.value, n.value, w.value, s.value), tout.value


def _taps(h, o, n, width, lpw=6, rolloff=0.99):
    """(rc, taps (n, S) with 8 guard floats behind, first (n,) with 2 guard ints behind) -- the guards NaN / -7 as given."""
    S = (2 * width + 1 + 3) // 4 * 4
    taps = np.full(n * S + 8, np.nan, dtype=np.float32)
    first = np.full(n + 2, -7, dtype=np.int32)
    rc = h.mfpa_resample_sparse_taps(o, n, width, lpw, rolloff, taps.ctypes.data_as(ctypes.c_void_p), first.ctypes.data_as(ctypes.c_void_p))
    return rc, taps, first


def _resample(h, **kw):
    a = dict(x=16, B=3, T=8979, ldx=8979, o=8979, n=8000, width=7, support=16, taps=16, first=16, y=16, Tout=8000, ldy=8000, stream=None)
    a.update(kw)
    return h.mfpa_resample_sparse(a["x"], a["B"], a["T"], a["ldx"], a["o"], a["n"], a["width"], a["support"], a["taps"], a["first"], a["y"],
                                  a["Tout"], a["ldy"], a["stream"])


def test_symbols_header_and_abi_version(lib):
    h = lib.lib()
    header = open(os.path.join(ROOT, "include", "mfpa.h")).read()
    declared = set(re.findall(r"^int\s+(mfpa_\w+)\s*\(", header, flags=re.M))
    for name in NEW:
        assert name in lib.exported_symbols() and name in declared and hasattr(h, name), name
    assert lib.ABI_VERSION == 47 and h.mfpa_version() == 47              # the new symbols are additive
    for name, value in (("MAX_PHASES", "65536"), ("MAX_ORIG", "(1 << 20)"), ("MAX_SUPPORT", "512")):
        assert re.search(r"#define MFPA_RESAMPLE_SPARSE_%s %s\s" % (name, re.escape(value)), header), name


@pytest.mark.parametrize("pair", sorted(ro.TABLE), ids=str)
def test_the_sparse_bank_is_the_dense_bank_without_its_zeros(lib, pair):
    """Scattered into (n, K) by `first`, the sparse rows are the dense bank: equal as floats everywhere (a dropped tap of the dense
    bank may be -0.0f), bit for bit wherever the dense tap is not zero, and 0.0f at every position behind K."""
    from musicfpaugment_amd import ops
    h = lib.lib()
    o, n, width, K = ro.TABLE[pair]
    rc, geo, _ = _geometry(h, *pair)
    S = geo[3]
    assert rc == 0 and geo == (o, n, width, so.geometry(*pair)[4])
    pitch = ops.resample_tap_pitch(K)
    dense = np.empty((n, pitch), dtype=np.float32)
    assert h.mfpa_resample_taps(o, n, width, 6, 0.99, dense.ctypes.data_as(ctypes.c_void_p)) == 0
    dense = dense[:, :K]
    rc, buf, fbuf = _taps(h, o, n, width)
    assert rc == 0 and np.all(np.isnan(buf[n * S:])) and np.all(fbuf[n:] == -7)          # nothing written behind the tables
    taps, first = buf[:n * S].reshape(n, S), fbuf[:n]
    assert first.min() >= 0 and np.array_equal(first, so.first(*pair))
    scattered = np.zeros((n, K + S), dtype=np.float32)
    for i in range(n):
        scattered[i, first[i]:first[i] + S] = taps[i]
    assert np.array_equal(scattered[:, :K], dense)
    nz = dense != 0
    assert np.array_equal(scattered[:, :K].view(np.uint32)[nz], dense.view(np.uint32)[nz])
    k = first[:, None] + np.arange(S)[None, :]
    assert np.array_equal(taps.view(np.uint32)[k >= K], np.zeros(int((k >= K).sum()), dtype=np.uint32))      # +0.0f behind the dense row


@pytest.mark.parametrize("pair", sorted(LARGE), ids=str)
def test_geometry_tile_and_tables_of_the_large_pairs(lib, pair):
    h = lib.lib()
    geo, tile = LARGE[pair]
    o, n, width, S = geo
    L = 2 * o + 17
    rc, got, tout = _geometry(h, *pair, T=L)
    assert rc == 0 and got == geo and tout == ro.out_len(*pair, L) and so.geometry(*pair)[4] == S
    assert h.mfpa_resample_sparse_tile(o, n, width) == tile
    rc, buf, fbuf = _taps(h, o, n, width)
    assert rc == 0 and np.all(np.isnan(buf[n * S:])) and np.all(fbuf[n:] == -7)
    want_taps, want_first = so.taps32(*pair)
    assert np.array_equal(fbuf[:n], want_first)
    got_taps = buf[:n * S].reshape(n, S).astype(np.float64)
    assert np.all(np.abs(got_taps - want_taps) <= 2.0 ** -24 * np.abs(want_taps) + 1e-15)     # libm against numpy, one rounding each
    assert np.array_equal(got_taps == 0, want_taps == 0)


def test_tile_follows_the_window(lib):
    h = lib.lib()
    assert h.mfpa_resample_sparse_tile(441, 80, 34) == 1024 and h.mfpa_resample_sparse_tile(2, 1, 13) == 1024
    assert h.mfpa_resample_sparse_tile(1, 2, 7) == 1024
    # 42 : 1, 512 taps: (tile - 1) * 42 + 3 + 512 <= 16384 floats gives 378 outputs, 320 as a multiple of 64
    assert h.mfpa_resample_sparse_tile(42, 1, 255) == 320
    for bad in ((0, 1, 13), (2, 0, 13), (2, 1, 0), (2, 65537, 13), ((1 << 20) + 1, 8000, 7), (2, 1, 256)):
        assert h.mfpa_resample_sparse_tile(*bad) == lib.EINVAL, bad
    # a width that is not the geometry's: 64 outputs of 1000 : 1 span 63000 floats, more than a workgroup stages
    assert h.mfpa_resample_sparse_tile(1000, 1, 7) == lib.EINVAL
    assert _resample(h, o=1000, n=1, width=7, support=16, T=8000, ldx=8000, Tout=8, ldy=8) == lib.EINVAL


def test_geometry_rejects(lib):
    h = lib.lib()
    for bad in (dict(orig=0), dict(orig=-8000), dict(new=0), dict(new=-1), dict(lpw=0), dict(lpw=-6), dict(rolloff=0.0),
                dict(rolloff=-0.5), dict(rolloff=1.01), dict(rolloff=float("nan")), dict(T=-1), dict(T=(1 << 40) + 1),
                dict(orig=8000, new=65537),             # coprime: n = 65537 phases
                dict(orig=(1 << 20) + 1, new=8000),     # coprime: o = 2^20 + 1
                dict(orig=96000, new=95999),            # n = 95999
                dict(orig=43, new=1),                   # width = ceil(6 * 43 / 0.99) = 261: more than 512 taps
                dict(orig=8000, new=8979, lpw=253)):    # width = ceil(253 / 0.99) = 256
        a = dict(orig=8979, new=8000, T=10, lpw=6, rolloff=0.99)
        a.update(bad)
        assert _geometry(h, **a) == (lib.EINVAL, (-1, -1, -1, -1), -1), bad           # ... and nothing written
    assert h.mfpa_resample_sparse_geometry(8979, 8000, 6, 0.99, 10, None, None, None, None, None) == 0    # every output is optional
    assert _geometry(h, 8000, 8979, lpw=252)[1] == (8000, 8979, 255, 512)              # the widest support
    assert _geometry(h, 65535, 65534)[:2] == (0, (65535, 65534, 7, 16))
    assert _geometry(h, 42, 1)[:2] == (0, (42, 1, 255, 512))
    assert _geometry(h, 8979, 8000, 1 << 40)[0] == 0


def test_taps_reject_and_write_nothing(lib):
    h = lib.lib()
    buf = np.zeros(64, dtype=np.float32).ctypes.data_as(ctypes.c_void_p)
    ibuf = np.zeros(8, dtype=np.int32).ctypes.data_as(ctypes.c_void_p)
    assert h.mfpa_resample_sparse_taps(2, 1, 13, 6, 0.99, None, ibuf) == lib.EINVAL
    assert h.mfpa_resample_sparse_taps(2, 1, 13, 6, 0.99, buf, None) == lib.EINVAL
    for bad in ((0, 1, 13, 6, 0.99), (2, 0, 13, 6, 0.99), (2, 1, 0, 6, 0.99), (2, 1, 13, 0, 0.99), (2, 1, 13, 6, 0.0), (2, 1, 13, 6, 1.5),
                (2, 65537, 13, 6, 0.99), ((1 << 20) + 1, 1, 13, 6, 0.99), (2, 1, 256, 6, 0.99)):
        assert h.mfpa_resample_sparse_taps(*bad, buf, ibuf) == lib.EINVAL, bad
    # a width that does not belong to (o, n, lowpass_filter_width): with o = 8, width 13 and a filter width of 60 all K = 34 taps
    # of the dense row lie inside |t| < 60, and S = 28 -- refused by the builder's own proof, with both tables untouched
    rc, taps, first = _taps(h, 8, 1, 13, lpw=60)
    assert rc == lib.EINVAL and np.all(np.isnan(taps)) and np.all(first == -7)


@pytest.mark.parametrize("change", [dict(x=None), dict(taps=None), dict(first=None), dict(y=None), dict(ldx=8978), dict(ldy=7999),
                                    dict(Tout=16001, ldy=16001), dict(B=-1), dict(T=-1), dict(Tout=-1), dict(o=0), dict(n=0), dict(width=0),
                                    dict(n=65537), dict(o=(1 << 20) + 1), dict(width=256, support=516), dict(support=15), dict(support=20),
                                    dict(taps=20), dict(B=65536), dict(T=(1 << 40) + 1, ldx=(1 << 40) + 1)], ids=str)
def test_resample_sparse_rejects_before_any_launch(lib, change):
    assert _resample(lib.lib(), **change) == lib.EINVAL


def test_empty_calls_are_no_ops(lib):
    h = lib.lib()
    assert _resample(h, B=0) == 0 and _resample(h, B=0, x=None, taps=None, first=None, y=None) == 0
    assert _resample(h, Tout=0, ldy=0) == 0 and _resample(h, Tout=0, ldy=0, T=0, ldx=0, x=None, y=None) == 0
    assert _resample(h, B=0, o=0) == lib.EINVAL                         # ... but a bad shape is still an error


def test_constructors_and_refusals_on_the_host():
    import torch
    from musicfpaugment_amd import ops
    from musicfpaugment_amd import transforms as tr
    from musicfpaugment_amd._lib import MfpaError
    assert ops.resample_sparse_geometry(8979, 8000, 2 * 8979 + 17) == (8979, 8000, 7, 16, 16016)
    assert ops.resample_sparse_tile(8979, 8000) == 1024
    ps = tr.PitchShift(8000, 2, any_ratio=True)
    assert ps.ratio == Fraction(8979, 8000) and ps.any_ratio
    sp = tr.Speed(8000, 1.0123, any_ratio=True)
    assert (sp.resampler.orig_freq, sp.resampler.new_freq, sp.resampler.any_ratio) == (4049, 4000, True)
    assert tr.Resample(8979, 8000, any_ratio=True).any_ratio and not tr.Resample(44100, 8000).any_ratio
    with pytest.raises(ValueError):
        tr.Resample(96000, 95999, any_ratio=True)                         # 95999 phases: beyond the sparse kernel too
    for refused in (lambda: tr.PitchShift(8000, 2), lambda: tr.Speed(8000, 1.0123), lambda: tr.Resample(8979, 8000)):
        with pytest.raises(ValueError, match="any_ratio"):                # the default still refuses, and says what would not
            refused()
    with pytest.raises(MfpaError):
        ops.resample(torch.zeros(1, 100), 8979, 8000, any_ratio=True)     # no CPU fallback
    if not torch.cuda.is_available():
        with pytest.raises(MfpaError):
            tr.Resample(8979, 8000, any_ratio=True)(torch.zeros(2, 100))
