"""CPU: the segment entry points (mfpa_segment_geometry, mfpa_segment_stats, mfpa_segment_select, mfpa_segment_gather) through
ctypes.  The first is a host function; the others check their arguments before any launch and never dereference a pointer on
the host, so all of this runs without a GPU (the style of tests/test_capi_resample.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import _segments_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mfpa_segment_geometry", "mfpa_segment_stats", "mfpa_segment_select", "mfpa_segment_gather")


@pytest.fixture(scope="module")
def lib():
    from musicfpaugment_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from musicfpaugment_amd.csrc.build import build
        build(verbose=False)
    return _lib


def _geometry(h, lengths, L, S):
    lens = np.asarray(lengths, dtype=np.int64)
    seg_off = np.full(len(lens) + 2, -7, dtype=np.int32)
    rc = h.mfpa_segment_geometry(lens.ctypes.data_as(ctypes.c_void_p), len(lens), L, S, seg_off.ctypes.data_as(ctypes.c_void_p))
    assert seg_off[-1] == -7                                             # nothing behind the n + 1 entries
    return rc, seg_off[:-1]


def _stats(h, **kw):
    a = dict(bank=8, off=8, len=8, seg_off=8, n=3, L=24, S=24, seg=8, trk=8, peak=8, stream=None)
    a.update(kw)
    return h.mfpa_segment_stats(a["bank"], a["off"], a["len"], a["seg_off"], a["n"], a["L"], a["S"], a["seg"], a["trk"], a["peak"], a["stream"])


def _select(h, **kw):
    a = dict(seg=8, trk=8, peak=8, off=8, len=8, seg_off=8, n=3, L=24, S=24, keys=8, thr=0.22, n_keep=2, do_norm=1, sel=8, src=8, div=8,
             kept=8, mask=8, stream=None)
    a.update(kw)
    return h.mfpa_segment_select(a["seg"], a["trk"], a["peak"], a["off"], a["len"], a["seg_off"], a["n"], a["L"], a["S"], a["keys"],
                                 a["thr"], a["n_keep"], a["do_norm"], a["sel"], a["src"], a["div"], a["kept"], a["mask"], a["stream"])


def _gather(h, **kw):
    a = dict(bank=8, src=8, div=8, rows=3, L=24, out=8, ldo=24, stream=None)
    a.update(kw)
    return h.mfpa_segment_gather(a["bank"], a["src"], a["div"], a["rows"], a["L"], a["out"], a["ldo"], a["stream"])


def test_symbols_header_and_abi_version(lib):
    h = lib.lib()
    header = open(os.path.join(ROOT, "include", "mfpa.h")).read()
    declared = set(re.findall(r"^int\s+(mfpa_\w+)\s*\(", header, flags=re.M))
    for name in NEW:
        assert name in lib.exported_symbols() and name in declared and hasattr(h, name), name
    assert lib.ABI_VERSION == 47 and h.mfpa_version() == 47              # the new symbols are additive
    assert int(re.search(r"#define MFPA_SEGMENT_MAX_PER_TRACK (\d+)", header).group(1)) == so.MAX_PER_TRACK
    from musicfpaugment_amd import ops
    assert ops.SEGMENT_MAX_PER_TRACK == so.MAX_PER_TRACK


@pytest.mark.parametrize("case", [([0, 3, 4, 9, 8], 4, 4), ([], 4, 4), ([8195], 4, 1), ([0, 23, 24, 25, 47, 127], 24, 24),
                                  ([0, 23, 24, 25, 47, 127], 24, 8), ([0, 23, 24, 25, 47, 127, 54, 53], 24, 30),
                                  ([10 ** 12], 10 ** 8, 130000000), ([1920000] * 5, 24000, 24000)], ids=str)
def test_geometry_against_the_oracle(lib, case):
    lengths, L, S = case
    rc, seg_off = _geometry(lib.lib(), lengths, L, S)
    assert rc == 0 and seg_off.tolist() == so.geometry(lengths, L, S).tolist()


def test_geometry_rejects(lib):
    h = lib.lib()
    for lengths, L, S in (([4], 0, 1), ([4], 1, 0), ([4], -3, 4), ([-1], 4, 4), ([8, -8], 4, 4), ([8196], 4, 1),
                          ([4], (1 << 27) + 1, 4), ([4], 4, (1 << 27) + 1),
                          ([8192] * 262145, 1, 1)):                      # 2^31 segments in all
        assert so.geometry(lengths, L, S) is None or L > 1 << 27 or S > 1 << 27
        assert _geometry(h, lengths, L, S)[0] == lib.EINVAL, (lengths[:2], L, S)
    assert _geometry(h, [8192] * 262143, 1, 1)[0] == 0                   # ... and just below
    buf = np.zeros(4, dtype=np.int32).ctypes.data_as(ctypes.c_void_p)
    lens = np.zeros(2, dtype=np.int64).ctypes.data_as(ctypes.c_void_p)
    assert h.mfpa_segment_geometry(None, 2, 4, 4, buf) == lib.EINVAL and h.mfpa_segment_geometry(lens, 2, 4, 4, None) == lib.EINVAL
    assert h.mfpa_segment_geometry(lens, -1, 4, 4, buf) == lib.EINVAL
    assert h.mfpa_segment_geometry(None, 0, 4, 4, buf) == 0              # no tracks: len is not read


@pytest.mark.parametrize("change", [dict(bank=None), dict(off=None), dict(len=None), dict(seg_off=None), dict(seg=None), dict(trk=None),
                                    dict(peak=None), dict(n=-1), dict(L=0), dict(S=0), dict(L=-24), dict(L=(1 << 27) + 1)], ids=str)
def test_stats_rejects_before_any_launch(lib, change):
    assert _stats(lib.lib(), **change) == lib.EINVAL


@pytest.mark.parametrize("change", [dict(seg=None), dict(trk=None), dict(peak=None), dict(off=None), dict(len=None), dict(seg_off=None),
                                    dict(keys=None), dict(sel=None), dict(src=None), dict(div=None), dict(kept=None), dict(n=-1),
                                    dict(n_keep=0), dict(n_keep=-2), dict(L=0), dict(S=0), dict(thr=-0.1), dict(thr=float("nan")),
                                    dict(n=1 << 20, n_keep=1 << 12)], ids=str)
def test_select_rejects_before_any_launch(lib, change):
    assert _select(lib.lib(), **change) == lib.EINVAL


@pytest.mark.parametrize("change", [dict(bank=None), dict(src=None), dict(out=None), dict(rows=-1), dict(rows=1 << 31), dict(L=0),
                                    dict(ldo=23), dict(L=(1 << 27) + 1, ldo=1 << 28)], ids=str)
def test_gather_rejects_before_any_launch(lib, change):
    assert _gather(lib.lib(), **change) == lib.EINVAL


def test_empty_calls_are_no_ops(lib):
    h = lib.lib()
    assert _stats(h, n=0) == 0 and _stats(h, n=0, bank=None, off=None, len=None, seg_off=None, seg=None, trk=None, peak=None) == 0
    assert _select(h, n=0) == 0 and _select(h, n=0, seg=None, keys=None, sel=None) == 0
    assert _gather(h, rows=0) == 0 and _gather(h, rows=0, bank=None, src=None, out=None) == 0
    assert _stats(h, n=0, L=0) == lib.EINVAL and _select(h, n=0, n_keep=0) == lib.EINVAL and _gather(h, rows=0, ldo=1) == lib.EINVAL


def test_no_cpu_fallback():
    import torch
    from musicfpaugment_amd import ops
    from musicfpaugment_amd._lib import MfpaError
    assert ops.segment_geometry([0, 3, 4, 9, 8], 4, 4).tolist() == [0, 0, 0, 1, 3, 5]
    assert ops.segment_geometry([0, 3, 4, 9, 8], 4, 4).dtype == np.int32
    with pytest.raises(ValueError):
        ops.segment_geometry([8196], 4, 1)
    assert abs(ops.segment_threshold() - so.threshold()) == 0 and abs(so.threshold() - np.exp(-1.5)) < 1e-16
    z64, z32 = torch.zeros(1, dtype=torch.int64), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(MfpaError):
        ops.segment_stats(torch.zeros(8), z64, z64, z32, 0, 4, 4)
    with pytest.raises(MfpaError):
        ops.segment_gather(torch.zeros(8), z64, None, 4)
