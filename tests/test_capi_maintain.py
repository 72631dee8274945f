"""CPU: the hash-table maintenance entry points (mfpa_audfprint_remove, mfpa_audfprint_retrieve_count, mfpa_audfprint_retrieve,
mfpa_audfprint_retrieve_work_ints) through ctypes.  Arguments are checked on the host before any launch and pointers are never
dereferenced, so this runs without a GPU (the style of tests/test_capi_track.py)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mfpa_audfprint_remove", "mfpa_audfprint_retrieve", "mfpa_audfprint_retrieve_count", "mfpa_audfprint_retrieve_work_ints")


@pytest.fixture(scope="module")
def lib():
    from musicfpaugment_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from musicfpaugment_amd.csrc.build import build
        build(verbose=False)
    return _lib


def _remove(h, **kw):
    a = dict(table=8, counts=8, hashbits=20, timebits=14, depth=100, in_set=8, n_ids=4, flags=0, removed=8, stream=None)
    a.update(kw)
    return h.mfpa_audfprint_remove(a["table"], a["counts"], a["hashbits"], a["timebits"], a["depth"], a["in_set"], a["n_ids"],
                                   a["flags"], a["removed"], a["stream"])


def _retrieve_args(kw):
    a = dict(table=8, counts=8, hashbits=20, timebits=14, depth=100, rank=8, n_ids=4, K=2, flags=0, work=8, offsets=8, rows=8,
             n_rows=5, stream=None)
    a.update(kw)
    return a


def _count(h, **kw):
    a = _retrieve_args(kw)
    return h.mfpa_audfprint_retrieve_count(a["table"], a["counts"], a["hashbits"], a["timebits"], a["depth"], a["rank"], a["n_ids"],
                                           a["K"], a["flags"], a["work"], a["offsets"], a["stream"])


def _retrieve(h, **kw):
    a = _retrieve_args(kw)
    return h.mfpa_audfprint_retrieve(a["table"], a["counts"], a["hashbits"], a["timebits"], a["depth"], a["rank"], a["n_ids"],
                                     a["K"], a["flags"], a["work"], a["offsets"], a["rows"], a["n_rows"], a["stream"])


def test_symbols_header_and_abi_version(lib):
    h = lib.lib()
    header = open(os.path.join(ROOT, "include", "mfpa.h")).read()
    declared = set(re.findall(r"^int\s+(mfpa_\w+)\s*\(", header, flags=re.M))
    for name in NEW:
        assert name in lib.exported_symbols() and name in declared and hasattr(h, name), name
    assert lib.ABI_VERSION == 47 and h.mfpa_version() == 47              # the new symbols are additive
    assert int(re.search(r"#define MFPA_MAINTAIN_FULL_ROWS (\d+)", header).group(1)) == 1
    from musicfpaugment_amd import ops
    assert ops.MAINTAIN_FULL_ROWS == 1


BAD_TABLE = [dict(hashbits=0), dict(hashbits=25), dict(depth=0), dict(depth=4097), dict(timebits=0), dict(timebits=21),
             dict(table=None), dict(counts=None), dict(flags=2), dict(flags=-1)]


@pytest.mark.parametrize("change", BAD_TABLE + [dict(n_ids=-1), dict(in_set=None), dict(removed=None)], ids=str)
def test_remove_rejects(lib, change):
    assert _remove(lib.lib(), **change) == lib.EINVAL


@pytest.mark.parametrize("change", BAD_TABLE + [dict(K=-1), dict(n_ids=-1), dict(K=5), dict(rank=None), dict(work=None),
                                                dict(offsets=None), dict(hashbits=24, depth=128)], ids=str)
def test_retrieve_rejects(lib, change):
    h = lib.lib()
    assert _count(h, **change) == lib.EINVAL
    assert _retrieve(h, **change) == lib.EINVAL


def test_retrieve_scatter_rejects_its_own_arguments(lib):
    h = lib.lib()
    assert _retrieve(h, rows=None) == lib.EINVAL and _retrieve(h, n_rows=-1) == lib.EINVAL


def test_empty_calls_are_no_ops(lib):
    h = lib.lib()
    assert _remove(h, n_ids=0) == 0 and _remove(h, n_ids=0, table=None, counts=None, in_set=None, removed=None) == 0
    assert _count(h, K=0) == 0 and _count(h, K=0, table=None, rank=None, work=None, offsets=None) == 0
    assert _retrieve(h, K=0) == 0 and _retrieve(h, K=0, table=None, rows=None) == 0
    assert _retrieve(h, n_rows=0, rows=None) == 0                        # nothing to write
    # ... but a bad shape is still an error
    assert _remove(h, n_ids=0, depth=0) == lib.EINVAL and _count(h, K=0, hashbits=0) == lib.EINVAL


def test_work_ints_is_host_arithmetic(lib):
    h = lib.lib()
    n = ctypes.c_longlong(-1)
    assert h.mfpa_audfprint_retrieve_work_ints(20, 0, ctypes.addressof(n)) == 0 and n.value == 0
    assert h.mfpa_audfprint_retrieve_work_ints(20, 1, ctypes.addressof(n)) == 0 and n.value == 4096
    assert h.mfpa_audfprint_retrieve_work_ints(1, 3, ctypes.addressof(n)) == 0 and n.value == 3 * 2       # never more chunks than buckets
    assert h.mfpa_audfprint_retrieve_work_ints(20, 1 << 18, ctypes.addressof(n)) == 0 and (1 << 18) <= n.value <= 1 << 22
    for bad in ((0, 1), (25, 1), (20, -1)):
        assert h.mfpa_audfprint_retrieve_work_ints(bad[0], bad[1], ctypes.addressof(n)) == lib.EINVAL
    assert h.mfpa_audfprint_retrieve_work_ints(20, 1, None) == lib.EINVAL


def test_no_cpu_fallback(lib):
    """The wrappers and HashTable's maintenance methods refuse tables that are not on the GPU; the bad-argument checks of the
    wrappers come before any device work."""
    import numpy as np
    import torch
    from musicfpaugment_amd import ops
    from musicfpaugment_amd._lib import MfpaError
    from musicfpaugment_amd.afp.audfprint.hash_table import HashTable
    table, counts = torch.zeros((4, 3), dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(MfpaError):
        ops.audfprint_remove(table, counts, [0], 1)
    with pytest.raises(MfpaError):
        ops.audfprint_retrieve(table, counts, [0])
    ht = HashTable.__new__(HashTable)
    ht.device, ht.seed, ht._hpid_dev = torch.device("cpu"), 0, None
    ht.hashbits, ht.depth, ht.maxtimebits = 2, 3, 14
    ht.table, ht.counts = table, counts
    ht.names, ht.hashesperid, ht.dirty = ["a", "b"], np.zeros(2, np.uint32), False
    for call in (lambda: ht.remove("a"), lambda: ht.remove_batch(["a", "b"]), lambda: ht.retrieve("a"),
                 lambda: ht.retrieve_batch(["a"])):
        with pytest.raises(MfpaError):
            call()
    assert ht.names == ["a", "b"] and ht.dirty is False                   # nothing was marked removed
    with pytest.raises(ValueError, match="not found"):
        ht.remove("zzz")
    with pytest.raises(ValueError, match="not found"):
        ht.retrieve("zzz")
    with pytest.raises(IndexError):
        ht.remove(2)
