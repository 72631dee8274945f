"""CPU: the identification oracle (tests/_identify_oracle.py) reproduces the reference's HashTable.store and
Matcher.match_hashes (tests/golden/g14_identify.npz, written by tools/make_identify_goldens.py), and the new C-ABI entry
points reject bad arguments without touching a GPU."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

from tests import _identify_oracle as io_

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _split(rows, off):
    return [rows[off[i]:off[i + 1]] for i in range(len(off) - 1)]


@pytest.fixture(scope="module")
def g14():
    return dict(np.load(os.path.join(GOLDEN, "g14_identify.npz")))


@pytest.fixture(scope="module")
def oracle_db(g14):
    table, counts = io_.empty_table()
    hpid = []
    for i, tr in enumerate(_split(g14["track_rows"], g14["track_off"])):
        hpid.append(io_.store(table, counts, tr, i))
    return table, counts, np.array(hpid, np.uint32)


def _sha256(a, dt):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, dt).tobytes()).digest(), np.uint8)


def test_store_matches_reference(g14, oracle_db):
    """The reference's table and counts are pinned bit for bit by SHA-256 digests of their bytes."""
    table, counts, hpid = oracle_db
    assert int(counts.sum()) == int(g14["n_entries"]) and np.count_nonzero(counts) == int(g14["n_buckets"])
    np.testing.assert_array_equal(_sha256(counts, "<i4"), g14["counts_sha256"])
    np.testing.assert_array_equal(_sha256(table, "<u4"), g14["table_sha256"])
    np.testing.assert_array_equal(hpid, g14["hashesperid"])
    assert counts.max() <= io_.DEPTH and np.count_nonzero(counts >= 90) >= 20      # buckets close to, not over, depth


def test_store_matches_reference_small_table(g14):
    """The table of the reference-written g14_hashtable.pklz (hashbits 12, depth 8), rebuilt by the oracle."""
    table, counts = io_.empty_table(hashbits=12, depth=8)
    tracks = _split(g14["track_rows"], g14["track_off"])
    hpid = [io_.store(table, counts, tracks[i], k) for k, i in enumerate(range(150, 170))]
    np.testing.assert_array_equal(table, g14["small_table"])
    np.testing.assert_array_equal(counts, g14["small_counts"])
    np.testing.assert_array_equal(np.array(hpid, np.uint32), g14["small_hashesperid"])


def test_match_matches_reference(g14, oracle_db):
    table, counts, hpid = oracle_db
    queries = _split(g14["query_rows"], g14["query_off"])
    results = _split(g14["result_rows"], g14["result_off"])
    many = 0
    for qi, (q, want) in enumerate(zip(queries, results)):
        got = io_.match(table, counts, hpid, q)
        err = io_.rows_equivalent(got, want, io_.rank_ties(table, counts, hpid, q))
        assert err is None, f"query {qi}: {err}"
        many += want.shape[0] > 0 and int(want[:, 4].max()) >= 99
    assert many >= 1                                                                  # search_depth reached
    assert any(len(q) == 0 for q in queries) and any(len(r) == 0 and len(q) > 0 for q, r in zip(queries, results))


def test_overflow_counts_match_reference(g14):
    table, counts = io_.empty_table()
    hpid = [io_.store(table, counts, tr, i, seed=7) for i, tr in enumerate(_split(g14["ovf_rows"], g14["ovf_off"]))]
    np.testing.assert_array_equal(np.flatnonzero(counts), g14["ovf_counts_idx"])
    np.testing.assert_array_equal(counts[counts != 0], g14["ovf_counts_val"])
    np.testing.assert_array_equal(np.array(hpid, np.uint32), g14["ovf_hashesperid"])
    assert counts.max() > io_.DEPTH
    for b in np.flatnonzero(counts):                                                  # every stored value from a row of that bucket
        vals = table[b, :min(io_.DEPTH, counts[b])]
        assert np.all(vals >> 14 >= 1)


def test_reservoir_slot_is_uniform():
    c = 399
    slots = np.array([io_.reservoir_slot(3, b, c) for b in range(20000)])
    assert slots.min() >= 0 and slots.max() <= c
    assert abs(np.mean(slots < 100) - 100 / 400) < 0.02


def test_identify_entry_points_reject_bad_arguments():
    from musicfpaugment_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from musicfpaugment_amd.csrc.build import build
        build(verbose=False)
    h = _lib.lib()
    E = _lib.EINVAL
    n = ctypes.c_longlong(0)
    assert h.mfpa_audfprint_match_scratch_bytes(1 << 15, ctypes.addressof(n)) == 0 and n.value == 32 << 15
    assert h.mfpa_audfprint_match_scratch_bytes(1000, ctypes.addressof(n)) == E                     # not a power of two
    assert h.mfpa_audfprint_match_scratch_bytes(1 << 15, None) == E
    assert h.mfpa_audfprint_store(1, 1, 1, 1, 1, 20, 14, 0, 0, 1, 1, None) == E                       # depth 0
    assert h.mfpa_audfprint_store(1, 1, 1, 1, 1, 30, 14, 100, 0, 1, 1, None) == E                     # hashbits
    assert h.mfpa_audfprint_store(None, 1, 1, 1, 1, 20, 14, 100, 0, 1, 1, None) == E
    assert h.mfpa_audfprint_store(None, None, None, None, 0, 20, 14, 100, 0, None, None, None) == 0   # nothing to store
    args = [1, 1, 1, 10, 20, 14, 100, 1, 1, 4, 64, 5, 100, 2, 100, 1 << 15, 1, 1, 1, 1, None]
    bad = {"search_depth": (12, 257), "window": (13, -1), "K": (17, 0), "hcap": (15, 3000), "cap": (10, -1),
           "thresh": (11, -1), "depth": (6, 0)}
    for name, (i, v) in bad.items():
        a = list(args)
        a[i] = v
        assert h.mfpa_audfprint_match(*a) == E, name
    a = list(args)
    a[16] = None                                                                                       # scratch
    assert h.mfpa_audfprint_match(*a) == E
    a = list(args)
    a[9] = 0                                                                                           # empty batch
    assert h.mfpa_audfprint_match(*a) == 0
