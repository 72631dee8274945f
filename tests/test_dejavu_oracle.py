"""CPU: the Dejavu identification oracle (tests/_dejavu_oracle.py) reproduces the reference's Postgres store,
return_matches, align_matches and FileRecognizer match rule (tests/golden/g15_dejavu_identify.npz, written by
tools/make_dejavu_identify_goldens.py), and the new C-ABI entry points reject bad arguments without touching a GPU."""
import ctypes
import os

import numpy as np
import pytest

from tests import _dejavu_oracle as do

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _split(a, n):
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    return [a[off[i]:off[i + 1]] for i in range(len(n))]


@pytest.fixture(scope="module")
def g15():
    return dict(np.load(os.path.join(GOLDEN, "g15_dejavu_identify.npz")))


@pytest.fixture(scope="module")
def table(g15):
    return do.store(g15["ins_dig"], g15["ins_sid"], g15["ins_off"])


def queries(g15):
    dig, off = _split(g15["q_dig"], g15["q_n"]), _split(g15["q_off"], g15["q_n"])
    return [list(zip([bytes(x) for x in d], o.tolist())) for d, o in zip(dig, off)]


def test_store_is_the_reference_set(g15, table):
    want = do.store(g15["fp_dig"], g15["fp_sid"], g15["fp_off"])
    assert len(g15["fp_sid"]) == table.shape[0] < len(g15["ins_sid"])          # duplicates were inserted and dropped
    np.testing.assert_array_equal(table, want)
    # an insertion order and a batching of their own give the same bytes
    perm = np.random.default_rng(0).permutation(len(g15["ins_sid"]))
    again = do.store(g15["ins_dig"][perm], g15["ins_sid"][perm], g15["ins_off"][perm])
    np.testing.assert_array_equal(again, table)


def test_return_matches_and_align_equal_the_reference(g15, table):
    idx = do.index(table)
    songs = {i + 1: int(t) for i, t in enumerate(g15["song_total"])}
    rm = list(zip(_split(g15["rm_sid"], g15["rm_n"]), _split(g15["rm_diff"], g15["rm_n"])))
    dd = list(zip(_split(g15["dd_sid"], g15["dd_n"]), _split(g15["dd_cnt"], g15["dd_n"])))
    tops = {t: (_split(g15[f"top{t}_int"], g15[f"top{t}_n"]), _split(g15[f"top{t}_float"], g15[f"top{t}_n"])) for t in (1, 3)}
    seen = set()
    for i, q in enumerate(queries(g15)):
        uniq = sorted({(d, t) for d, t in q})
        res, dedup = do.return_matches(idx, uniq)
        assert sorted(res) == list(zip(rm[i][0].tolist(), rm[i][1].tolist())), i
        assert sorted(dedup.items()) == list(zip(dd[i][0].tolist(), dd[i][1].tolist())), i
        rows, nq, match = do.recognize(idx, q)
        assert nq == int(g15["queried"][i]) and match == bool(g15["match"][i]), i
        for t in (1, 3):
            rows = do.align_matches(res, dedup, topn=t)
            ints, floats = do.report(rows, nq, songs)
            np.testing.assert_array_equal(ints, tops[t][0][i], err_msg=f"query {i} topn {t}")
            np.testing.assert_array_equal(floats, tops[t][1][i], err_msg=f"query {i} topn {t}")
        if rows:
            seen.add("negative diff" if rows[0][1] < 0 else "positive diff")
            if len(rows) > 1 and rows[1][2] < rows[0][4]:
                seen.add("topn quirk")
            if rows[0][4] == 1:
                seen.add("count 1")
        else:
            seen.add("no rows")
    assert {"negative diff", "positive diff", "topn quirk", "count 1", "no rows"} <= seen, seen


@pytest.fixture(scope="module")
def lib():
    from musicfpaugment_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from musicfpaugment_amd.csrc.build import build
        build(verbose=False)
    return _lib


def test_dejavu_entry_points_refuse_bad_arguments(lib):
    h = lib.lib()
    E = lib.EINVAL
    n = ctypes.c_longlong(0)
    assert h.mfpa_dejavu_match_scratch_bytes(100, 1 << 15, ctypes.addressof(n)) == 0 and n.value == 48 * 128 + 16 + 32 * (1 << 15)
    for cap, hcap in ((100, 63), (100, 100), (100, 1 << 27), (-1, 1 << 15), ((1 << 24) + 1, 1 << 15)):
        assert h.mfpa_dejavu_match_scratch_bytes(cap, hcap, ctypes.addressof(n)) == E, (cap, hcap)
    assert h.mfpa_dejavu_match_scratch_bytes(100, 1 << 15, None) == E
    # table, directory, dirbits, digests, t1, nq, B, cap, hcap, scratch, K, out, info, stream
    assert h.mfpa_dejavu_match(1, 1, 20, 1, 1, 1, 4, 16, 1 << 15, 1, 0, 1, 1, None) == E          # K < 1
    assert h.mfpa_dejavu_match(1, 1, 20, 1, 1, 1, 4, 16, 1000, 1, 1, 1, 1, None) == E             # hcap not a power of two
    assert h.mfpa_dejavu_match(1, 1, 20, 1, 1, 1, 4, 16, 32, 1, 1, 1, 1, None) == E               # hcap < 64
    assert h.mfpa_dejavu_match(1, 1, 0, 1, 1, 1, 4, 16, 1 << 15, 1, 1, 1, 1, None) == E           # dirbits
    assert h.mfpa_dejavu_match(1, 1, 25, 1, 1, 1, 4, 16, 1 << 15, 1, 1, 1, 1, None) == E
    assert h.mfpa_dejavu_match(None, 1, 20, 1, 1, 1, 4, 16, 1 << 15, 1, 1, 1, 1, None) == E       # null pointers
    assert h.mfpa_dejavu_match(1, 1, 20, 1, 1, 1, 4, 16, 1 << 15, None, 1, 1, 1, None) == E
    assert h.mfpa_dejavu_match(1, 1, 20, 1, 1, 1, -1, 16, 1 << 15, 1, 1, 1, 1, None) == E         # B < 0
    assert h.mfpa_dejavu_match(None, None, 20, None, None, None, 0, 16, 1 << 15, None, 1, None, None, None) == 0   # empty batch
    # digests, sids, offsets, order, n, dirbits, work, table, n_rows, directory, stream
    assert h.mfpa_dejavu_store(1, 1, 1, 1, 10, 0, 1, 1, 1, 1, None) == E                          # dirbits
    assert h.mfpa_dejavu_store(1, 1, 1, 1, -1, 20, 1, 1, 1, 1, None) == E                         # n < 0
    assert h.mfpa_dejavu_store(None, 1, 1, 1, 10, 20, 1, 1, 1, 1, None) == E                      # null rows with n > 0
    assert h.mfpa_dejavu_store(1, 1, 1, 1, 10, 20, None, 1, 1, 1, None) == E                      # null work
    assert h.mfpa_dejavu_store(1, 1, 1, 1, 10, 20, 1, 1, None, 1, None) == E                      # null n_rows
    assert h.mfpa_dejavu_lookup(1, 1, 20, None, 4, 1, None) == E
    assert h.mfpa_dejavu_lookup(1, 1, 30, 1, 4, 1, None) == E
    assert h.mfpa_dejavu_lookup(1, 1, 20, 1, -1, 1, None) == E
    assert h.mfpa_dejavu_lookup(None, None, 20, None, 0, None, None) == 0
