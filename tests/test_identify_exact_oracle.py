"""CPU: the oracle of the matcher's extended modes (tests/_identify_exact_oracle.py) reproduces the reference's Matcher with
exact_count / find_time_range / hashesfor (tests/golden/g15_identify_exact.npz, written by
tools/make_identify_exact_goldens.py)."""
import hashlib
import os

import numpy as np
import pytest

from tests import _identify_exact_oracle as xo
from tests import _identify_oracle as io_

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
COMBOS = {"ff": (False, False), "ft": (False, True), "tf": (True, False), "tt": (True, True)}


def _split(rows, off):
    return [rows[off[i]:off[i + 1]] for i in range(len(off) - 1)]


@pytest.fixture(scope="module")
def g15():
    return dict(np.load(os.path.join(GOLDEN, "g15_identify_exact.npz")))


@pytest.fixture(scope="module")
def oracle_db(g15):
    g14 = np.load(os.path.join(GOLDEN, "g14_identify.npz"))
    table, counts = io_.empty_table()
    hpid = []
    for i, tr in enumerate(_split(g14["track_rows"], g14["track_off"]) + _split(g15["extra_track_rows"], g15["extra_track_off"])):
        hpid.append(io_.store(table, counts, tr, i))
    return table, counts, np.array(hpid, np.uint32)


def _sha256(a, dt):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, dt).tobytes()).digest(), np.uint8)


def test_table_is_g14s_plus_four_tracks(g15, oracle_db):
    table, counts, hpid = oracle_db
    np.testing.assert_array_equal(_sha256(table, "<u4"), g15["table_sha256"])
    np.testing.assert_array_equal(_sha256(counts, "<i4"), g15["counts_sha256"])
    np.testing.assert_array_equal(hpid, g15["hashesperid"])
    assert len(hpid) == 304 and counts.max() <= io_.DEPTH


@pytest.mark.parametrize("key", list(COMBOS))
def test_rows_match_reference(g15, oracle_db, key):
    ex, tr = COMBOS[key]
    queries = _split(g15["query_rows"], g15["query_off"])
    for qi, (q, want) in enumerate(zip(queries, _split(g15["rows_" + key], g15["off_" + key]))):
        got, _ = xo.match(*oracle_db, q, exact_count=ex, find_time_range=tr)
        err = xo.rows_equivalent(got, want, xo.rank_ties(*oracle_db, q))
        assert err is None, f"{key} query {qi}: {err}"
        if key == "ff":
            np.testing.assert_array_equal(got, io_.match(*oracle_db, q))
    assert sum(len(q) and int(q[:, 0].min()) < 0 for q in queries) >= 9                 # negative query times are covered


def test_exact_and_approximate_differ_where_they_should(g15):
    names = g15["query_names"].tolist()
    first = int(g15["first_new_query"])
    row = lambda key, name, id_: [r for r in _split(g15["rows_" + key], g15["off_" + key])[first + names.index(name)].tolist()
                                  if r[0] == id_]
    assert (row("ff", "double", 300)[0][1], row("tf", "double", 300)[0][1]) == (52, 40)   # one query row, two hits in one window
    assert sorted(r[2] for r in row("tf", "two_maxima", 301)) == [50, 52]                 # two maxima two bins apart
    assert (row("ff", "pow2", 302)[0][1], row("tf", "pow2", 302)[0][1]) == (20, 19)       # times 0 and 2^10 pack to one value
    assert (row("ff", "high_bits", 302)[0][1], row("tf", "high_bits", 302)[0][1]) == (18, 12)


@pytest.mark.parametrize("key", list(COMBOS))
def test_threshcount_one_matches_reference(g15, oracle_db, key):
    ex, tr = COMBOS[key]
    queries = _split(g15["query_rows"], g15["query_off"])
    for qi, want in zip(g15["t1_queries"], _split(g15["t1_rows_" + key], g15["t1_off_" + key])):
        got, _ = xo.match(*oracle_db, queries[qi], threshcount=1, exact_count=ex, find_time_range=tr)
        err = xo.rows_equivalent(got, want, xo.rank_ties(*oracle_db, queries[qi]))
        assert err is None, f"{key} query {qi}: {err}"
    if key == "tt":                                                                         # windows of one hit: match_times[-1]
        one = [r for r in _split(g15["t1_rows_tt"], g15["t1_off_tt"])[0].tolist() if r[0] == 303]
        assert len(one) == 2 and all(r[1] == 1 and r[5] == r[6] for r in one)


@pytest.mark.parametrize("tag,quantile", [("q0", 0.0), ("q25", 0.25)])
def test_other_quantiles_match_reference(g15, oracle_db, tag, quantile):
    queries = _split(g15["query_rows"], g15["query_off"])
    for key in ("ft", "tt"):
        for qi, want in zip(g15["quantile_queries"], _split(g15[f"{tag}_rows_{key}"], g15[f"{tag}_off_{key}"])):
            got, _ = xo.match(*oracle_db, queries[qi], exact_count=COMBOS[key][0], find_time_range=True, time_quantile=quantile)
            err = xo.rows_equivalent(got, want, xo.rank_ties(*oracle_db, queries[qi]))
            assert err is None, f"{tag} {key} query {qi}: {err}"


def test_hash_lists_match_reference(g15, oracle_db):
    queries = _split(g15["query_rows"], g15["query_off"])
    lists = _split(g15["hf_rows"], g15["hf_off"])
    assert len(lists) == len(g15["hf_spec"]) >= 20
    for (qi, ex, k), want in zip(g15["hf_spec"].tolist(), lists):
        _, got = xo.match(*oracle_db, queries[qi], exact_count=bool(ex), hashesfor=k)
        np.testing.assert_array_equal(got, want, err_msg=f"query {qi} exact {ex} row {k}")   # sorted and unique: the order is determined
    with pytest.raises(IndexError):
        xo.match(*oracle_db, queries[0], hashesfor=10 ** 6)


def test_exact_count_rejects_threshcount_below_one(oracle_db, g15):
    with pytest.raises(ValueError):
        xo.match(*oracle_db, _split(g15["query_rows"], g15["query_off"])[0], threshcount=0, exact_count=True)


def test_pow2_roundup_mask_is_numpys():
    """The mask the host hands to the kernel: encpowerof2(2^k) - k for k < 32; for every other value the integer formula holds."""
    from musicfpaugment_amd import ops
    mask = ops.pow2_roundup_mask()
    for k in range(31):
        assert xo.encpowerof2(1 << k) == k + ((mask >> k) & 1), k
    for v in list(range(1, 5000)) + [(1 << k) + d for k in range(2, 31) for d in (-1, 1)]:
        if v & (v - 1):
            assert xo.encpowerof2(v) == v.bit_length(), v
