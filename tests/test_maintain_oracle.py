"""CPU: the maintenance oracle (tests/_maintain_oracle.py) reproduces the reference's HashTable.remove and HashTable.retrieve
bit for bit on tests/golden/g18_maintain.npz (written by tools/make_maintain_goldens.py with the reference's own class), both
one id after the other and as a set in one pass."""
import hashlib

import numpy as np
import pytest

from tests import _maintain_oracle as mo

CASES = mo.CASES


def sha(a, dt):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, dt).tobytes()).digest(), np.uint8)


@pytest.fixture(scope="module", params=range(len(CASES)), ids=lambda i: "h%d_d%d_t%d" % CASES[i])
def case(request):
    c = mo.load_case(request.param)
    assert tuple(c["shape"][:3]) == CASES[request.param]
    return c


def test_fixture_holds_the_cases_the_issue_names(case):
    hashbits, depth, timebits, n_ids = (int(v) for v in case["shape"])
    assert case["table0"].shape == (1 << hashbits, depth) and case["table0"].dtype == np.uint32
    assert mo.invariant_holds(case["table0"], case["counts0"]) and mo.invariant_holds(case["table1"], case["counts1"])
    order = case["order"].tolist()
    assert 0 in order and n_ids - 1 in order and case["by_int"].any()
    t, c = case["table0"].copy(), case["counts0"].copy()
    seen = set()
    for id_ in order:
        seen |= mo.features(t, c, [id_], timebits)
        mo.remove(t, c, [id_], n_ids, timebits)
    want = {"overfull_hit", "overfull_not_hit", "emptied", "slot0", "last_valid", "adjacent"}
    if depth > 64:
        want.add("slots_63_64")
    if timebits == 20:
        want.add("top_bit")                                        # id 2047: (id + 1) << 20 = 2^31
        assert n_ids == 2048 and case["table0"].max() >= 1 << 31
    assert want <= seen, want - seen
    assert np.any((case["table0"] & ((1 << timebits) - 1)) == (1 << timebits) - 1)      # a time with every bit set


def test_remove_one_id_after_the_other(case):
    hashbits, depth, timebits, n_ids = (int(v) for v in case["shape"])
    t, c = case["table0"].copy(), case["counts0"].copy()
    for k, id_ in enumerate(case["order"].tolist()):
        removed = mo.remove(t, c, [id_], n_ids, timebits)
        assert int(removed[id_]) == int(case["printed"][k]) and int(removed.sum()) == int(removed[id_])
        assert np.array_equal(sha(t, "<u4"), case["step_table_sha256"][k]), k
        assert np.array_equal(sha(c, "<i4"), case["step_counts_sha256"][k]), k
    assert np.array_equal(t, case["table1"]) and np.array_equal(c, case["counts1"])


@pytest.mark.parametrize("flip", [False, True], ids=["set", "set_reversed"])
def test_remove_the_set_in_one_pass(case, flip):
    hashbits, depth, timebits, n_ids = (int(v) for v in case["shape"])
    t, c = case["table0"].copy(), case["counts0"].copy()
    order = case["order"].tolist()
    removed = mo.remove(t, c, order[::-1] if flip else order, n_ids, timebits)
    assert np.array_equal(t, case["table1"]) and np.array_equal(c, case["counts1"])
    assert removed[order].tolist() == case["printed"].tolist() and int(removed.sum()) == int(case["printed"].sum())


def test_retrieve_before_and_after(case):
    hashbits, depth, timebits, n_ids = (int(v) for v in case["shape"])
    for tab, cnt, rows, off in ((case["table0"], case["counts0"], case["ret0_rows"], case["ret0_off"]),
                                (case["table1"], case["counts1"], case["ret1_rows"], case["ret1_off"])):
        ids = list(range(n_ids)) if n_ids <= 64 else [0, 1, 2, 3, n_ids // 2, n_ids - 3, n_ids - 2, n_ids - 1]
        for i in ids:
            got = mo.retrieve(tab, cnt, i, timebits)
            assert got.dtype == np.int32 and np.array_equal(got, rows[off[i]:off[i + 1]]), i
        got_rows, got_off = mo.retrieve_batch(tab, cnt, ids[::-1], timebits)
        want = [rows[off[i]:off[i + 1]] for i in ids[::-1]]
        assert np.array_equal(got_rows, np.concatenate(want)) and got_off.tolist() == np.cumsum([0] + [len(w) for w in want]).tolist()
        stored = np.unique((tab[tab != 0].astype(np.int64) >> timebits) - 1)    # every other id holds nothing, in the fixture too
        assert np.array_equal(stored, np.flatnonzero(np.diff(off)))
    for id_ in case["order"].tolist():
        assert case["ret1_off"][id_] == case["ret1_off"][id_ + 1]
    names1 = [None if gone else str(n) for n, gone in zip(case["names1"], case["names1_none"])]
    assert [i for i, n in enumerate(names1) if n is None] == sorted(case["order"].tolist())
    assert not case["hpid1"][case["order"]].any()
    keep = np.setdiff1d(np.arange(n_ids), case["order"])
    assert np.array_equal(case["hpid1"][keep], case["hpid0"][keep])
