#!/usr/bin/env python3
"""Generate tests/golden/g18_maintain.npz with the REAL reference's HashTable.remove and HashTable.retrieve
(afp/audfprint/hash_table.py:277-316) on tiny tables.  Build-container only, like tools/make_identify_goldens.py, whose
import_reference() it reuses; the class is loaded from the reference tree at run time and only numbers go into the repository.

The reference object is made with __new__ and its hashbits, depth, maxtimebits, table and counts are set by hand, so the class
works on tables of a few buckets.  Each case's table is laid out slot by slot:

    bucket 0   full and overfull; matches at slot 0 and 1 (adjacent), at the last valid slot, one id at slots 63 and 64 and one at
               127 and 128 (across the rounds of 64) where the depth has them; a stored time with every time bit set
    bucket 1   full and overfull, holding two ids only: the first removal hits it, the second empties it
    bucket 2   full and overfull, ids that stay: never hit, its count above depth survives
    bucket 3   three entries of one id: emptied by one removal
    bucket 4   65 entries, one id at its last two slots 63 and 64 (depth > 64)
    others     mostly a few entries, some empty, some full or overfull
and then the reference's own store adds two tracks whose times lie above the time mask (random.seed fixed: a full bucket
takes the reservoir draw from Python's `random`).  Buckets 2..4 exist from hashbits 3 on.

Five ids are removed one after the other (id 0, id n_ids - 1, one in the middle, the two of bucket 1), one of them by its
integer id.  Recorded per case: table, counts, names and hashesperid before and after all removals, SHA-256 of the table and
counts after each single removal, the counts the reference printed, retrieve() of every id before and after.

Usage:  python tools/make_maintain_goldens.py
"""
from __future__ import annotations

import contextlib
import hashlib
import io
import os
import random
import re
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from make_goldens import OUT, import_reference  # noqa: E402
from tests import _maintain_oracle as mo  # noqa: E402

# (hashbits, depth, timebits, n_ids)
CASES = [(6, 4, 14, 12), (8, 100, 14, 12), (7, 130, 14, 12), (1, 100, 14, 12), (6, 100, 20, 2048)]
WANTED = {"overfull_hit", "overfull_not_hit", "emptied", "slot0", "last_valid", "adjacent"}


def name_of(i: int) -> str:
    return "trk%04d" % i


def digest(a, dt) -> np.ndarray:
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, dt).tobytes()).digest(), np.uint8)


def lay_out(hashbits, depth, timebits, n_ids, rng):
    nb, D, mask = 1 << hashbits, depth, (1 << timebits) - 1
    A, Z, M, X, Y = 0, n_ids - 1, n_ids // 2, 1, 2
    stay = np.array([i for i in (3, 4, 5, 7, 8, n_ids - 2, n_ids - 3) if i not in (A, Z, M, X, Y)])
    table = np.zeros((nb, D), np.uint32)
    counts = np.zeros(nb, np.int32)

    def val(ids, times):
        return (((np.asarray(ids, np.int64) + 1) << timebits) | (np.asarray(times, np.int64) & mask)).astype(np.uint32)

    def fill(b, ids, extra=0):
        ids = np.asarray(ids, np.int64)
        table[b, : ids.size] = val(ids, rng.integers(0, mask + 1, ids.size))
        counts[b] = ids.size + extra

    mixed = np.concatenate([stay, stay, [A, Z, M]])
    row0 = rng.choice(mixed, D)
    row0[0] = A
    if D > 1:
        row0[1] = A
    row0[D - 1] = Z
    if D > 64:
        row0[63], row0[64] = A, A
    if D > 128:
        row0[127], row0[128] = M, M
    fill(0, row0, extra=7)
    table[0, 0] = val(A, mask)
    row1 = rng.choice([X, Y], D)
    row1[0], row1[D - 1] = X, Y
    fill(1, row1, extra=3)
    free = 2
    if nb >= 8:
        fill(2, rng.choice(stay, D), extra=11)
        fill(3, [A] * min(D, 3))
        if D > 64:
            r = rng.choice(stay, 65)
            r[63], r[64] = Z, Z
            fill(4, r)
        free = 5
    for b in range(free, nb):
        u = rng.random()
        n = 0 if u < 0.25 else D if u > 0.9 else int(min(D, rng.geometric(0.2)))
        fill(b, rng.choice(mixed, n), extra=int(rng.integers(1, 9)) if n == D and rng.random() < 0.5 else 0)
    hpid = np.zeros(n_ids, np.uint32)
    ids_in = (table[table != 0].astype(np.int64) >> timebits) - 1
    hpid += np.bincount(ids_in, minlength=n_ids).astype(np.uint32)
    hpid[hpid > 0] += (np.arange(n_ids)[hpid > 0] % 3).astype(np.uint32)          # as if the reservoir had dropped some
    return table, counts, hpid, (A, Z, M, X, Y), free


def main():
    import_reference()
    from afp.audfprint.hash_table import HT_VERSION, HashTable

    rng = np.random.default_rng(18)
    random.seed(1818)
    out = {"n_cases": np.int64(len(CASES))}
    for ci, (hashbits, depth, timebits, n_ids) in enumerate(CASES):
        nb, mask = 1 << hashbits, (1 << timebits) - 1
        table, counts, hpid, (A, Z, M, X, Y), free = lay_out(hashbits, depth, timebits, n_ids, rng)
        ht = HashTable.__new__(HashTable)
        ht.hashbits, ht.depth, ht.maxtimebits = hashbits, depth, timebits
        ht.table, ht.counts = table, counts
        ht.names = [name_of(i) for i in range(n_ids)]
        ht.hashesperid = hpid
        ht.ht_version, ht.dirty = HT_VERSION, False
        # the reference's own store: times above the time mask, hashes above the hash mask, into bucket 0 (full: the
        # reservoir draw) and the free buckets -- never buckets 1..4, whose ids are fixed above
        allowed = np.array([0] + list(range(free, nb)))
        for id_ in (3, M):
            n = 40
            rows = np.stack([rng.integers(mask + 1, 4 * (mask + 1), n),
                             rng.choice(allowed, n) + nb * rng.integers(0, 8, n)], 1).astype(np.int32)
            ht.store(name_of(id_), rows)
        # the slots the draw may have taken in bucket 0 are laid out again
        forced = [(0, A), (1, A), (depth - 1, Z)] + ([(63, A), (64, A)] if depth > 64 else []) + \
                 ([(127, M), (128, M)] if depth > 128 else [])
        for j, id_ in forced:
            if j < depth:
                ht.table[0, j] = np.uint32(((id_ + 1) << timebits) | (mask if j == 0 else int(rng.integers(0, mask + 1))))
        assert mo.invariant_holds(ht.table, ht.counts)
        order = [X, Y, A, Z, M]
        by_int = {Z}

        table0, counts0 = ht.table.copy(), ht.counts.copy()
        names0, hpid0 = list(ht.names), np.asarray(ht.hashesperid).astype(np.uint32)
        ret0 = [np.asarray(ht.retrieve(i), np.int32).reshape(-1, 2) for i in range(n_ids)]

        seen, printed, step_t, step_c = set(), [], [], []
        for id_ in order:
            seen |= mo.features(ht.table, ht.counts, [id_], timebits)
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                ht.remove(id_ if id_ in by_int else name_of(id_))
            m = re.fullmatch(r"Removed (\S+) \( (\d+) hashes\)\.\n", buf.getvalue())
            assert m and m.group(1) == (str(id_) if id_ in by_int else name_of(id_)), buf.getvalue()
            printed.append(int(m.group(2)))
            step_t.append(digest(ht.table, "<u4"))
            step_c.append(digest(ht.counts, "<i4"))
        want = set(WANTED) | ({"slots_63_64"} if depth > 64 else set()) | ({"top_bit"} if (n_ids << timebits) >= 1 << 31 else set())
        assert want <= seen, (ci, want - seen)
        assert mo.invariant_holds(ht.table, ht.counts) and ht.dirty
        if nb >= 8:
            assert int(ht.counts[2]) > depth                                   # a count above depth survives where nothing matched
        ret1 = [np.asarray(ht.retrieve(i), np.int32).reshape(-1, 2) for i in range(n_ids)]
        assert all(len(ret1[i]) == 0 for i in order) and ht.names[Z] is None

        cat = lambda xs: np.concatenate(xs).astype(np.int32).reshape(-1, 2)
        off = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
        p = "c%d_" % ci
        out.update({
            p + "shape": np.array([hashbits, depth, timebits, n_ids], np.int64),
            p + "table0": table0.astype(np.uint32), p + "counts0": counts0.astype(np.int32),
            p + "names0": np.array(names0, dtype=str), p + "hpid0": hpid0,
            p + "order": np.array(order, np.int64), p + "by_int": np.array([i in by_int for i in order]),
            p + "printed": np.array(printed, np.int64),
            p + "step_table_sha256": np.stack(step_t), p + "step_counts_sha256": np.stack(step_c),
            p + "table1": ht.table.astype(np.uint32), p + "counts1": ht.counts.astype(np.int32),
            p + "names1": np.array(["" if n is None else n for n in ht.names], dtype=str),
            p + "names1_none": np.array([n is None for n in ht.names]),
            p + "hpid1": np.asarray(ht.hashesperid).astype(np.uint32),
            p + "ret0_rows": cat(ret0), p + "ret0_off": off(ret0), p + "ret1_rows": cat(ret1), p + "ret1_off": off(ret1),
        })
        print(f"case {ci}: hashbits {hashbits} depth {depth} timebits {timebits}: {int(np.count_nonzero(table0))} entries, "
              f"removed {printed}, features {sorted(seen)}")
    path = os.path.join(OUT, "g18_maintain.npz")
    np.savez_compressed(path, **out)
    print(f"g18_maintain.npz {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
