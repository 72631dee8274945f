"""Test oracle for the maintenance of the Audfprint hash table: a numpy restatement of HashTable.remove and
HashTable.retrieve, written from the specification of mfpa_audfprint_remove / mfpa_audfprint_retrieve (include/mfpa.h), not from
the reference's code.  tests/test_maintain_oracle.py pins it to the reference's own results (tests/golden/g18_maintain.npz);
the GPU tests then compare the device with the fixture and, on tables of their own, with this.

Tables are (2^hashbits, depth) uint32 of ((id + 1) << timebits) | time, counts int32 that may exceed depth; with
n = min(counts[b], depth) a match is a slot j < n whose (value >> timebits) - 1, on the unsigned value, is in the set.
Specified on tables whose slots at or beyond n are zero (`invariant_holds`).

    remove(table, counts, ids, n_ids, timebits)   in place, the whole set at once -> removed (n_ids,) int64
    retrieve(table, counts, id_, timebits)        (n, 2) int32 rows (time, bucket), bucket ascending then slot ascending
    retrieve_batch(table, counts, ids, timebits)  rows of all ids in request order, offsets (K + 1,)
    features(...)                                 which edge cases one removal exercises (the fixture's cases must show all)
    CASES, load_case(i)                           the fixture
"""
from __future__ import annotations

import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g18_maintain.npz")
# (hashbits, depth, timebits) of the fixture's cases, in its order
CASES = [(6, 4, 14), (8, 100, 14), (7, 130, 14), (1, 100, 14), (6, 100, 20)]


def load_case(ci):
    """Case ci of the fixture as a dict of arrays (keys without the case prefix)."""
    with np.load(GOLDEN, allow_pickle=False) as z:
        p = "c%d_" % ci
        return {k[len(p):]: z[k] for k in z.files if k.startswith(p)}


def invariant_holds(table, counts) -> bool:
    depth = table.shape[1]
    n = np.minimum(np.maximum(counts.astype(np.int64), 0), depth)
    return not np.any(table[np.arange(depth)[None, :] >= n[:, None]])


def _matches(table, counts, in_set, timebits):
    """(buckets, depth) bool: slot j < n holds an id of the set."""
    depth = table.shape[1]
    n = np.minimum(np.maximum(counts.astype(np.int64), 0), depth)
    ids = (table.astype(np.int64) >> timebits) - 1                    # the unsigned value: ids >= 2^(31 - timebits) - 1 included
    known = (ids >= 0) & (ids < in_set.size)
    hit = np.zeros(table.shape, bool)
    hit[known] = in_set[ids[known]]
    return hit & (np.arange(depth)[None, :] < n[:, None]), ids


def remove(table, counts, ids, n_ids, timebits):
    in_set = np.zeros(n_ids, bool)
    in_set[np.asarray(list(ids), np.int64)] = True
    hit, id_of = _matches(table, counts, in_set, timebits)
    removed = np.bincount(id_of[hit], minlength=n_ids).astype(np.int64)
    depth = table.shape[1]
    for b in np.flatnonzero(hit.any(axis=1)):
        n = min(max(int(counts[b]), 0), depth)
        kept = table[b, :n][~hit[b, :n]]
        table[b] = 0
        table[b, : kept.size] = kept
        counts[b] = kept.size                                         # the entries the reservoir dropped are forgotten
    return removed


def retrieve(table, counts, id_, timebits):
    in_set = np.zeros(int(id_) + 1, bool)
    in_set[int(id_)] = True
    hit, _ = _matches(table, counts, in_set, timebits)
    b, j = np.nonzero(hit)                                            # row-major: bucket ascending, then slot ascending
    return np.stack([table[b, j] & np.uint32((1 << timebits) - 1), b.astype(np.uint32)], 1).astype(np.int32).reshape(-1, 2)


def retrieve_batch(table, counts, ids, timebits):
    parts = [retrieve(table, counts, i, timebits) for i in ids]
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int32)
    rows = np.concatenate(parts) if parts else np.zeros((0, 2), np.int32)
    return rows.astype(np.int32).reshape(-1, 2), offsets


def features(table, counts, ids, timebits):
    """Edge cases that removing the set `ids` from this table exercises, as a set of names."""
    depth = table.shape[1]
    n_ids = int(max(ids)) + 1
    in_set = np.zeros(n_ids, bool)
    in_set[np.asarray(list(ids), np.int64)] = True
    hit, _ = _matches(table, counts, in_set, timebits)
    n = np.minimum(np.maximum(counts.astype(np.int64), 0), depth)
    over, any_hit = counts > depth, hit.any(axis=1)
    f = set()
    if np.any(over & any_hit):
        f.add("overfull_hit")
    if np.any(over & ~any_hit):
        f.add("overfull_not_hit")
    if np.any((n > 0) & (hit.sum(axis=1) == n)):
        f.add("emptied")
    if np.any(hit[:, 0]):
        f.add("slot0")
    if np.any(hit[np.arange(len(n))[n > 0], n[n > 0] - 1]):
        f.add("last_valid")
    if np.any(hit[:, 1:] & hit[:, :-1]):
        f.add("adjacent")
    if depth > 64 and np.any(hit[:, 63]) and np.any(hit[:, 64]):
        f.add("slots_63_64")
    if np.any(hit & (table >= np.uint32(1 << 31))):
        f.add("top_bit")
    return f
