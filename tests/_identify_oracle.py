"""Test oracle for the Audfprint hash table and matcher: a numpy restatement of the semantics the device
kernels implement, written from the specification, not from the reference's code.  tests/test_identify_oracle.py pins it
to the reference's own results (tests/golden/g14_identify.npz); the GPU tests then apply it to hashes the device made.

    store(table, counts, rows, id_, seed)  HashTable.store; past `depth` the reservoir slot comes from the same counter-based
                                           draw as the kernel (splitmix64 keyed by seed, bucket, count)
    match(table, counts, hpid, hashes)     Matcher.match_hashes rows [id, filtered, offset, raw, rank, 0, 0]
    tie_groups(...)                        which row orders / ranks the reference leaves to numpy's unstable sort
"""
from __future__ import annotations

import numpy as np

HASHBITS, DEPTH, TIMEBITS = 20, 100, 14
M64 = (1 << 64) - 1


def _splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def reservoir_slot(seed: int, bucket: int, count: int) -> int:
    """Uniform over 0..count: the high 64 bits of a 64-bit draw times (count + 1)."""
    r = _splitmix64((seed & M64) ^ _splitmix64(((bucket << 32) | (count & 0xFFFFFFFF)) & M64))
    return (r * (count + 1)) >> 64


def empty_table(hashbits=HASHBITS, depth=DEPTH):
    return np.zeros((1 << hashbits, depth), np.uint32), np.zeros(1 << hashbits, np.int32)


def store(table, counts, rows, id_, seed=0, timebits=TIMEBITS):
    """Entries of one track, in row order.  In-bucket slot = arrival rank while the bucket has room."""
    nb, depth = table.shape
    rows = np.asarray(rows, np.int64).reshape(-1, 2)
    for t, h in rows:
        b = int(h) & (nb - 1)
        c = int(counts[b])
        val = ((id_ + 1) << timebits) | (int(t) & ((1 << timebits) - 1))
        slot = c if c < depth else reservoir_slot(seed, b, c)
        if slot < depth:
            table[b, slot] = val
        counts[b] = c + 1
    return len(rows)


def hits(table, counts, hashes, timebits=TIMEBITS):
    """(id, dt) of every stored entry of every query hash; query hashes masked, query times not."""
    nb, depth = table.shape
    q = np.asarray(hashes, np.int64).reshape(-1, 2)
    ids, dts = [], []
    for t, h in q:
        b = int(h) & (nb - 1)
        v = table[b, : min(depth, int(counts[b]))].astype(np.int64)
        ids.append((v >> timebits) - 1)
        dts.append((v & ((1 << timebits) - 1)) - int(t))
    if not ids:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(ids), np.concatenate(dts)


def ranking(ids, hpid):
    """All ids with hits, ordered by rawcount / hashesperid (float64) descending; ties: larger id first."""
    uid, raw = np.unique(ids, return_counts=True)
    w = raw / hpid[uid].astype(np.float64)
    order = np.lexsort((-uid, -w))
    return uid[order], raw[order], w[order]


def locmax_values(hist):
    """hist with every point that is not a local maximum zeroed (>= left neighbour, > right neighbour; ends see zeros)."""
    left = np.concatenate([[-1], hist[:-1]])
    right = np.concatenate([hist[1:], [-1]])
    return np.where((hist >= left) & (hist > right), hist, 0)


def match(table, counts, hpid, hashes, threshcount=5, search_depth=100, window=2, max_alignments_per_id=100,
          timebits=TIMEBITS):
    ids, dts = hits(table, counts, hashes, timebits)
    if ids.size == 0:
        return np.zeros((0, 7), np.int32)
    uid, raw, _ = ranking(ids, np.asarray(hpid))
    ncand = min(int(np.count_nonzero(raw > threshcount)), search_depth)
    base = int(dts.min())
    rows = []
    for rank in range(ncand):
        id_ = int(uid[rank])
        hist = np.bincount(dts[ids == id_] - base)
        filt = locmax_values(hist)
        for _ in range(max_alignments_per_id + 1):
            mode = int(np.argmax(filt))
            if filt[mode] <= threshcount:
                break
            lo, hi = max(0, mode - window), mode + window + 1
            rows.append([id_, int(hist[lo:hi].sum()), mode + base, int(raw[rank]), rank, 0, 0])
            filt[lo:hi] = 0
    if not rows:
        return np.zeros((0, 7), np.int32)
    r = np.array(rows, np.int64)
    return r[np.argsort(-r[:, 1], kind="stable")].astype(np.int32)


def rank_ties(table, counts, hpid, hashes, timebits=TIMEBITS):
    """{id: (first, last) ranking position of its weighted-count tie group} over ids with hits: positions inside a group
    are not determined by the reference (numpy's argsort without kind=)."""
    ids, _ = hits(table, counts, hashes, timebits)
    if ids.size == 0:
        return {}
    uid, _, w = ranking(ids, np.asarray(hpid))
    out = {}
    for v in np.unique(w):
        pos = np.nonzero(w == v)[0]
        for p in pos:
            out[int(uid[p])] = (int(pos[0]), int(pos[-1]))
    return out


def rows_equivalent(got, want, ties=None):
    """Rows of match_hashes compared under the reference's determinism: the filtered-count column in order, the rows as a
    multiset, a row at its position wherever its count is unique, and orig_rank exactly unless the id's weighted count ties
    (then within the tie group's positions).  Returns an error string, or None."""
    got = np.asarray(got, np.int64).reshape(-1, 7)
    want = np.asarray(want, np.int64).reshape(-1, 7)
    if got.shape != want.shape:
        return f"{got.shape[0]} rows, expected {want.shape[0]}"
    if not np.array_equal(got[:, 1], want[:, 1]):
        return f"filtered counts {got[:, 1].tolist()} != {want[:, 1].tolist()}"
    ties = ties or {}
    key = lambda r: (r[0], r[1], r[2], r[3], r[5], r[6])
    if sorted(map(key, got.tolist())) != sorted(map(key, want.tolist())):
        return "row sets differ"
    for r in got.tolist() + want.tolist():
        lo, hi = ties.get(r[0], (None, None))
        if lo is not None and lo != hi and not lo <= r[4] <= hi:
            return f"orig_rank {r[4]} of id {r[0]} outside its tie group [{lo}, {hi}]"
    strict = [r for r in want.tolist() if ties.get(r[0], (0, 0))[0] == ties.get(r[0], (0, 0))[1]]
    for r in strict:
        if r not in got.tolist():
            return f"row {r} missing"
    cnt = want[:, 1]
    for i in range(len(cnt)):
        if np.count_nonzero(cnt == cnt[i]) == 1 and key(got[i]) != key(want[i]):
            return f"row {i}: {got[i].tolist()} != {want[i].tolist()}"
    return None
