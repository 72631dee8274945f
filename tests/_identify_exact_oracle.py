"""Test oracle for the matcher's extended modes: exact_count, find_time_range and hashesfor restated in
numpy from the specification, on top of tests/_identify_oracle.py (hits, ranking, rank_ties, rows_equivalent are its).
tests/test_identify_exact_oracle.py pins it to the reference's own results (tests/golden/g15_identify_exact.npz).

    match(table, counts, hpid, hashes, exact_count=, find_time_range=, time_quantile=, hashesfor=)
        -> (rows [id, filtered, offset, raw, rank, min_time, max_time], None or the (n, 2) [time, hash] list of row hashesfor)
"""
from __future__ import annotations

import numpy as np

from tests import _identify_oracle as io_
from tests._identify_oracle import TIMEBITS, rank_ties, rows_equivalent  # noqa: F401  (re-exported for the tests)


def encpowerof2(v) -> int:
    """N with 2^N >= v through float64 logs: for v = 2^k the quotient is not always exactly k."""
    return int(np.ceil(np.log(max(1, v)) / np.log(2)))


def full_hits(table, counts, hashes, timebits=TIMEBITS):
    """(id, dt, masked hash, query time) of every hit, in io_.hits' order (query row by query row)."""
    nb, depth = table.shape
    ids, dts = io_.hits(table, counts, hashes, timebits)
    q = np.asarray(hashes, np.int64).reshape(-1, 2)
    bucket = q[:, 1] & (nb - 1)
    per_row = np.minimum(depth, counts[bucket].astype(np.int64))
    return ids, dts, np.repeat(bucket, per_row), np.repeat(q[:, 0], per_row)


def packed_hashes(ids, dts, hs, qt, id_, mode, window):
    """Sorted distinct query_time + (hash << timebits) over the hits of id_ within `window` of `mode`; timebits from the
    largest query time over ALL hits.  When that time is a power of two, 2^timebits is not above it and values collide."""
    timebits = max(1, encpowerof2(int(qt.max())))
    sel = (ids == id_) & (np.abs(dts - mode) <= window)
    return np.unique(qt[sel] + (hs[sel] << timebits)), timebits


def time_range(ids, dts, qt, id_, mode, window, quantile):
    """Order statistics of the query times of the window's hits, one entry per hit."""
    mt = np.sort(qt[(ids == id_) & (dts >= mode - window) & (dts <= mode + window)])
    return int(mt[int(len(mt) * quantile)]), int(mt[int(len(mt) * (1.0 - quantile)) - 1])     # index -1: the last one


def match(table, counts, hpid, hashes, threshcount=5, search_depth=100, window=2, max_alignments_per_id=100,
          exact_count=False, find_time_range=False, time_quantile=0.05, hashesfor=None, timebits=TIMEBITS):
    if exact_count and threshcount < 1:
        raise ValueError("exact_count needs threshcount >= 1")
    ids, dts, hs, qt = full_hits(table, counts, hashes, timebits)
    if ids.size == 0:
        if hashesfor is not None:
            raise IndexError(hashesfor)
        return np.zeros((0, 7), np.int32), None
    uid, raw, _ = io_.ranking(ids, np.asarray(hpid))
    ncand = min(int(np.count_nonzero(raw > threshcount)), search_depth)
    base = int(dts.min())
    rows = []
    for rank in range(ncand):
        id_ = int(uid[rank])
        hist = np.bincount(dts[ids == id_] - base)
        filt = io_.locmax_values(hist)
        found = []                                       # (count, mode) in mode order
        if exact_count:                                  # every local maximum >= threshcount, offsets ascending, no cap
            for mode in np.nonzero((filt > 0) & (hist >= threshcount))[0]:
                n = len(packed_hashes(ids, dts, hs, qt, id_, int(mode) + base, window)[0])
                if n >= threshcount:
                    found.append((n, int(mode) + base))
        else:                                            # repeated first-index argmax, strictly above threshcount
            for _ in range(max_alignments_per_id + 1):
                mode = int(np.argmax(filt))
                if filt[mode] <= threshcount:
                    break
                lo, hi = max(0, mode - window), mode + window + 1
                found.append((int(hist[lo:hi].sum()), mode + base))
                filt[lo:hi] = 0
        for n, mode in found:
            t0, t1 = time_range(ids, dts, qt, id_, mode, window, time_quantile) if find_time_range else (0, 0)
            rows.append([id_, n, mode, int(raw[rank]), rank, t0, t1])
    if not rows:
        if hashesfor is not None:
            raise IndexError(hashesfor)
        return np.zeros((0, 7), np.int32), None
    r = np.array(rows, np.int64)
    r = r[np.argsort(-r[:, 1], kind="stable")].astype(np.int32)           # ties: (rank, mode order), the project's rule
    if hashesfor is None:
        return r, None
    p, tb = packed_hashes(ids, dts, hs, qt, int(r[hashesfor, 0]), int(r[hashesfor, 2]), window)
    return r, np.stack([p & ((1 << tb) - 1), p >> tb], 1)
