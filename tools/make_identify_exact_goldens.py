#!/usr/bin/env python3
"""Generate tests/golden/g15_identify_exact.npz with the REAL reference's Matcher (afp/audfprint/audfprint_match.py) run with
exact_count / find_time_range / hashesfor.  Build-container only, like tools/make_identify_goldens.py, whose make_tracks /
make_queries it reuses with the same seed; only numbers go into the repository.

The table is g14's 300 tracks (the digests of the table are asserted equal to g14's) followed by four more tracks, ids
300..303, stored on top.  g14's table has no id with one hash at two nearby times, so the cases below need them:

  300  12 of its 40 hashes stored at t and t + 1: one query row gives two hits inside one window (exact < approximate);
  301  a query whose offsets to it are 50 (12 rows), 51 (3 rows) and 52 (10 rows): two local maxima two bins apart;
  302  rows (100, h + 1) and (1124, h): the query shifted by 100 has the largest time 1024 = 2^10 and a row at time 0,
       and the two rows pack to the same value; a second query with rows at one time whose hashes differ only above bit 20;
  303  two rows at offsets far apart, run with threshcount = 1: windows of one hit (match_times[-1]).

Recorded for every query (g14's 38, 9 of which have negative query times, and the 5 new ones): the reference's rows for
(exact_count, find_time_range) = (F,F), (F,T), (T,F), (T,T); for a few queries the same with threshcount = 1 and with
time_quantile 0 and 0.25; and hashesfor lists of rows 0 and 1 wherever the filtered count decides that row's place.

Usage:  python tools/make_identify_exact_goldens.py
"""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from make_goldens import OUT, import_reference  # noqa: E402
from make_identify_goldens import make_queries, make_tracks  # noqa: E402

COMBOS = {"ff": (False, False), "ft": (False, True), "tf": (True, False), "tt": (True, True)}


def extra_tracks(rng, used):
    """Tracks 300..303 and their queries.  Hashes are fresh: none of them is in the g14 table."""
    def fresh(n):
        out = []
        while len(out) < n:
            h = int(rng.integers(0, (1 << 20) - 1))
            if h not in used and h + 1 not in used:
                used.update((h, h + 1))
                out.append(h)
        return np.array(out, np.int64)

    tracks, queries = [], {}
    # 300: stored times t and t + 1 under one hash
    t = np.sort(rng.choice(np.arange(200, 3000, 3), 40, replace=False))
    h = fresh(40)
    base = np.stack([t, h], 1)
    tracks.append(np.concatenate([base, base[:12] + [1, 0]]))
    queries["double"] = base - [100, 0]
    # 301: offsets 50 x 12, 51 x 3, 52 x 10
    t = np.sort(rng.choice(np.arange(200, 3000, 3), 30, replace=False))
    base = np.stack([t, fresh(30)], 1)
    tracks.append(base)
    queries["two_maxima"] = np.concatenate([base[:12] - [50, 0], base[12:15] - [51, 0], base[15:25] - [52, 0]])
    # 302: query times 0 and 1024 = 2^10 that pack to one value; hashes that differ only above bit 20
    h = fresh(24)
    t = np.sort(rng.choice(np.arange(101, 1124), 18, replace=False))
    base = np.concatenate([[[100, h[0] + 1], [1124, h[0]]], np.stack([t, h[1:19]], 1),
                           np.stack([np.arange(2000, 2005), h[19:24]], 1)])
    tracks.append(base)
    queries["pow2"] = base[:20] - [100, 0]
    sub = base[2:14] - [90, 0]
    queries["high_bits"] = np.concatenate([sub, sub[:4] + [0, 1 << 20], sub[:2] + [0, 3 << 20]])
    # 303: two single hits far apart (threshcount = 1)
    base = np.stack([np.arange(500, 3500, 500), fresh(6)], 1)
    tracks.append(base)
    queries["single_hits"] = np.array([base[0] - [10, 0], base[4] - [400, 0]])
    out = {}
    for name, q in queries.items():                                            # hashes_batch order: unique, sorted by (time, hash)
        q = np.asarray(q, np.int64)
        k = np.unique((q[:, 0] << 32) + (q[:, 1] & 0xFFFFFFFF))
        out[name] = np.stack([k >> 32, k & 0xFFFFFFFF], 1).astype(np.int32)
    return [np.asarray(tr, np.int32) for tr in tracks], out


def main():
    import_reference()
    from afp.audfprint.audfprint_match import Matcher, encpowerof2
    from afp.audfprint.hash_table import HashTable

    g14 = np.load(os.path.join(OUT, "g14_identify.npz"))
    digest = lambda a, dt: np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, dt).tobytes()).digest(), np.uint8)
    rng = np.random.default_rng(14)
    tracks, hot = make_tracks(rng)
    ht = HashTable()
    for i, tr in enumerate(tracks):
        ht.store("track_%03d" % i, tr.copy())
    assert np.array_equal(digest(ht.table, "<u4"), g14["table_sha256"]) and np.array_equal(digest(ht.counts, "<i4"), g14["counts_sha256"])
    queries = make_queries(rng, tracks, hot)
    assert np.array_equal(np.concatenate(queries), g14["query_rows"])
    used = set((np.concatenate(tracks)[:, 1].astype(np.int64) & 0xFFFFF).tolist())
    xtracks, xq = extra_tracks(np.random.default_rng(15), used)
    for i, tr in enumerate(xtracks):
        ht.store("track_%03d" % (len(tracks) + i), tr.copy())
    assert int(ht.counts.max()) <= ht.depth, "the golden database must not overflow"
    names = list(xq)
    first = len(queries)
    queries = queries + [xq[n] for n in names]
    qix = {n: first + i for i, n in enumerate(names)}

    def run(q, exact, trange, thresh=5, quantile=0.05, hashesfor=None):
        m = Matcher()
        m.exact_count, m.find_time_range, m.threshcount, m.time_quantile = exact, trange, thresh, quantile
        r, hf = m.match_hashes(ht, q.copy(), hashesfor)
        return np.asarray(r, np.int32).reshape(-1, 7), hf

    cat = lambda xs: (np.concatenate(xs).astype(np.int32) if xs else np.zeros((0, 2), np.int32))
    off = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    out = {}
    res = {}
    for key, (ex, tr) in COMBOS.items():
        res[key] = [run(q, ex, tr)[0] if len(q) else np.zeros((0, 7), np.int32) for q in queries]
        out["rows_" + key], out["off_" + key] = cat(res[key]), off(res[key])
    differ = sum(len(a) != len(b) or not np.array_equal(np.sort(a[:, 1]), np.sort(b[:, 1])) for a, b in zip(res["ff"], res["tf"]))
    assert differ >= 8, differ

    # a tie of weighted counts across the search_depth cut would make the reference's candidate SET undetermined
    m = Matcher()
    for q in queries:
        hits = ht.get_hits(q)
        if hits.size == 0:
            continue
        uid, raw = np.unique(hits[:, 0], return_counts=True)
        w = np.sort(raw / ht.hashesperid[uid].astype(float))[::-1]
        for thresh in (5, 1):
            d = min(int(np.count_nonzero(raw > thresh)), m.search_depth)
            assert d == 0 or d == len(w) or w[d - 1] != w[d], ("weighted-count tie at the candidate cut", len(q), d)

    # ---- the reference itself shows each effect
    row_of = lambda key, name, id_: [r for r in res[key][qix[name]].tolist() if r[0] == id_]
    a, e = row_of("ff", "double", 300), row_of("tf", "double", 300)
    assert len(a) == len(e) == 1 and a[0][1] == 52 and e[0][1] == 40, (a, e)             # one query row, two hits in one window
    e = row_of("tf", "two_maxima", 301)
    assert sorted(r[2] for r in e) == [50, 52] and len(row_of("ff", "two_maxima", 301)) == 1, e
    q = queries[qix["pow2"]]
    hits = ht.get_hits(q)
    assert int(hits[:, 3].max()) == 1024 == int(q[:, 0].max()) and int(q[:, 0].min()) == 0 and encpowerof2(1024) == 10
    a, e = row_of("ff", "pow2", 302), row_of("tf", "pow2", 302)
    assert a[0][1] == 20 and e[0][1] == 19, (a, e)                                        # 1024 + (h << 10) == 0 + ((h + 1) << 10)
    a, e = row_of("ff", "high_bits", 302), row_of("tf", "high_bits", 302)
    assert a[0][1] == 18 and e[0][1] == 12, (a, e)
    t1 = [qix["single_hits"], qix["double"], qix["pow2"], qix["two_maxima"], 24, 25]     # 24: the empty query, 25: noise
    assert len(queries[24]) == 0
    for key, (ex, tr) in COMBOS.items():
        rs = [run(queries[qi], ex, tr, thresh=1)[0] if len(queries[qi]) else np.zeros((0, 7), np.int32) for qi in t1]
        out["t1_rows_" + key], out["t1_off_" + key] = cat(rs), off(rs)
        if key == "tt":
            one = [r for r in rs[0].tolist() if r[0] == 303]
            assert len(one) == 2 and all(r[1] == 1 and r[5] == r[6] for r in one), one    # match_times of length 1: index -1
            assert sorted(r[5] for r in one) == sorted(queries[t1[0]][:, 0].tolist())
    out["t1_queries"] = np.array(t1, np.int32)
    qq = [qix["double"], 0, 16, 20]
    out["quantile_queries"] = np.array(qq, np.int32)
    for tag, quant in (("q0", 0.0), ("q25", 0.25)):
        for key in ("ft", "tt"):
            rs = [run(queries[qi], *COMBOS[key], quantile=quant)[0] for qi in qq]
            out[f"{tag}_rows_{key}"], out[f"{tag}_off_{key}"] = cat(rs), off(rs)
            assert any(not np.array_equal(r[:, 5:], res[key][qi][:, 5:]) for r, qi in zip(rs, qq)), (tag, key)

    # ---- hashesfor: rows 0 and 1 where the filtered count decides the row's place
    spec, lists = [], []
    for qi in [0, 5, 16, 17, 20, 22] + [qix[n] for n in ("double", "two_maxima", "pow2", "high_bits")]:
        for ex in (False, True):
            rows = res["tf" if ex else "ff"][qi]
            for k in (0, 1):
                if k >= len(rows) or np.count_nonzero(rows[:, 1] == rows[k, 1]) != 1:
                    continue
                r, hf = run(queries[qi], ex, False, hashesfor=k)
                assert np.array_equal(r, rows)
                spec.append([qi, int(ex), k])
                lists.append(np.asarray(hf, np.int64).reshape(-1, 2))
    hf = lists[[s[:2] for s in spec].index([qix["pow2"], 1])]
    qset = set(map(tuple, (queries[qix["pow2"]].astype(np.int64) & [0xFFFFFFFF, 0xFFFFF]).tolist()))
    assert len(hf) == 19 and not any(int(t) == 1024 for t in hf[:, 0]) and set(map(tuple, hf.tolist())) < qset
    assert len(spec) >= 20, len(spec)
    out["hf_spec"], out["hf_rows"], out["hf_off"] = np.array(spec, np.int32), cat(lists), off(lists)

    cnz = np.flatnonzero(ht.counts)
    path = os.path.join(OUT, "g15_identify_exact.npz")
    np.savez_compressed(
        path, extra_track_rows=cat(xtracks), extra_track_off=off(xtracks),
        table_sha256=digest(ht.table, "<u4"), counts_sha256=digest(ht.counts, "<i4"),
        n_entries=np.int64(ht.counts.sum()), n_buckets=np.int64(cnz.size), hashesperid=np.asarray(ht.hashesperid, np.uint32),
        query_rows=cat(queries), query_off=off(queries), query_names=np.array(names), first_new_query=np.int64(first), **out)
    print(f"g15_identify_exact.npz {os.path.getsize(path) / 1024:.1f} KiB; {len(queries)} queries; rows "
          + ", ".join(f"{k} {len(out['rows_' + k])}" for k in COMBOS) + f"; exact differs on {differ} queries; {len(spec)} hash lists")


if __name__ == "__main__":
    main()
