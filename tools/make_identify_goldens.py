#!/usr/bin/env python3
"""Generate tests/golden/g14_identify.npz and tests/golden/g14_hashtable.pklz with the REAL reference's HashTable.store,
Matcher.match_hashes and HashTable.save (afp/audfprint/hash_table.py, afp/audfprint/audfprint_match.py) on synthetic
(time, hash) sets.  Build-container only, like tools/make_goldens.py, whose import_reference() it reuses; only numbers and
the file the reference itself writes go into the repository.

The large table is recorded by SHA-256 digests of its exact bytes (table as little-endian uint32, counts as int32), which
pins it bit for bit; the .pklz holds a small table (hashbits 12, depth 8) that the reference's store filled and its save wrote.

Cases: tracks of 3 to 1500 hashes; "hot" buckets filled close to, not over, depth; hashes with bits above
the 20 the table keeps and stored times above 14 bits; queries that are shifted subsets of a track with dt jitter of +-1
and +-2 and negative offsets; a track matched at two alignments; more than 100 candidate ids above threshold; short tracks
whose weighted count is high with rawcount <= 5; duplicate tracks (ties on the weighted and the filtered count); empty
queries and queries with no hits.  A second database, built with a seeded `random`, overflows its buckets: only its counts
and hashesperid are recorded (the reference's reservoir draw cannot be reproduced).

Usage:  python tools/make_identify_goldens.py
"""
from __future__ import annotations

import contextlib
import hashlib
import io
import os
import random
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from make_goldens import OUT, import_reference  # noqa: E402

N_TRACKS = 300
N_HOT = 40                 # hot hashes shared by tracks 0..N_HOT_TRACKS-1
N_HOT_TRACKS, HOT_PER_TRACK = 110, 35
PRIMES = [p for p in range(41, 1000) if all(p % d for d in range(2, int(p ** 0.5) + 1))]
SMALL_HASHBITS, SMALL_DEPTH, SMALL_TRACKS = 12, 8, range(150, 170)      # the reference-written .pklz (a small table)


def make_tracks(rng):
    tracks = []
    hot = rng.choice(np.arange(1 << 20), N_HOT, replace=False)
    for i in range(N_TRACKS):
        if i >= 280:                                     # short tracks: 3..5 hashes (some duplicated below)
            n = int(rng.integers(3, 6)) if i != 281 else 5     # 281 longer than its 3-row duplicate 295
        elif i < N_HOT_TRACKS:                           # hashesperid a distinct prime: no weighted-count ties among them
            n = PRIMES[i] - HOT_PER_TRACK
        else:
            n = 1500 if i == 250 else int(np.clip(rng.lognormal(3.8, 1.0), 8, 1500))
        t = np.sort(rng.integers(0, 4000 if i != 7 else 24000, n))      # track 7: times beyond 14 bits
        h = rng.integers(0, 1 << 20, n)
        if i % 11 == 3:
            h = h | (int(rng.integers(1, 1 << 11)) << 20)                  # bits above the table's 20
        rows = [np.stack([t, h], 1)]
        if i < N_HOT_TRACKS:                             # 35 of the 40 hot hashes at a track-consistent time
            sel = (np.arange(HOT_PER_TRACK) + HOT_PER_TRACK * i) % N_HOT    # balanced: every hot bucket gets 96 or 97 entries
            off = int(rng.integers(100, 2000))
            rows.append(np.stack([off + 7 * sel, hot[sel]], 1))
        tracks.append(np.concatenate(rows).astype(np.int32))
    tracks[290] = tracks[200].copy()                     # duplicates: identical weighted counts and modes
    tracks[291] = tracks[200].copy()
    tracks[295] = tracks[281][:3].copy()                 # short duplicates
    return tracks, hot


def make_queries(rng, tracks, hot):
    qs = []

    def excerpt(i, frac, offset, jitter=0, noise=0):
        tr = tracks[i]
        keep = tr[rng.random(len(tr)) < frac].astype(np.int64)
        q = keep.copy()
        q[:, 0] = keep[:, 0] - offset
        if jitter:
            q[:, 0] += rng.integers(-jitter, jitter + 1, len(q))
        if noise:
            q = np.concatenate([q, np.stack([rng.integers(0, 3000, noise), rng.integers(0, 1 << 22, noise)], 1)])
        return q

    for i in (10, 40, 160, 170, 200, 230, 250, 7):
        qs.append(excerpt(i, 0.5, int(rng.integers(0, 400))))
    for i, off in ((20, -30), (165, -250), (210, -1)):                          # negative offsets: query times after the track's
        qs.append(excerpt(i, 0.6, off))
    for i, j in ((30, 1), (175, 1), (180, 2), (215, 2), (240, 2)):             # dt jitter +-1 / +-2
        qs.append(excerpt(i, 0.8, int(rng.integers(-100, 300)), jitter=j, noise=20))
    for i in (190, 220):                                                       # two alignments of one track
        a = excerpt(i, 0.5, 100)
        b = excerpt(i, 0.5, 900)
        qs.append(np.concatenate([a, b]))
    # more than 100 candidates above threshold: every hot hash at every multiple-of-7 time (the hot tracks align)
    sel = np.arange(N_HOT)
    qs.append(np.stack([7 * sel, hot[sel]], 1))
    qs.append(np.concatenate([np.stack([7 * sel + 3, hot[sel]], 1), excerpt(60, 0.4, 50)]))
    # short tracks with a high weighted count and rawcount <= 5 taking candidate slots
    qs.append(np.concatenate([tracks[281], tracks[282], tracks[283], excerpt(45, 0.5, 10)]))
    qs.append(np.concatenate([tracks[284][:-1], tracks[295], excerpt(120, 0.5, -5)]))
    # ties: the duplicated track 200 (and 290, 291) on its own, with query times beyond 14 bits
    qs.append(excerpt(200, 0.7, 40))
    big = excerpt(200, 0.7, 0)
    big[:, 0] += 20000
    qs.append(big)
    qs.append(np.zeros((0, 2), np.int64))                                      # empty query
    qs.append(np.stack([rng.integers(0, 3000, 50), rng.integers(0, 1 << 20, 50)], 1))   # noise (few or no hits)
    for i in rng.choice(280, 12, replace=False):                               # random excerpts, mixed fractions / offsets
        qs.append(excerpt(int(i), float(rng.uniform(0.1, 0.9)), int(rng.integers(-300, 600)), jitter=int(rng.integers(0, 3)),
                          noise=int(rng.integers(0, 50))))
    out = []
    for q in qs:                                                               # hashes_batch order: unique, sorted by (time, hash)
        q = np.asarray(q, np.int64).reshape(-1, 2)
        k = np.unique((q[:, 0] << 32) + (q[:, 1] & 0xFFFFFFFF))
        out.append(np.stack([k >> 32, k & 0xFFFFFFFF], 1).astype(np.int64).astype(np.int32))
    return out


def main():
    import_reference()
    from afp.audfprint.audfprint_match import Matcher
    from afp.audfprint.hash_table import HashTable

    rng = np.random.default_rng(14)
    tracks, hot = make_tracks(rng)
    ht = HashTable()
    quiet = contextlib.redirect_stdout(io.StringIO())
    for i, tr in enumerate(tracks):
        ht.store("track_%03d" % i, tr.copy())
    assert int(ht.counts.max()) <= ht.depth, "the golden database must not overflow"
    full = int(np.count_nonzero(ht.counts >= 90))
    assert full >= 20, full
    queries = make_queries(rng, tracks, hot)
    m = Matcher()
    res, nres = [], []
    for q in queries:
        r, _ = m.match_hashes(ht, q.copy())
        res.append(np.asarray(r, np.int32).reshape(-1, 7))
        nres.append(len(r))
    # a tie of weighted counts across the search_depth cut would make the reference's candidate SET undetermined
    for q in queries:
        hits = ht.get_hits(q)
        if hits.size == 0:
            continue
        uid, raw = np.unique(hits[:, 0], return_counts=True)
        w = np.sort(raw / ht.hashesperid[uid].astype(float))[::-1]
        d = min(int(np.count_nonzero(raw > m.threshcount)), m.search_depth)
        assert d == 0 or d == len(w) or w[d - 1] != w[d], ("weighted-count tie at the candidate cut", len(q), d, w[d - 2:d + 2])
    assert max(nres) > 0 and min(nres) == 0

    # a small table (hashbits 12, depth 8) filled by the reference's own store and written by its save: the .pklz golden
    small = HashTable()
    small.hashbits, small.depth = SMALL_HASHBITS, SMALL_DEPTH
    small.table = np.zeros((1 << SMALL_HASHBITS, SMALL_DEPTH), np.uint32)
    small.counts = np.zeros(1 << SMALL_HASHBITS, np.int32)
    for i in SMALL_TRACKS:
        small.store("track_%03d" % i, tracks[i].copy())
    assert int(small.counts.max()) <= small.depth
    with quiet:
        small.save(os.path.join(OUT, "g14_hashtable.pklz"))

    # overflowing database: 30 tracks over the same 40 buckets, seeded `random` for the reservoir draw
    random.seed(1414)
    orng = np.random.default_rng(1415)
    ovf = HashTable()
    otracks = []
    pool = orng.choice(1 << 20, 40, replace=False)
    for i in range(30):
        n = int(orng.integers(100, 250))
        tr = np.stack([np.sort(orng.integers(0, 5000, n)), pool[orng.integers(0, 40, n)]], 1).astype(np.int32)
        otracks.append(tr)
        ovf.store("ovf_%02d" % i, tr.copy())
    assert int(ovf.counts.max()) > ovf.depth

    cat = lambda xs: (np.concatenate(xs).astype(np.int32) if xs else np.zeros((0, 2), np.int32))
    off = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    digest = lambda a, dt: np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, dt).tobytes()).digest(), np.uint8)
    cnz = np.flatnonzero(ht.counts)
    onz = np.flatnonzero(ovf.counts)
    path = os.path.join(OUT, "g14_identify.npz")
    np.savez_compressed(
        path,
        track_rows=cat(tracks), track_off=off(tracks),
        table_sha256=digest(ht.table, "<u4"), counts_sha256=digest(ht.counts, "<i4"),
        n_entries=np.int64(ht.counts.sum()), n_buckets=np.int64(cnz.size),
        small_table=small.table.astype(np.uint32), small_counts=small.counts.astype(np.int32),
        small_hashesperid=np.asarray(small.hashesperid, np.uint32),
        hashesperid=np.asarray(ht.hashesperid, np.uint32),
        query_rows=cat(queries), query_off=off(queries),
        result_rows=np.concatenate(res).astype(np.int32), result_off=off(res),
        ovf_rows=cat(otracks), ovf_off=off(otracks),
        ovf_counts_idx=onz.astype(np.int32), ovf_counts_val=ovf.counts[onz].astype(np.int32),
        ovf_hashesperid=np.asarray(ovf.hashesperid, np.uint32),
    )
    print(f"g14_identify.npz {os.path.getsize(path) / 1024:.1f} KiB; g14_hashtable.pklz "
          f"{os.path.getsize(os.path.join(OUT, 'g14_hashtable.pklz')) / 1024:.1f} KiB; {len(queries)} queries, "
          f"{sum(nres)} result rows, {full} buckets >= 90 entries, max rows {max(nres)}")


if __name__ == "__main__":
    main()
