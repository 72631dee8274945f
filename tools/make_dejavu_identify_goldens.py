#!/usr/bin/env python3
"""Generate tests/golden/g15_dejavu_identify.npz with the REAL reference's PostgreSQLDatabase.insert_song / insert_hashes /
return_matches (afp/dejavu/postgres_database.py), Dejavu.align_matches (afp/dejavu/dejavu.py:312-378) and
FileRecognizer.recognize_file's match rule (afp/dejavu/file_recognizer.py:42-75) on synthetic (hash, offset) sets.
Build-container only, like tools/make_goldens.py, whose import_reference() it reuses; only numbers go into the repository.

psycopg2 is stubbed: an in-memory cursor executes exactly the four statements this path issues -- INSERT_FINGERPRINT (ON
CONFLICT DO NOTHING under UNIQUE(song_id, offset, hash)), INSERT_SONG ... RETURNING song_id (SERIAL from 1),
SELECT_MULTIPLE with one IN value, and SELECT_SONG -- and refuses any other.

Cases: ties between songs (identical songs: the smaller sid wins); ties between offsets within a song (the smallest diff
wins); negative diffs; one hash at several query offsets; duplicate pairs in a query and on insert; a "hot" hash shared by
every song; an empty song; a query with no hits; an empty query; a best count of exactly 1 (no match); topn = 3.

Usage:  python tools/make_dejavu_identify_goldens.py
"""
from __future__ import annotations

import os
import sys
import types
import warnings

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from make_goldens import OUT, import_reference  # noqa: E402

N_SONGS = 40
EMPTY_SONG = 7                  # sid 8: no hashes at all
TWIN = (20, 21)                 # sids 21 and 22 carry the same rows
TOPNS = (1, 3)
LONE = bytes(range(1, 11))


class _Store:
    def __init__(self, pg):
        self.pg = pg
        self.fp = set()         # (hash bytes, sid, offset)
        self.songs = []         # (name, sha1 hex, total)


class _Cursor:
    def __init__(self, store, dictionary):
        self.s, self.dictionary, self._rows = store, dictionary, []

    def execute(self, q, params=()):
        pg = self.s.pg
        if q == pg.INSERT_FINGERPRINT:
            sid, hsh, off = params
            self.s.fp.add((bytes.fromhex(hsh), int(sid), int(off)))
            self._rows = []
        elif q == pg.INSERT_SONG:
            self.s.songs.append(tuple(params))
            self._rows = [(len(self.s.songs),)]
        elif q == pg.SELECT_MULTIPLE % pg.IN_MATCH:
            (hsh,) = params
            h = bytes.fromhex(hsh)
            self._rows = sorted((r[0].hex().upper(), r[1], r[2]) for r in self.s.fp if r[0] == h)
        elif q == pg.SELECT_SONG:
            name, sha, total = self.s.songs[int(params[0]) - 1]
            self._rows = [{"song_name": name, "file_sha1": sha.upper(), "total_hashes": total}]
        else:
            raise NotImplementedError(q)

    def executemany(self, q, seq):
        for p in seq:
            self.execute(q, p)

    def fetchone(self):
        return self._rows[0] if self._rows else None

    def __iter__(self):
        return iter(self._rows)

    def close(self):
        pass


def stub_psycopg2(holder):
    class _Conn:
        def cursor(self, cursor_factory=None):
            return _Cursor(holder["store"], cursor_factory is not None)

        def commit(self):
            pass

        def close(self):
            pass

    pg = types.ModuleType("psycopg2")
    pg.connect = lambda **k: _Conn()
    pg.DatabaseError = RuntimeError
    ex = types.ModuleType("psycopg2.extras")
    ex.DictCursor = object
    pg.extras = ex
    sys.modules["psycopg2"], sys.modules["psycopg2.extras"] = pg, ex


def reference_modules():
    import torch
    holder = {}
    stub_psycopg2(holder)
    ref = import_reference()
    from training.model import Demucs
    sd = Demucs().state_dict()
    orig = torch.load
    torch.load = lambda *a, **k: {"model_state_dict": sd}
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            import dejavu.dejavu as rdj
            import dejavu.file_recognizer as rfr
            import dejavu.postgres_database as rpg
    finally:
        torch.load = orig
    return holder, ref, rdj, rfr, rpg


def make_songs(rng):
    pool = rng.integers(0, 256, (600, 10), dtype=np.uint8)
    pool[300:320, :9] = pool[299, :9]           # hashes differing in the last byte only (one directory bucket)
    pool[320:340, :4] = pool[298, :4]           # same leading 32 bits
    hot = pool[0]
    songs = []
    for s in range(N_SONGS):
        if s == EMPTY_SONG:
            songs.append([])
            continue
        n = int(rng.integers(20, 160))
        h = pool[rng.integers(1, len(pool), n)]
        off = rng.integers(0, 3000, n)
        rows = [(bytes(h[i]), int(off[i])) for i in range(n)]
        rows.append((bytes(hot), int(rng.integers(0, 3000))))
        rows += rows[: n // 5]                  # duplicates on insert
        songs.append(rows)
    songs[TWIN[1]] = list(songs[TWIN[0]])
    songs[15].append((LONE, 1234))              # a hash no other song carries
    return songs, pool, hot


def make_queries(rng, songs, pool, hot):
    qs = []

    def excerpt(s, frac, shift, noise=0):
        rows = [(d, o + shift) for d, o in sorted(set(songs[s])) if rng.random() < frac]
        rows += [(bytes(rng.integers(0, 256, 10, dtype=np.uint8)), int(rng.integers(0, 2000))) for _ in range(noise)]
        return rows

    qs.append(excerpt(3, 0.5, -100))                        # positive diffs
    qs.append(excerpt(4, 0.6, 500, noise=5))                # negative diffs
    qs.append(excerpt(TWIN[0], 0.7, 0))                     # two identical songs: the smaller sid wins
    base = sorted(set(songs[12]))                           # two diffs of song 12 with equal counts: the smaller wins
    a, b = base[: len(base) // 2], base[len(base) // 2:]
    k = min(len(a), len(b))
    qs.append([(d, o + 50) for d, o in a[:k]] + [(d, o + 80) for d, o in b[:k]])
    d0, o0 = sorted(set(songs[5]))[0]                       # one hash at several query offsets
    qs.append(excerpt(5, 0.4, 10) + [(d0, o0 + 10 + j) for j in (1, 2, 3)])
    q = excerpt(6, 0.5, 30)
    qs.append(q + q[: len(q) // 2])                         # duplicate pairs in the query
    qs.append([(bytes(hot), 100), (bytes(hot), 900)] + excerpt(9, 0.1, 0))   # hot hash
    qs.append([(bytes(rng.integers(0, 256, 10, dtype=np.uint8)), int(rng.integers(0, 500))) for _ in range(30)])  # no hits
    qs.append([(LONE, 1000)])                               # a best count of exactly 1: no match
    qs.append([])                                           # empty query
    for _ in range(20):
        s = int(rng.integers(0, N_SONGS))
        qs.append(excerpt(s, float(rng.uniform(0.05, 0.9)), int(rng.integers(-400, 400)), noise=int(rng.integers(0, 40))))
    return qs


def main():
    holder, ref, rdj, rfr, rpg = reference_modules()
    rng = np.random.default_rng(15)
    songs, pool, hot = make_songs(rng)
    queries = make_queries(rng, songs, pool, hot)
    db = rpg.PostgreSQLDatabase()
    holder["store"] = _Store(db)
    for s, rows in enumerate(songs):
        sid = db.insert_song("song_%03d" % s, "%040X" % (s + 1), len(set(rows)))
        assert sid == s + 1
        db.insert_hashes(sid, [(d.hex(), o) for d, o in rows])
    djv = rdj.Dejavu.__new__(rdj.Dejavu)
    djv.db, djv.settings = db, ref["afp_settings"]["dejavu"]
    djv.denoising, djv.denoising_model = False, None
    djv.generate_fingerprints = lambda channel: (channel, 0.0)

    out = {"ins_dig": [], "ins_sid": [], "ins_off": []}
    for s, rows in enumerate(songs):
        for d, o in rows:
            out["ins_dig"].append(np.frombuffer(d, np.uint8))
            out["ins_sid"].append(s + 1)
            out["ins_off"].append(o)
    fp = sorted(holder["store"].fp)
    res = {k: [] for k in ("q_dig", "q_off", "q_n", "rm_sid", "rm_diff", "rm_n", "dd_sid", "dd_cnt", "dd_n", "match",
                           "queried")}
    for t in TOPNS:
        res[f"top{t}_int"], res[f"top{t}_float"], res[f"top{t}_n"] = [], [], []
    for q in queries:
        res["q_n"].append(len(q))
        for d, o in q:
            res["q_dig"].append(np.frombuffer(d, np.uint8))
            res["q_off"].append(o)
        hashes = set((d.hex(), o) for d, o in q)
        matches, dedup, _ = djv.find_matches(hashes)
        m = sorted(matches)
        res["rm_n"].append(len(m))
        res["rm_sid"] += [x[0] for x in m]
        res["rm_diff"] += [x[1] for x in m]
        res["dd_n"].append(len(dedup))
        res["dd_sid"] += sorted(dedup)
        res["dd_cnt"] += [dedup[k] for k in sorted(dedup)]
        res["queried"].append(len(hashes))
        rfr.read = lambda filename, **kw: ([[(d.hex(), o) for d, o in q]], 8000, None)
        r = rfr.FileRecognizer(djv).recognize_file("query")
        res["match"].append(int(r["match"]))
        for t in TOPNS:
            rows = r["results"] if t == 1 else djv.align_matches(matches, dedup, len(hashes), topn=t)
            res[f"top{t}_n"].append(len(rows))
            for row in rows:
                res[f"top{t}_int"].append([row["song_id"], row["offset"], row["input_total_hashes"],
                                           row["fingerprinted_hashes_in_db"], row["hashes_matched_in_input"],
                                           row["nb_matches_with_offset"]])
                res[f"top{t}_float"].append([row["input_confidence"], row["input_confidence_2"],
                                             row["fingerprinted_confidence"], row["offset_seconds"]])
    arrays = dict(
        ins_dig=np.array(out["ins_dig"], np.uint8).reshape(-1, 10), ins_sid=np.array(out["ins_sid"], np.int32),
        ins_off=np.array(out["ins_off"], np.int32),
        song_total=np.array([s[2] for s in holder["store"].songs], np.int64),
        fp_dig=np.array([np.frombuffer(r[0], np.uint8) for r in fp], np.uint8).reshape(-1, 10),
        fp_sid=np.array([r[1] for r in fp], np.int32), fp_off=np.array([r[2] for r in fp], np.int32),
        q_dig=np.array(res["q_dig"], np.uint8).reshape(-1, 10), q_off=np.array(res["q_off"], np.int32),
        q_n=np.array(res["q_n"], np.int64), rm_sid=np.array(res["rm_sid"], np.int64), rm_diff=np.array(res["rm_diff"], np.int64),
        rm_n=np.array(res["rm_n"], np.int64), dd_sid=np.array(res["dd_sid"], np.int64), dd_cnt=np.array(res["dd_cnt"], np.int64),
        dd_n=np.array(res["dd_n"], np.int64), match=np.array(res["match"], np.int64), queried=np.array(res["queried"], np.int64))
    for t in TOPNS:
        arrays[f"top{t}_int"] = np.array(res[f"top{t}_int"], np.int64).reshape(-1, 6)
        arrays[f"top{t}_float"] = np.array(res[f"top{t}_float"], np.float64).reshape(-1, 4)
        arrays[f"top{t}_n"] = np.array(res[f"top{t}_n"], np.int64)
    path = os.path.join(OUT, "g15_dejavu_identify.npz")
    np.savez_compressed(path, **arrays)
    print(f"g15_dejavu_identify.npz  {os.path.getsize(path) / 1024:.1f} KiB, {len(fp)} rows, {len(queries)} queries, "
          f"matches {int(arrays['match'].sum())}")


if __name__ == "__main__":
    main()
