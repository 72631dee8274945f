"""Numpy restatement of Dejavu's fingerprint store and matcher, for the tests (no reference code is copied).

- store: the fingerprints table under UNIQUE(song_id, offset, hash) with INSERT ... ON CONFLICT DO NOTHING
  (afp/dejavu/postgres_database.py:266-281, :288-295), as the device lays it out: (M, 5) int32 rows [w0, w1, w2, sid, offset]
  sorted by (hash, sid, offset), w0..w2 the digest as big-endian words.
- return_matches: postgres_database.py:180-229 (query offsets grouped by hash; one dedup count per matching row, one
  (sid, db offset - query offset) per matching row and query offset).
- align_matches: afp/dejavu/dejavu.py:312-378 (counts per (sid, diff), per song the first maximum in diff order, songs by
  count descending with ties to the smaller sid, the first topn; every row reports the first song's count).
- recognize: file_recognizer.py:17-75 on a list of (digest, t1) pairs (taken as a set), with the MIN_HASHES rule.
"""
from __future__ import annotations

from collections import defaultdict

import numpy as np

MIN_HASHES = 1


def digest_words(dig: np.ndarray) -> np.ndarray:
    """(N, 10) uint8 -> (N, 3) uint32 big-endian words, bytes 8-9 in the high half of the third."""
    d = np.zeros((dig.shape[0], 12), np.uint8)
    d[:, :10] = dig
    return d.reshape(-1, 3, 4)[:, :, ::-1].copy().view("<u4").reshape(-1, 3)


def store(dig: np.ndarray, sid: np.ndarray, off: np.ndarray) -> np.ndarray:
    """The table of the set of rows, (M, 5) int32."""
    w = digest_words(np.asarray(dig, np.uint8).reshape(-1, 10)).astype(np.int64)
    rows = np.concatenate([w, np.asarray(sid, np.int64).reshape(-1, 1), np.asarray(off, np.int64).reshape(-1, 1)], 1)
    rows = np.unique(rows, axis=0)                 # lexicographic on (w0, w1, w2, sid, off), all non-negative here
    return rows.astype(np.uint32).view(np.int32) if rows.size else np.zeros((0, 5), np.int32)


def index(table: np.ndarray):
    """hash (bytes of the 3 words) -> [(sid, offset)] in table order."""
    idx = defaultdict(list)
    for r in np.asarray(table).tolist():
        idx[tuple(np.array(r[:3], np.int32).view(np.uint32).tolist())].append((r[3], r[4]))
    return idx


def return_matches(idx, pairs):
    """pairs: [(digest bytes (10,), offset)] -> (results [(sid, diff)], dedup {sid: rows})."""
    mapper = {}
    for d, off in pairs:
        mapper.setdefault(bytes(d), []).append(int(off))
    results, dedup = [], {}
    for d, offs in mapper.items():
        key = tuple(digest_words(np.frombuffer(d, np.uint8).reshape(1, 10))[0].tolist())
        for sid, off in idx.get(key, []):
            dedup[sid] = dedup.get(sid, 0) + 1
            results.extend((sid, off - q) for q in offs)
    return results, dedup


def align_matches(results, dedup, topn=1):
    """-> [(sid, offset, count of that song's best offset, hashes_matched, nb_matches_with_offset)]."""
    counts = defaultdict(int)
    for m in results:
        counts[m] += 1
    best = {}
    for (sid, diff) in sorted(counts):
        c = counts[(sid, diff)]
        if sid not in best or c > best[sid][1]:
            best[sid] = (diff, c)
    songs = sorted(best, key=lambda s: (-best[s][1], s))
    rows = [(s, best[s][0], best[s][1], dedup[s]) for s in songs[:topn]]
    return [r + (rows[0][2],) for r in rows]


def recognize(idx, pairs, topn=1):
    """The query as a set of (digest, t1) pairs -> (aligned rows, number of distinct pairs, match flag)."""
    uniq = sorted({(bytes(d), int(t)) for d, t in pairs})
    rows = align_matches(*return_matches(idx, uniq), topn=topn)
    return rows, len(uniq), bool(rows) and rows[0][4] > MIN_HASHES


def report(rows, queried, songs, samplerate=8000, n_hop=256):
    """The reference's per-row fields: [sid, offset, input_total_hashes, fingerprinted_hashes_in_db, hashes_matched,
    nb_matches_with_offset] and [input_confidence, input_confidence_2, fingerprinted_confidence, offset_seconds].
    songs: {sid: total_hashes}."""
    ints, floats = [], []
    for sid, off, _, hm, nb in rows:
        total = songs[sid]
        ints.append([sid, off, queried, total, hm, nb])
        floats.append([round(hm / queried, 2), round(nb / queried, 2), round(hm / total, 2),
                       round(float(off) / samplerate * n_hop, 5)])
    return np.array(ints, np.int64).reshape(-1, 6), np.array(floats, np.float64).reshape(-1, 4)
