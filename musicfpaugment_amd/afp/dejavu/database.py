"""Dejavu fingerprint database on MI355X -- drop-in for the PostgreSQLDatabase of afp/dejavu/postgres_database.py.

The reference keeps two Postgres tables: `songs` (song_id SERIAL, name, file SHA-1, total_hashes, fingerprinted) and
`fingerprints` (hash BYTEA, song_id, offset) under UNIQUE(song_id, offset, hash), with a hash index for the lookup
(:239-281).  Here the songs stay on the host and the fingerprints live on the device as one table sorted by
(hash, song_id, offset) with a bucket directory over the leading hash bits (ops.dejavu_store).  Inserted rows
are collected and placed by the store on the next read, so the table's bytes depend only on the set of rows, not on the
order or the batching of the inserts.

Postgres semantics kept: song ids count 1, 2, ... in insertion order and are never reused until `empty()`; duplicate rows
are dropped (ON CONFLICT DO NOTHING); `setup()` deletes the songs never marked fingerprinted together with their rows
(DELETE_UNFINGERPRINTED and the ON DELETE CASCADE), `delete_songs_by_id` the songs it is given in the same way.  The
connection options of the reference's config are not used.

`save` / `load` use a plain .npz (no pickle).  `insert_batch` / `match_batch` are the batched device forms.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from ... import ops


def _hex_digests(hexes) -> np.ndarray:
    raw = []
    for h in hexes:
        b = bytes.fromhex(h)
        if len(b) != 10:
            raise ValueError(f"fingerprint {h!r}: the device table holds 10-byte hashes (sha1 hex[:20], fingerprint.py:211)")
        raw.append(b)
    return np.frombuffer(b"".join(raw), np.uint8).reshape(-1, 10)


class DeviceDatabase(object):
    type = "device"

    def __init__(self, device=None, dirbits: int = ops.DEJAVU_DIRBITS):
        self.device = torch.device(device if device is not None else "cuda")
        self.dirbits = int(dirbits)
        self._hcap = 1 << 15
        self.empty()

    # ------------------------------------------------------------------ BaseDatabase (afp/dejavu/database.py)
    def before_fork(self) -> None:
        pass

    def after_fork(self) -> None:
        pass

    def setup(self) -> None:
        """CREATE ... IF NOT EXISTS (nothing to do) and DELETE_UNFINGERPRINTED (postgres_database.py:27-36, :350-352)."""
        self.delete_unfingerprinted_songs()

    def empty(self) -> None:
        """DROP both tables and create them again: song ids restart at 1."""
        self._songs: Dict[int, dict] = {}
        self._next_sid = 1
        self._table = torch.zeros((0, 5), dtype=torch.int32, device=self.device)
        self._dir: Optional[torch.Tensor] = None
        self._pending: List[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = []

    def delete_unfingerprinted_songs(self) -> None:
        self._delete_songs([sid for sid, s in self._songs.items() if not s["fingerprinted"]])

    def _delete_songs(self, gone: List[int]) -> None:
        """DELETE FROM songs WHERE song_id IN (gone), and the ON DELETE CASCADE of their fingerprints: the rows that stay are
        placed again by the store, so the table's bytes are those of a database that never held the songs."""
        if not gone:
            return
        for sid in gone:
            del self._songs[sid]
        self._flush()
        keep = ~torch.isin(self._table[:, 3], torch.tensor(gone, dtype=torch.int32, device=self.device))
        self._rebuild(self._table[keep])

    def get_num_songs(self) -> int:
        return sum(1 for s in self._songs.values() if s["fingerprinted"])

    def get_num_fingerprints(self) -> int:
        self._flush()
        return int(self._table.shape[0])

    def set_song_fingerprinted(self, song_id) -> None:
        if int(song_id) in self._songs:
            self._songs[int(song_id)]["fingerprinted"] = 1

    def get_songs(self) -> List[Dict[str, str]]:
        return [{"song_id": sid, "song_name": s["song_name"], "file_sha1": s["file_sha1"], "total_hashes": s["total_hashes"]}
                for sid, s in sorted(self._songs.items()) if s["fingerprinted"]]

    def get_song_by_id(self, song_id: int) -> Optional[Dict[str, str]]:
        s = self._songs.get(int(song_id))
        if s is None:
            return None
        return {"song_name": s["song_name"], "file_sha1": s["file_sha1"], "total_hashes": s["total_hashes"]}

    def insert(self, fingerprint: str, song_id: int, offset: int) -> None:
        self.insert_hashes(song_id, [(fingerprint, offset)])

    def insert_song(self, song_name: str, file_hash: str, total_hashes: int) -> int:
        sid = self._next_sid
        if sid > ops.DEJAVU_MAX_SID:
            raise ValueError(f"the device table holds at most {ops.DEJAVU_MAX_SID} song ids (24 bits of the matcher's sort key)")
        self._songs[sid] = {"song_name": song_name, "file_sha1": None if file_hash is None else str(file_hash).upper(),
                            "total_hashes": int(total_hashes), "fingerprinted": 0}
        self._next_sid += 1
        return sid

    def query(self, fingerprint: str = None):
        raise NotImplementedError("row-by-row SELECTs are not on the experiment's path: use return_matches or match_batch")

    def get_iterable_kv_pairs(self):
        raise NotImplementedError("dumping every fingerprint is not on the experiment's path: save() writes the table")

    def delete_songs_by_id(self, song_ids, batch_size: int = 1000) -> None:
        """DELETE_SONGS (postgres_database.py:231-245, :362-364) with the cascade to the fingerprints.  Ids the songs table
        does not hold are ignored, as by SQL's IN; deleted ids are not handed out again (song_id is SERIAL).  batch_size only
        splits the reference's statement: here the whole list is one pass."""
        gone = sorted({int(s) for s in song_ids} & set(self._songs))
        self._delete_songs(gone)

    def insert_hashes(self, song_id: int, hashes, batch_size: int = 1000) -> None:
        """INSERT_FINGERPRINT ... ON CONFLICT DO NOTHING for every (hash hex, offset) (postgres_database.py:156-178)."""
        sid = self._check_sid(song_id)
        hashes = list(hashes)
        if not hashes:
            return
        dig = torch.from_numpy(_hex_digests(h for h, _ in hashes).copy()).to(self.device)
        off = torch.tensor([int(o) for _, o in hashes], dtype=torch.int32, device=self.device)
        self._pending.append((dig, torch.full_like(off, sid), off))

    def return_matches(self, hashes, batch_size: int = 1) -> Tuple[List[Tuple[int, int]], Dict[int, int]]:
        """postgres_database.py:180-229: the (sid, db offset - query offset) of every matching row and query offset of its
        hash, and the number of matching rows per song.  Rows come from mfpa_dejavu_lookup; the list is built on the host."""
        mapper: Dict[str, List[int]] = {}
        for hsh, offset in hashes:
            mapper.setdefault(hsh.upper(), []).append(offset)
        results: List[Tuple[int, int]] = []
        dedup: Dict[int, int] = {}
        self._flush()
        if not mapper or self._table.shape[0] == 0:
            return results, dedup
        keys = list(mapper)
        dig = torch.from_numpy(_hex_digests(keys).copy()).to(self.device)
        ranges = ops.dejavu_lookup(self._table, self._dir, dig).cpu().numpy()
        idx = np.concatenate([np.arange(lo, hi) for lo, hi in ranges] + [np.zeros(0, np.int64)])
        rows = self._table[torch.from_numpy(idx).to(self.device)][:, 3:].cpu().numpy() if idx.size else np.zeros((0, 2), np.int32)
        p = 0
        for key, (lo, hi) in zip(keys, ranges):
            for sid, off in rows[p:p + hi - lo].tolist():
                dedup[sid] = dedup.get(sid, 0) + 1
                results.extend((sid, off - q) for q in mapper[key])
            p += hi - lo
        return results, dedup

    # ------------------------------------------------------------------ device forms
    def insert_batch(self, sids, digests: torch.Tensor, t1: torch.Tensor, counts: torch.Tensor) -> None:
        """Insert the hashes of B songs as mfpa_dejavu_hashes writes them: digests (B,cap,10) uint8, t1 (B,cap) int32,
        counts (B,) valid rows each; sids (B,) the songs' ids (insert_song first)."""
        B, cap = digests.shape[0], digests.shape[1]
        sids = [self._check_sid(s) for s in (sids.tolist() if isinstance(sids, torch.Tensor) else sids)]
        if len(sids) != B or counts.shape != (B,) or t1.shape != (B, cap):
            raise ValueError("one song id and one count per clip, t1 (B, cap)")
        n = counts.to(torch.int64).to(self.device)
        if bool((n < 0).any()) or bool((n > cap).any()):
            raise ValueError("counts must lie in [0, cap] (a negative count flags a clip the hash kernel could not hold)")
        valid = torch.arange(cap, device=self.device)[None, :] < n[:, None]
        sid_t = torch.tensor(sids, dtype=torch.int32, device=self.device)[:, None].expand(B, cap)
        self._pending.append((digests.to(self.device)[valid], sid_t[valid].contiguous(), t1.to(self.device)[valid].contiguous()))

    def match_batch(self, digests: torch.Tensor, t1: torch.Tensor, n: torch.Tensor, k: int = 1):
        """return_matches + align_matches(topn=k) of B queries (each the set of its pairs) on the device -> (rows (B,k,4) int32
        [sid, offset, count, hashes_matched], info (B,4) int32 [n_hits, n_distinct_pairs, rows written, songs hit])."""
        self._flush()
        rows, info, self._hcap = ops.dejavu_match(self._table, self._dir, digests.to(self.device), t1.to(self.device),
                                                  n.to(self.device, torch.int32), k=k, hcap=self._hcap)
        return rows, info

    def count_fingerprints(self, sids) -> List[int]:
        """Rows stored per song id (the size of each song's set of (hash, offset) pairs)."""
        self._flush()
        c = torch.bincount(self._table[:, 3].to(torch.int64), minlength=self._next_sid).cpu().tolist()
        return [c[int(s)] for s in sids]

    def set_total_hashes(self, song_id: int, total_hashes: int) -> None:
        self._songs[self._check_sid(song_id)]["total_hashes"] = int(total_hashes)

    @property
    def table(self) -> torch.Tensor:
        """(M, 5) int32 rows [w0, w1, w2, sid, offset] sorted by (hash, sid, offset)."""
        self._flush()
        return self._table

    @property
    def directory(self) -> torch.Tensor:
        self._flush()
        return self._dir

    def save(self, path: str) -> None:
        self._flush()
        sids = sorted(self._songs)
        s = [self._songs[i] for i in sids]
        with open(path, "wb") as fh:
            np.savez(fh, table=self._table.cpu().numpy(), dirbits=np.int64(self.dirbits), next_sid=np.int64(self._next_sid),
                     song_id=np.array(sids, np.int64), song_name=np.array([x["song_name"] for x in s], dtype=str),
                     file_sha1=np.array(["" if x["file_sha1"] is None else x["file_sha1"] for x in s], dtype=str),
                     total_hashes=np.array([x["total_hashes"] for x in s], np.int64),
                     fingerprinted=np.array([x["fingerprinted"] for x in s], np.int64))

    def load(self, path: str) -> None:
        with np.load(path, allow_pickle=False) as z:
            self.empty()
            self.dirbits = int(z["dirbits"])
            self._next_sid = int(z["next_sid"])
            for i, sid in enumerate(z["song_id"].tolist()):
                self._songs[sid] = {"song_name": str(z["song_name"][i]), "file_sha1": str(z["file_sha1"][i]) or None,
                                    "total_hashes": int(z["total_hashes"][i]), "fingerprinted": int(z["fingerprinted"][i])}
            self._rebuild(torch.from_numpy(z["table"].astype(np.int32)).to(self.device).reshape(-1, 5))

    # ------------------------------------------------------------------ internals
    def _check_sid(self, song_id) -> int:
        sid = int(song_id)
        if sid not in self._songs:
            raise ValueError(f"song id {sid} is not in the songs table (the fingerprints' foreign key)")
        return sid

    def _rebuild(self, table: torch.Tensor) -> None:
        self._pending = [(ops.dejavu_table_digests(table), table[:, 3].contiguous(), table[:, 4].contiguous())]
        self._table = torch.zeros((0, 5), dtype=torch.int32, device=self.device)
        self._dir = None
        self._flush()

    def _flush(self) -> None:
        if not self._pending and self._dir is not None:
            return
        parts = [(ops.dejavu_table_digests(self._table), self._table[:, 3].contiguous(), self._table[:, 4].contiguous())]
        parts += self._pending
        dig = torch.cat([p[0] for p in parts]).contiguous()
        sid = torch.cat([p[1] for p in parts]).contiguous()
        off = torch.cat([p[2] for p in parts]).contiguous()
        self._table, self._dir = ops.dejavu_store(dig, sid, off, self.dirbits)
        self._pending = []
