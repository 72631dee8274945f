"""Audfprint hash table on MI355X -- drop-in for afp/audfprint/hash_table.py (HashTable).

The table ((2^20, 100) values ((id + 1) << 14) | (time & 16383), the reference's uint32 held as int32) and the per-bucket
counts live on the device; names and hashesperid stay on the host like the reference's, with a device copy of hashesperid
for the matcher.  ``store`` / ``store_batch`` run mfpa_audfprint_store: slots are arrival ranks exactly as in the reference,
and a full bucket's reservoir slot comes from a counter-based draw keyed by (seed, bucket, arrival index) instead of
Python's global `random`, so two ingests of the same input give the same table.

``remove`` / ``remove_batch`` and ``retrieve`` / ``retrieve_batch`` (hash_table.py:277-316) run on the device too
(mfpa_audfprint_remove, mfpa_audfprint_retrieve): one pass over the table for any number of tracks, the table never leaves the
device, results equal the reference's bit for bit.

``save`` writes the reference's gzip-pickle layout under the class path ``afp.audfprint.hash_table.HashTable`` (the
reference loads it), ``load`` reads a file the reference's ``HashTable.save`` wrote.
"""
from __future__ import annotations

import gzip
import pickle
import sys
import types
from typing import Any, Callable, List, Optional, Union

import numpy as np
import torch

from ... import ops

HT_VERSION = 20170724
HT_OLD_COMPAT_VERSION = 20140920
REF_MODULE, REF_CLASS = "afp.audfprint.hash_table", "HashTable"
basestring = (str, bytes)


class _Attrs(object):
    """Plain attribute holder for the state of a pickled reference HashTable."""

    def __setstate__(self, state):
        self.__dict__.update(state)


class _RefUnpickler(pickle.Unpickler):
    def find_class(self, module, name):
        if (module, name) == (REF_MODULE, REF_CLASS):
            return _Attrs
        return super().find_class(module, name)


def _ref_class():
    """A class whose pickle path is the reference's, for `save` (installed in sys.modules only while pickling)."""
    cls = type(REF_CLASS, (object,), {})
    cls.__module__ = REF_MODULE
    return cls


class HashTable(object):
    def __init__(self, filename: Optional[str] = None, device=None, seed: int = 0):
        self.device = torch.device(device if device is not None else "cuda")
        self.seed = int(seed)
        self._hpid_dev = None
        if filename is not None:
            self.load(filename)
        else:
            self.hashbits = 20
            self.depth = 100
            self.maxtimebits = 14
            size = 2 ** self.hashbits
            self.table = torch.zeros((size, self.depth), dtype=torch.int32, device=self.device)
            self.counts = torch.zeros(size, dtype=torch.int32, device=self.device)
            self.names: List[Any] = []
            self.hashesperid = np.zeros(0, np.uint32)
            self.ht_version = HT_VERSION
            self.dirty = True

    # ------------------------------------------------------------------ ids
    def max_ids(self) -> int:
        """(id + 1) << maxtimebits must fit the table's 32-bit values: at most 2^(32 - maxtimebits) - 1 ids (2^18 - 1)."""
        return (1 << (32 - self.maxtimebits)) - 1

    def name_to_id(self, name: Union[int, str], add_if_missing: bool = False) -> int:
        if isinstance(name, basestring):
            if name not in self.names:
                if not add_if_missing:
                    raise ValueError("name " + name + " not found")
                try:
                    id_ = self.names.index(None)
                    self.names[id_] = name
                    self.hashesperid[id_] = 0
                except ValueError:
                    if len(self.names) >= self.max_ids():
                        raise ValueError(f"the table holds at most {self.max_ids()} ids ((id + 1) << {self.maxtimebits} "
                                         "must fit 32 bits)")
                    self.names.append(name)
                    self.hashesperid = np.append(self.hashesperid, [0]).astype(np.uint32)
                self._hpid_dev = None
            return self.names.index(name)
        return int(name)

    def hashesperid_device(self) -> torch.Tensor:
        if self._hpid_dev is None or self._hpid_dev.numel() != len(self.hashesperid):
            self._hpid_dev = torch.from_numpy(np.asarray(self.hashesperid).astype(np.int32)).to(self.device)
        return self._hpid_dev

    # ------------------------------------------------------------------ store
    def store(self, name: Union[int, str], timehashpairs) -> None:
        """hash_table.py:72-113 for one track: (n, 2) (time, hash) rows in arrival order."""
        id_ = self.name_to_id(name, add_if_missing=True)
        rows = torch.as_tensor(np.asarray(timehashpairs, dtype=np.int64).reshape(-1, 2).astype(np.int32))
        self._store_rows(rows.to(self.device), torch.full((rows.shape[0],), id_, dtype=torch.int32, device=self.device))
        self.hashesperid[id_] += rows.shape[0]
        self._hpid_dev = None
        self.dirty = True

    def store_batch(self, names, uniq: torch.Tensor, counts: torch.Tensor) -> None:
        """Store B tracks in order from hashes_batch's output: uniq (B, cap, 2) int32 (time, hash), counts (B,) rows each."""
        B = uniq.shape[0]
        if len(names) != B or counts.shape != (B,):
            raise ValueError("one name and one count per track")
        ids = [self.name_to_id(n, add_if_missing=True) for n in names]
        n = counts.to(torch.int64).cpu()
        if bool((n < 0).any()) or bool((n > uniq.shape[1]).any()):
            raise ValueError("counts must lie in [0, cap] (a negative count flags a clip the landmark kernel could not hold)")
        uniq = uniq.to(self.device)
        valid = torch.arange(uniq.shape[1], device=self.device)[None, :] < n.to(self.device)[:, None]
        rows = uniq[valid].contiguous()                                      # row-major: track order, then row order
        ids_t = torch.repeat_interleave(torch.tensor(ids, dtype=torch.int32, device=self.device), n.to(self.device))
        self._store_rows(rows, ids_t)
        for id_, k in zip(ids, n.tolist()):
            self.hashesperid[id_] += k
        self._hpid_dev = None
        self.dirty = True

    def _store_rows(self, rows: torch.Tensor, ids: torch.Tensor) -> None:
        ops.audfprint_store(self.table, self.counts, rows.to(torch.int32).contiguous(), ids.contiguous(), self.seed,
                            self.maxtimebits)

    # ------------------------------------------------------------------ lookup
    def get_entry(self, hash_: int) -> np.ndarray:
        c = min(self.depth, int(self.counts[hash_]))
        vals = self.table[hash_, :c].cpu().numpy().view(np.uint32)
        return np.c_[(vals >> self.maxtimebits) - 1, vals & ((1 << self.maxtimebits) - 1)].astype(np.int32)

    def get_hits(self, hashes) -> np.ndarray:
        """hash_table.py:222-247: [id, delta_time, hash, time] rows of each (time, hash) query row, in query order (host
        assembly of the rows the query's buckets hold; the matcher gathers its hits on the device itself)."""
        q = np.asarray(hashes, dtype=np.int64).reshape(-1, 2)
        if q.shape[0] == 0:
            return np.zeros((0, 4), np.int32)
        h = q[:, 1] & ((1 << self.hashbits) - 1)
        hi = torch.from_numpy(h).to(self.device)
        vals = self.table[hi].cpu().numpy().view(np.uint32).astype(np.int64)
        nids = np.minimum(self.depth, self.counts[hi].cpu().numpy().astype(np.int64))
        keep = np.arange(self.depth)[None, :] < nids[:, None]
        v = vals[keep]
        rep = np.repeat(np.arange(q.shape[0]), nids)
        out = np.zeros((v.size, 4), np.int32)
        out[:, 0] = (v >> self.maxtimebits) - 1
        out[:, 1] = (v & ((1 << self.maxtimebits) - 1)) - q[rep, 0]
        out[:, 2] = h[rep]
        out[:, 3] = q[rep, 0]
        return out

    def totalhashes(self):
        return int(self.counts.to(torch.int64).sum())

    # ------------------------------------------------------------------ files
    def _report(self, verb: str, name: str) -> None:
        c = self.counts.to(torch.int64)
        nhashes = int(c.sum())
        dropped = nhashes - int(torch.clamp(c, max=self.depth).sum())
        print(verb, "fprints for", sum(n is not None for n in self.names), "files (", nhashes, "hashes)",
              "to" if verb == "Saved" else "from", name, "(%.2f%% dropped)" % (100.0 * dropped / max(1, nhashes)))

    def save(self, name: str) -> None:
        """The reference's gzip pickle (HIGHEST_PROTOCOL) of an afp.audfprint.hash_table.HashTable."""
        cls = _ref_class()
        obj = cls.__new__(cls)
        obj.__dict__.update(hashbits=self.hashbits, depth=self.depth, maxtimebits=self.maxtimebits,
                            table=self.table.cpu().numpy().view(np.uint32), counts=self.counts.cpu().numpy(),
                            names=list(self.names), hashesperid=np.asarray(self.hashesperid, np.uint32),
                            ht_version=self.ht_version, dirty=False)
        parts = REF_MODULE.split(".")
        added = []
        for i in range(len(parts)):
            mod = ".".join(parts[: i + 1])
            if mod not in sys.modules:
                sys.modules[mod] = types.ModuleType(mod)
                added.append(mod)
        saved = getattr(sys.modules[REF_MODULE], REF_CLASS, None)
        setattr(sys.modules[REF_MODULE], REF_CLASS, cls)
        try:
            with gzip.open(name, "wb") as f:
                pickle.dump(obj, f, pickle.HIGHEST_PROTOCOL)
        finally:
            if saved is None:
                delattr(sys.modules[REF_MODULE], REF_CLASS)
            else:
                setattr(sys.modules[REF_MODULE], REF_CLASS, saved)
            for mod in reversed(added):
                del sys.modules[mod]
        self.dirty = False
        self._report("Saved", name)

    def load(self, name: str) -> None:
        self.load_pkl(name)
        self._report("Read", name)

    def load_pkl(self, name: str, file_object: Any = None) -> None:
        f = file_object if file_object else gzip.open(name, "rb")
        try:
            temp = _RefUnpickler(f, encoding="latin1").load()
        finally:
            if not file_object:
                f.close()
        if temp.ht_version < HT_OLD_COMPAT_VERSION:
            raise ValueError(f"Version of {name} is {temp.ht_version} which is not at least {HT_OLD_COMPAT_VERSION}")
        self.hashbits = temp.hashbits
        self.depth = temp.depth
        self.maxtimebits = temp.maxtimebits if hasattr(temp, "maxtimebits") else int(round(np.log2(temp.maxtime)))
        table = np.ascontiguousarray(temp.table, dtype=np.uint32)
        if temp.ht_version < HT_VERSION:                      # hash_table.py:186-193: ids offset by one in older files
            table = table + np.uint32(1 << self.maxtimebits) * (table != 0)
        self.table = torch.from_numpy(table.view(np.int32)).to(self.device)
        self.counts = torch.from_numpy(np.ascontiguousarray(temp.counts, dtype=np.int32)).to(self.device)
        self.ht_version = HT_VERSION
        self.names = list(temp.names)
        self.hashesperid = np.array(temp.hashesperid).astype(np.uint32)
        self._hpid_dev = None
        self.dirty = False

    def reset(self) -> None:
        self.table.zero_()
        self.counts.zero_()
        self.names = []
        self.hashesperid = np.zeros(0, np.uint32)
        self._hpid_dev = None
        self.dirty = True

    # ------------------------------------------------------------------ maintenance
    def _known_id(self, name: Union[int, str]) -> int:
        """name_to_id without adding: an unknown name raises ValueError, an integer id outside the names list IndexError
        (the reference's names[id_])."""
        id_ = self.name_to_id(name)
        if not 0 <= id_ < len(self.names):
            raise IndexError(f"id {id_} is not in the table's {len(self.names)} ids")
        return id_

    def remove(self, name: Union[int, str]) -> None:
        """hash_table.py:277-295: drop every entry of the track and free its id (the next new name takes it)."""
        self.remove_batch([name])

    def remove_batch(self, names) -> List[int]:
        """`remove` of every name (or integer id) of the list in ONE pass over the table -> the entries each one had.  The
        table, counts, names and hashesperid are what the reference's remove, called once per name, leaves."""
        names = list(names)
        ids = [self._known_id(n) for n in names]
        removed = ops.audfprint_remove(self.table, self.counts, sorted(set(ids)), len(self.names), self.maxtimebits)
        removed = removed.cpu().tolist() if ids else []
        for id_ in ids:
            self.names[id_] = None
            self.hashesperid[id_] = 0
        self._hpid_dev = None
        self.dirty = True
        out = [removed[id_] for id_ in ids]
        for name, n in zip(names, out):
            print("Removed", name, "(", n, "hashes).")
        return out

    def retrieve(self, name: Union[int, str]) -> np.ndarray:
        """hash_table.py:297-316: the (time, hash) rows the table holds of the track, (n, 2) int32, by hash then slot."""
        return self.retrieve_batch([name])[0]

    def retrieve_batch(self, names, on_device: bool = False):
        """`retrieve` of every name (or integer id) of the list in one count and one scatter pass -> a list of (n, 2) int32
        arrays; with on_device, (rows (N, 2), offsets (len(names) + 1,)) int32 tensors instead: rows[offsets[k]:offsets[k + 1]]
        are names[k]'s (the names must then be distinct)."""
        ids = [self._known_id(n) for n in names]
        uniq = sorted(set(ids))
        if on_device:
            if len(uniq) != len(ids):
                raise ValueError("retrieve_batch(on_device=True) needs distinct names")
            return ops.audfprint_retrieve(self.table, self.counts, ids, self.maxtimebits)
        rows, offsets = ops.audfprint_retrieve(self.table, self.counts, uniq, self.maxtimebits)
        rows, offsets = rows.cpu().numpy(), offsets.cpu().numpy()
        at = {id_: k for k, id_ in enumerate(uniq)}
        return [rows[offsets[at[id_]]:offsets[at[id_] + 1]].copy() for id_ in ids]

    def list(self, print_fn: Optional[Callable[[str], None]] = None) -> None:
        print_fn = print_fn or print
        for name, count in zip(self.names, self.hashesperid):
            if name:
                print_fn(name + " (" + str(count) + " hashes)")
