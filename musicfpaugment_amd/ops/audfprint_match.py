"""The Audfprint hash table on the device: store, match, remove, retrieve (csrc/match.hip, audfprint_maintain.hip)."""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from .._lib import check, lib, ptr, require_gpu, stream


def audfprint_store(table: torch.Tensor, counts: torch.Tensor, rows: torch.Tensor, ids: torch.Tensor, seed: int = 0,
                    timebits: int = 14) -> None:
    """HashTable.store (hash_table.py:72-113) of N entries in arrival order, in place: table (2^hashbits, depth) int32
    (bit pattern of the reference's uint32), counts (2^hashbits,) int32, rows (N, 2) int32 (time, hash), ids (N,) int32.
    Torch only groups the entries by bucket (a stable sort); the slot assignment and the reservoir step run in the kernel."""
    for t, name in ((table, "table"), (counts, "counts"), (rows, "rows"), (ids, "ids")):
        require_gpu(t, name)
        if t.dtype != torch.int32:
            raise TypeError(f"{name} must be int32")
    nb, depth = table.shape
    hashbits = nb.bit_length() - 1
    if nb != 1 << hashbits or counts.shape != (nb,):
        raise ValueError("table must have 2^hashbits rows and counts one entry per row")
    N = rows.shape[0]
    if rows.shape != (N, 2) or ids.shape != (N,):
        raise ValueError("rows must be (N, 2) and ids (N,)")
    if N == 0:
        return
    bucket = rows[:, 1].to(torch.int64) & (nb - 1)
    sb, order = torch.sort(bucket, stable=True)
    _, seg_counts = torch.unique_consecutive(sb, return_counts=True)
    seg = torch.zeros(seg_counts.numel() + 1, dtype=torch.int32, device=rows.device)
    seg[1:] = torch.cumsum(seg_counts, 0)
    check(lib().mfpa_audfprint_store(ptr(rows.contiguous()), ptr(ids.contiguous()), ptr(order.contiguous()), ptr(seg),
                                     int(seg_counts.numel()), hashbits, timebits, depth, int(seed) & ((1 << 64) - 1),
                                     ptr(table), ptr(counts), stream()), "mfpa_audfprint_store")


def match_scratch_bytes(hcap: int, extended: bool = False) -> int:
    n = ctypes.c_longlong(0)
    name = "mfpa_audfprint_match_ex_scratch_bytes" if extended else "mfpa_audfprint_match_scratch_bytes"
    check(getattr(lib(), name)(int(hcap), ctypes.addressof(n)), name)
    return int(n.value)


def pow2_roundup_mask() -> int:
    """Bit k is set when encpowerof2(2^k) (audfprint_match.py:17-21: int(ceil(log(v) / log(2))) in numpy's float64) is
    k + 1, not k; the extended matcher reproduces encpowerof2 on the device from this mask."""
    mask = 0
    for k in range(32):
        if int(np.ceil(np.log(np.int64(1) << k) / np.log(2))) > k:
            mask |= 1 << k
    return mask


def audfprint_match(table: torch.Tensor, counts: torch.Tensor, hashesperid: torch.Tensor, hashes: torch.Tensor,
                    nq: torch.Tensor, k: int = 1, threshcount: int = 5, search_depth: int = 100, window: int = 2,
                    max_alignments_per_id: int = 100, hcap: int = 1 << 15, timebits: int = 14,
                    scratch_budget: int = 1 << 30, exact_count: bool = False, find_time_range: bool = False,
                    time_quantile: float = 0.05, hashesfor: Optional[int] = None, hashes_cap: int = 2048,
                    extended: Optional[bool] = None):
    """Matcher.match_hashes (audfprint_match.py:322-346) for B queries: hashes (B, cap, 2) int32 (time, hash) with nq (B,)
    valid rows each -> (rows (B, k, 7) int32 sorted by filtered count, info (B, 3) int32 [n_hits, rows written, rows in
    total], the hit capacity used).  A query with more hits than the scratch capacity is reported by the kernel and the
    batch runs again with a capacity that holds it: nothing is truncated.

    exact_count, find_time_range (with time_quantile) and hashesfor go through mfpa_audfprint_match_ex (`extended` forces
    that entry point, or the default one, regardless); they need cap <= 32768.  With hashesfor = r the
    result has two more members: (B, n, 2) int32 rows [time, hash] of the matching hashes of result row r, and (B,) int32
    their number per query (-1: the query has no row r); the buffer grows from hashes_cap until every list fits."""
    for t, name in ((table, "table"), (counts, "counts"), (hashesperid, "hashesperid"), (hashes, "hashes"), (nq, "nq")):
        require_gpu(t, name)
        if t.dtype != torch.int32:
            raise TypeError(f"{name} must be int32")
    nb, depth = table.shape
    hashbits = nb.bit_length() - 1
    if hashes.dim() != 3 or hashes.shape[2] != 2 or nq.shape != (hashes.shape[0],):
        raise ValueError("hashes must be (B, cap, 2) and nq (B,)")
    flags = (1 if exact_count else 0) | (2 if find_time_range else 0)
    if extended is None:
        extended = bool(flags) or hashesfor is not None
    elif not extended and (flags or hashesfor is not None):
        raise ValueError("exact_count, find_time_range and hashesfor need the extended entry point")
    if exact_count and threshcount < 1:
        raise ValueError("exact_count needs threshcount >= 1: with less, empty bins of the dt histogram would be modes")
    if not 0.0 <= time_quantile < 1.0:
        raise ValueError("time_quantile must lie in [0, 1)")
    if hashesfor is not None and hashesfor < 0:
        raise ValueError("hashesfor must be a row index >= 0")
    B, cap = hashes.shape[0], hashes.shape[1]
    if extended and cap > 1 << 15:
        raise ValueError(f"the extended matcher takes at most 32768 rows per query, not {cap}")
    dev = hashes.device
    out = torch.zeros((B, k, 7), dtype=torch.int32, device=dev)
    info = torch.zeros((B, 3), dtype=torch.int32, device=dev)
    want_hashes = hashesfor is not None
    hf = torch.zeros((B, hashes_cap, 2), dtype=torch.int32, device=dev) if want_hashes else None
    hf_n = torch.full((B,), -1, dtype=torch.int32, device=dev) if want_hashes else None

    def done():
        if not want_hashes:
            return out, info, hcap
        return out, info, hcap, hf[:, :max(0, int(hf_n.max())) if B else 0], hf_n

    if B == 0:
        return done()
    hashes, nq = hashes.contiguous(), nq.contiguous()
    p2mask = pow2_roundup_mask() if extended else 0
    while True:
        per_q = match_scratch_bytes(hcap, extended)
        chunk = max(1, min(B, scratch_budget // per_q))
        scratch = torch.empty(chunk * per_q, dtype=torch.uint8, device=dev)
        for s in range(0, B, chunk):
            e = min(B, s + chunk)
            head = (ptr(table), ptr(counts), ptr(hashesperid), hashesperid.numel(), hashbits, timebits, depth, ptr(hashes[s:e]),
                    ptr(nq[s:e]), e - s, cap, threshcount, search_depth, window, max_alignments_per_id)
            tail = (hcap, ptr(scratch), k, ptr(out[s:e]), ptr(info[s:e]), stream())
            if extended:
                check(lib().mfpa_audfprint_match_ex(*head, flags, float(time_quantile), p2mask, hashesfor if want_hashes else -1,
                                                    hf.shape[1] if want_hashes else 0, ptr(hf[s:e]) if want_hashes else None,
                                                    ptr(hf_n[s:e]) if want_hashes else None, *tail), "mfpa_audfprint_match_ex")
            else:
                check(lib().mfpa_audfprint_match(*head, *tail), "mfpa_audfprint_match")
        del scratch
        need = int(info[:, 0].max())
        if need > hcap:
            if need > 1 << 26:
                raise ValueError(f"a query has {need} table hits: more than the matcher's limit of 2^26 per query")
            while hcap < need:
                hcap <<= 1
            continue
        if want_hashes and int(hf_n.max()) > hf.shape[1]:              # a list longer than the buffer: reported, run again
            hf = torch.zeros((B, int(hf_n.max()), 2), dtype=torch.int32, device=dev)
            continue
        return done()


MAINTAIN_FULL_ROWS = 1          # MFPA_MAINTAIN_FULL_ROWS


def _maintain_table(table: torch.Tensor, counts: torch.Tensor):
    for t, name in ((table, "table"), (counts, "counts")):
        require_gpu(t, name)
        if t.dtype != torch.int32:
            raise TypeError(f"{name} must be int32")
    if table.dim() != 2:
        raise ValueError("table must be (2^hashbits, depth)")
    nb, depth = table.shape
    hashbits = nb.bit_length() - 1
    if nb != 1 << hashbits or counts.shape != (nb,):
        raise ValueError("table must have 2^hashbits rows and counts one entry per row")
    return hashbits, depth


def _maintain_ids(ids, limit: Optional[int]) -> np.ndarray:
    a = ids.cpu().numpy() if isinstance(ids, torch.Tensor) else np.asarray(ids)
    if a.size and a.dtype.kind not in "iu":
        raise TypeError("ids must be integers")
    a = a.astype(np.int64).reshape(-1)
    if a.size and (int(a.min()) < 0 or (limit is not None and int(a.max()) >= limit)):
        raise ValueError("ids must lie in [0, n_ids)" if limit is not None else "ids must not be negative")
    return a


def audfprint_remove(table: torch.Tensor, counts: torch.Tensor, ids, n_ids: int, timebits: int = 14,
                     full_rows: bool = False) -> torch.Tensor:
    """HashTable.remove (hash_table.py:277-295) of a SET of ids in one pass over the table, in place -> removed (n_ids,)
    int32, the entries each id had.  The same table and counts as the reference's remove called once per id, in any order
    (mfpa_audfprint_remove; tables whose slots at or beyond min(counts, depth) are zero).  ids: integers in [0, n_ids)."""
    hashbits, depth = _maintain_table(table, counts)
    n_ids = int(n_ids)
    if n_ids < 0:
        raise ValueError("n_ids must not be negative")
    a = _maintain_ids(ids, n_ids)
    removed = torch.zeros(n_ids, dtype=torch.int32, device=table.device)
    if a.size == 0:
        return removed
    in_set = np.zeros(n_ids, np.uint8)
    in_set[a] = 1
    in_set = torch.from_numpy(in_set).to(table.device)
    check(lib().mfpa_audfprint_remove(ptr(table), ptr(counts), hashbits, int(timebits), depth, ptr(in_set), n_ids,
                                      MAINTAIN_FULL_ROWS if full_rows else 0, ptr(removed), stream()), "mfpa_audfprint_remove")
    return removed


def audfprint_retrieve(table: torch.Tensor, counts: torch.Tensor, ids, timebits: int = 14, full_rows: bool = False):
    """HashTable.retrieve (hash_table.py:297-316) of K distinct ids -> (rows (N, 2) int32 (time, hash) of all of them in
    request order, each id's by bucket then slot; offsets (K + 1,) int32: rows[offsets[k]:offsets[k + 1]] are ids[k]'s).
    Both stay on the device; the table is never copied, one integer (N) is read back to size `rows`."""
    hashbits, depth = _maintain_table(table, counts)
    a = _maintain_ids(ids, None)
    K = int(a.size)
    dev = table.device
    if len(np.unique(a)) != K:
        raise ValueError("ids must be distinct")
    if K == 0:
        return torch.zeros((0, 2), dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    n_ids = int(a.max()) + 1
    rank = np.full(n_ids, -1, np.int32)
    rank[a] = np.arange(K, dtype=np.int32)
    rank = torch.from_numpy(rank).to(dev)
    n = ctypes.c_longlong(0)
    check(lib().mfpa_audfprint_retrieve_work_ints(hashbits, K, ctypes.addressof(n)), "mfpa_audfprint_retrieve_work_ints")
    work = torch.empty(int(n.value), dtype=torch.int32, device=dev)
    offsets = torch.empty(K + 1, dtype=torch.int32, device=dev)
    flags = MAINTAIN_FULL_ROWS if full_rows else 0
    head = (ptr(table), ptr(counts), hashbits, int(timebits), depth, ptr(rank), n_ids, K, flags, ptr(work), ptr(offsets))
    check(lib().mfpa_audfprint_retrieve_count(*head, stream()), "mfpa_audfprint_retrieve_count")
    n_rows = int(offsets[K])
    rows = torch.empty((n_rows, 2), dtype=torch.int32, device=dev)
    check(lib().mfpa_audfprint_retrieve(*head, ptr(rows), n_rows, stream()), "mfpa_audfprint_retrieve")
    return rows, offsets
