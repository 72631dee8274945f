"""The Dejavu fingerprint store and matcher on the device (csrc/dejavu_match.hip)."""
from __future__ import annotations

import ctypes
from typing import Tuple

import torch

from .._lib import check, lib, ptr, require_gpu, stream


DEJAVU_MAX_SID = (1 << 24) - 1        # song ids are packed into 24 bits of the matcher's sort key
DEJAVU_DIRBITS = 20


def _dejavu_dirbits(directory: torch.Tensor) -> int:
    nd = directory.numel() - 1
    dirbits = nd.bit_length() - 1
    if nd < 2 or nd != 1 << dirbits or directory.dtype != torch.int32:
        raise ValueError("directory must be (2^dirbits + 1,) int32")
    return dirbits


def dejavu_store(digests: torch.Tensor, sids: torch.Tensor, offsets: torch.Tensor, dirbits: int = DEJAVU_DIRBITS):
    """The fingerprints table of the SET of rows (digest (N,10) uint8, song id (N,) int32, offset (N,) int32):
    INSERT ... ON CONFLICT DO NOTHING under UNIQUE(song_id, offset, hash) (postgres_database.py:266-295) -> (table (M,5) int32
    sorted by (hash, sid, offset), directory (2^dirbits + 1,) int32).  Torch orders the rows (three stable sorts, least
    significant key first); deduplication, placement and the directory run in mfpa_dejavu_store."""
    for t, name, dt in ((digests, "digests", torch.uint8), (sids, "sids", torch.int32), (offsets, "offsets", torch.int32)):
        require_gpu(t, name)
        if t.dtype != dt:
            raise TypeError(f"{name} must be {dt}")
    N = digests.shape[0]
    if digests.shape != (N, 10) or sids.shape != (N,) or offsets.shape != (N,):
        raise ValueError("digests must be (N, 10), sids and offsets (N,)")
    dev = digests.device
    if N:
        if int(sids.min()) < 1 or int(sids.max()) > DEJAVU_MAX_SID:
            raise ValueError(f"song ids must lie in [1, {DEJAVU_MAX_SID}] (24 bits of the matcher's sort key)")
        if int(offsets.min()) < 0:
            raise ValueError("offsets must be >= 0")
    d = digests.to(torch.int64)
    hi = (d[:, 0] - 128) * (1 << 56)                       # bytes 0-7 in signed order = their unsigned byte order
    for i in range(1, 8):
        hi = hi + (d[:, i] << (56 - 8 * i))
    mid = (((d[:, 8] << 8) | d[:, 9]) << 24) | sids.to(torch.int64)
    order = torch.sort(offsets.to(torch.int64), stable=True).indices
    order = order[torch.sort(mid[order], stable=True).indices]
    order = order[torch.sort(hi[order], stable=True).indices]
    work = torch.empty(max(1, (N + 255) // 256), dtype=torch.int32, device=dev)
    table = torch.empty((max(N, 1), 5), dtype=torch.int32, device=dev)
    n_rows = torch.zeros(1, dtype=torch.int32, device=dev)
    directory = torch.empty((1 << dirbits) + 1, dtype=torch.int32, device=dev)
    check(lib().mfpa_dejavu_store(ptr(digests.contiguous()), ptr(sids.contiguous()), ptr(offsets.contiguous()), ptr(order),
                                  N, int(dirbits), ptr(work), ptr(table), ptr(n_rows), ptr(directory), stream()),
          "mfpa_dejavu_store")
    return table[: int(n_rows)].clone(), directory


def dejavu_table_digests(table: torch.Tensor) -> torch.Tensor:
    """(M,5) table rows -> their (M,10) uint8 digests (the words are big-endian, the tensors little-endian)."""
    M = table.shape[0]
    return table[:, :3].contiguous().view(torch.uint8).view(M, 3, 4).flip(-1).reshape(M, 12)[:, :10].contiguous()


def dejavu_lookup(table: torch.Tensor, directory: torch.Tensor, digests: torch.Tensor) -> torch.Tensor:
    """Row ranges (n, 2) int32 [first, end) of the table rows carrying each of the (n, 10) uint8 digests."""
    require_gpu(table, "table")
    require_gpu(directory, "directory")
    require_gpu(digests, "digests")
    dirbits = _dejavu_dirbits(directory)
    if digests.dtype != torch.uint8 or digests.dim() != 2 or digests.shape[1] != 10:
        raise ValueError("digests must be (n, 10) uint8")
    n = digests.shape[0]
    ranges = torch.zeros((n, 2), dtype=torch.int32, device=digests.device)
    check(lib().mfpa_dejavu_lookup(ptr(table.contiguous()), ptr(directory), dirbits, ptr(digests.contiguous()), n, ptr(ranges),
                                   stream()), "mfpa_dejavu_lookup")
    return ranges


def dejavu_match_scratch_bytes(cap: int, hcap: int) -> int:
    n = ctypes.c_longlong(0)
    check(lib().mfpa_dejavu_match_scratch_bytes(int(cap), int(hcap), ctypes.addressof(n)), "mfpa_dejavu_match_scratch_bytes")
    return int(n.value)


def dejavu_match(table: torch.Tensor, directory: torch.Tensor, digests: torch.Tensor, t1: torch.Tensor, nq: torch.Tensor,
                 k: int = 1, hcap: int = 1 << 15, scratch_budget: int = 1 << 30) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """return_matches + align_matches (postgres_database.py:180-229, dejavu.py:312-378) for B queries, each the SET of its
    (digest, t1) pairs: digests (B,cap,10) uint8, t1 (B,cap) int32, nq (B,) int32 as mfpa_dejavu_hashes writes them ->
    (rows (B,k,4) int32 [sid, offset, count of the song's best offset, hashes_matched], info (B,4) int32 [n_hits,
    n_distinct_pairs, rows written, songs hit], the hit capacity used).  A query with more hits than the scratch capacity is
    reported by the kernel and the batch runs again with a capacity that holds it: nothing is truncated."""
    for t, name in ((table, "table"), (directory, "directory"), (digests, "digests"), (t1, "t1"), (nq, "nq")):
        require_gpu(t, name)
    dirbits = _dejavu_dirbits(directory)
    if table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] != 5:
        raise ValueError("table must be (M, 5) int32")
    if digests.dtype != torch.uint8 or digests.dim() != 3 or digests.shape[2] != 10:
        raise ValueError("digests must be (B, cap, 10) uint8")
    B, cap = digests.shape[0], digests.shape[1]
    if t1.shape != (B, cap) or t1.dtype != torch.int32 or nq.shape != (B,) or nq.dtype != torch.int32:
        raise ValueError("t1 must be (B, cap) int32 and nq (B,) int32")
    dev = digests.device
    out = torch.zeros((B, k, 4), dtype=torch.int32, device=dev)
    info = torch.zeros((B, 4), dtype=torch.int32, device=dev)
    if B == 0:
        return out, info, hcap
    table = table if table.numel() else torch.zeros((1, 5), dtype=torch.int32, device=dev)   # never read: the directory is empty
    digests, t1, nq = digests.contiguous(), t1.contiguous(), nq.contiguous()
    while True:
        per_q = dejavu_match_scratch_bytes(cap, hcap)
        chunk = max(1, min(B, scratch_budget // per_q))
        scratch = torch.empty(chunk * per_q, dtype=torch.uint8, device=dev)
        for s in range(0, B, chunk):
            e = min(B, s + chunk)
            check(lib().mfpa_dejavu_match(ptr(table), ptr(directory), dirbits, ptr(digests[s:e]), ptr(t1[s:e]), ptr(nq[s:e]),
                                          e - s, cap, hcap, ptr(scratch), k, ptr(out[s:e]), ptr(info[s:e]), stream()),
                  "mfpa_dejavu_match")
        del scratch
        need = int(info[:, 0].max())
        if need <= hcap:
            return out, info, hcap
        if need > 1 << 26:
            raise ValueError(f"a query has {need} table hits: more than the matcher's limit of 2^26 per query")
        while hcap < need:
            hcap <<= 1
