"""Audfprint matcher on MI355X -- drop-in for afp/audfprint/audfprint_match.py (Matcher).

``match_batch`` is the batched hot path: B query hash lists in hashes_batch's layout -> the top k rows
[id, filtered_count, time_offset, raw_count, orig_rank, min_time, max_time] of each, all on the device (hit gathering,
per-id counts, candidate ranking, mode extraction and ordering in one kernel).  ``match_hashes``, ``match_file`` and
``file_match_to_msgs`` keep the reference's signatures and results.  Ties of the filtered count, which the reference
leaves to numpy's unstable argsort, are ordered by candidate rank, then mode order.

The defaults run mfpa_audfprint_match.  exact_count (every local maximum of an id's offset histogram is a mode, counted
by its distinct matching hashes), find_time_range with time_quantile (columns 5-6: where in the query the match lies)
and ``match_hashes(..., hashesfor=k)`` (the matching hashes of result row k) run mfpa_audfprint_match_ex on the device;
they take at most 32768 query rows.  sort_by_time and max_returns are host post-processing and
behave as in the reference.
"""
from __future__ import annotations

from typing import Any, Optional, Tuple

import numpy as np
import torch

from ... import ops
from .hash_table import HashTable


class Matcher(object):
    def __init__(self) -> None:
        self.window = 2
        self.threshcount = 5
        self.max_returns = 1
        self.search_depth = 100
        self.sort_by_time = False
        self.verbose = 1
        self.exact_count = False
        self.find_time_range = False
        self.time_quantile = 0.05
        self.max_alignments_per_id = 100
        self.hit_capacity = 1 << 15           # scratch hits per query; grows (and stays grown) when a query needs more

    def match_batch(self, ht: HashTable, uniq: torch.Tensor, counts: torch.Tensor, k: int = 1, hashesfor: Optional[int] = None):
        """uniq (B, cap, 2) int32 (time, hash), counts (B,) -> (rows (B, k, 7) int32, info (B, 3) int32 = [n_hits, rows
        written, rows in total]) on the device; a query with no rows has info[:, 1] == 0.  With hashesfor = r two more results: (B, n, 2) int32 [time, hash] rows of the
        matching hashes of result row r and their number (B,) int32 per query (-1: no row r)."""
        dev = ht.table.device
        res = ops.audfprint_match(
            ht.table, ht.counts, ht.hashesperid_device(), uniq.to(dev, torch.int32), counts.to(dev, torch.int32), k=k,
            threshcount=self.threshcount, search_depth=self.search_depth, window=self.window,
            max_alignments_per_id=self.max_alignments_per_id, hcap=self.hit_capacity, timebits=ht.maxtimebits,
            exact_count=bool(self.exact_count), find_time_range=bool(self.find_time_range),
            time_quantile=float(self.time_quantile), hashesfor=hashesfor)
        self.hit_capacity = res[2]
        return (res[0], res[1]) + tuple(res[3:])

    def match_hashes(self, ht: HashTable, hashes, hashesfor: Optional[int] = None) -> Tuple[Any, Any]:
        """audfprint_match.py:322-349: every result row of one query, filtered count descending, and with hashesfor = k the
        (n, 2) [time, hash] rows of the matching hashes of row k (IndexError when there is no row k, as in the reference)."""
        q = np.asarray(hashes, dtype=np.int64).reshape(-1, 2).astype(np.int32)
        dev = ht.table.device
        uq = torch.from_numpy(q).to(dev).reshape(1, -1, 2)
        n = torch.tensor([q.shape[0]], dtype=torch.int32, device=dev)
        if q.shape[0] == 0:
            if hashesfor is not None:
                raise IndexError(f"hashesfor={hashesfor}: the query has no result rows")
            return np.zeros((0, 7), np.int32), None
        k = 64
        while True:
            res = self.match_batch(ht, uq, n, k=k, hashesfor=hashesfor)
            total = int(res[1][0, 2])
            if total <= k:
                break
            k = total
        rows = res[0][0, :total].cpu().numpy()
        if hashesfor is None:
            return rows, None
        count = int(res[3][0])
        if count < 0:
            raise IndexError(f"hashesfor={hashesfor}: the query has {total} result rows")
        return rows, res[2][0, :count].cpu().numpy().astype(np.int64)

    def match_file(self, analyzer, ht: HashTable, filename: str) -> Tuple[Any, float, int]:
        q_hashes = analyzer.wavfile2hashes(filename)
        durd = 0.0 if len(q_hashes) == 0 else analyzer.n_hop * q_hashes[-1][0] / analyzer.target_sr
        rslts, _ = self.match_hashes(ht, q_hashes)
        if self.sort_by_time:
            rslts = rslts[np.argsort(-rslts[:, 2], kind="stable"), :]
        return rslts[: self.max_returns, :], durd, len(q_hashes)

    def file_match_to_msgs(self, analyzer, ht: HashTable, qry: str) -> Tuple[str, str, int]:
        """audfprint_match.py:374-435: ("MATCH", name of the last returned row, its filtered count) or ("NOMATCH", "", 0)."""
        rslts, _, _ = self.match_file(analyzer, ht, qry)
        if len(rslts) == 0:
            return "NOMATCH", "", 0
        tophitid, nhashaligned = int(rslts[-1][0]), int(rslts[-1][1])
        return "MATCH", ht.names[tophitid], nhashaligned
