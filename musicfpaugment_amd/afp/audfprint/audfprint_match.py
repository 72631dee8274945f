"""Audfprint matcher on MI355X -- drop-in for afp/audfprint/audfprint_match.py (Matcher).

``match_batch`` is the batched hot path: B query hash lists in hashes_batch's layout -> the top k rows
[id, filtered_count, time_offset, raw_count, orig_rank, 0, 0] of each, all on the device (mfpa_audfprint_match: hit
gathering, per-id counts, candidate ranking, mode extraction and ordering in one kernel).  ``match_hashes``, ``match_file``
and ``file_match_to_msgs`` keep the reference's signatures and results.  Ties of the filtered count, which the reference
leaves to numpy's unstable argsort, are ordered by candidate rank, then mode order.

exact_count and find_time_range raise NotImplementedError (the identification experiment uses neither, and there is no
CPU fallback); sort_by_time and max_returns are host post-processing and behave as in the reference.
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

    def _check_supported(self) -> None:
        if self.exact_count:
            raise NotImplementedError("exact_count=True: only the approximate counts (_approx_match_counts) run on the device")
        if self.find_time_range:
            raise NotImplementedError("find_time_range=True is not implemented on the device")

    def match_batch(self, ht: HashTable, uniq: torch.Tensor, counts: torch.Tensor, k: int = 1):
        """uniq (B, cap, 2) int32 (time, hash), counts (B,) -> (rows (B, k, 7) int32, info (B, 3) int32 = [n_hits, rows
        written, rows in total]) on the device; a query with no rows has info[:, 1] == 0."""
        self._check_supported()
        dev = ht.table.device
        rows, info, self.hit_capacity = ops.audfprint_match(
            ht.table, ht.counts, ht.hashesperid_device(), uniq.to(dev, torch.int32), counts.to(dev, torch.int32), k=k,
            threshcount=self.threshcount, search_depth=self.search_depth, window=self.window,
            max_alignments_per_id=self.max_alignments_per_id, hcap=self.hit_capacity, timebits=ht.maxtimebits)
        return rows, info

    def match_hashes(self, ht: HashTable, hashes, hashesfor: Optional[int] = None) -> Tuple[Any, Any]:
        """audfprint_match.py:322-346: every result row of one query, filtered count descending."""
        self._check_supported()
        if hashesfor is not None:
            raise NotImplementedError("hashesfor (_unique_match_hashes) is not implemented on the device")
        q = np.asarray(hashes, dtype=np.int64).reshape(-1, 2).astype(np.int32)
        dev = ht.table.device
        uq = torch.from_numpy(q).to(dev).reshape(1, -1, 2)
        n = torch.tensor([q.shape[0]], dtype=torch.int32, device=dev)
        if q.shape[0] == 0:
            return np.zeros((0, 7), np.int32), None
        k = 64
        while True:
            rows, info = self.match_batch(ht, uq, n, k=k)
            total = int(info[0, 2])
            if total <= k:
                return rows[0, :total].cpu().numpy(), None
            k = total

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
