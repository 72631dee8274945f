#!/usr/bin/env python3
"""Timing of HashTable.remove_batch / retrieve on the 2000-track table of DESIGN.md §3.8, on one MI355X.

Fingerprints synthetic 30-s tracks once (hash lists kept on the device), builds the table with store_batch, and prints one
JSON line.  Every timed call is warmed up first and timed as the median of --reps runs, the table restored from a device copy
between runs (not timed).  `*_ms` is the host clock around the method ending in a device synchronise: what the caller waits,
the upload of the id map and the read-back of the counts included.  `*_dev_ms` is device events around the C entry point alone,
its arguments already on the device; there the two read shapes alternate run by run.
  remove1 / remove100   HashTable.remove_batch of 1 / 100 tracks: counts first and the valid prefix of each row (the default)
  *_full                the same with every row read whole (MFPA_MAINTAIN_FULL_ROWS)
  retrieve1 / 100       HashTable.retrieve of one track, retrieve_batch of 100; retrieve1_count: the count walk and its scans
  rebuild*_store_ms     the parent commit's only way: a new table from the kept hash lists without those tracks (store_batch
                        alone), and fingerprint_s, what it costs when the hash lists were not kept
  *_hbm_fraction        bytes the pass has to read (prefix: 4 B per bucket + 4 B per valid entry; full: the whole table and
                        the counts) over the device time, as a fraction of --hbm-tbs (6.29 TB/s measured for a float4 copy)

Usage:  python tools/time_maintain.py [--tracks 2000] [--reps 7]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from musicfpaugment_amd import ops, synth  # noqa: E402
from musicfpaugment_amd._lib import check, lib, ptr, stream  # noqa: E402
from musicfpaugment_amd.afp.audfprint.hash_table import HashTable  # noqa: E402
from musicfpaugment_amd.testing.audfprint_exps import _database_analyzer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--hbm-tbs", type=float, default=6.29)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_maintain.py measures on the MI355X: no GPU, no number")
    dev = torch.device("cuda:0")
    N = args.tracks
    names = ["trk%05d" % i for i in range(N)]
    tracks = torch.from_numpy(synth.batch(N, seed=20000, n=240000))
    analyzer = _database_analyzer(dev, False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lists = []
    with torch.no_grad():
        for s in range(0, N, args.batch):
            uq, n = analyzer.hashes_batch(tracks[s:s + args.batch].to(dev).contiguous(), shifts=1)
            lists.append((uq, n))
    torch.cuda.synchronize()
    fingerprint_s = time.perf_counter() - t0
    cap = max(u.shape[1] for u, _ in lists)
    uq_all = torch.zeros((N, cap, 2), dtype=torch.int32, device=dev)
    n_all = torch.cat([n for _, n in lists])
    for k, (u, _) in enumerate(lists):
        uq_all[k * args.batch: k * args.batch + u.shape[0], : u.shape[1]] = u

    def build(skip=()):
        skip = set(skip)
        keep = [i for i in range(N) if i not in skip]
        ht = HashTable(device=dev)
        for s in range(0, len(keep), args.batch):
            idx = torch.tensor(keep[s:s + args.batch], device=dev)
            ht.store_batch([names[i] for i in keep[s:s + args.batch]], uq_all[idx], n_all[idx])
        return ht

    def clock(fn, before=None):
        """(host ms, device ms) medians of args.reps runs of fn() after one warm-up."""
        host, devt = [], []
        for r in range(args.reps + 1):
            if before is not None:
                before()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r:
                host.append(1e3 * (time.perf_counter() - t0))
                devt.append(e0.elapsed_time(e1))
        return float(np.median(host)), float(np.median(devt)), [round(x, 4) for x in devt]

    rng = np.random.default_rng(1)
    gone1 = [int(rng.integers(0, N))]
    gone100 = sorted(rng.choice(N, min(100, N // 2), replace=False).tolist())
    out = {"tracks": N, "track_seconds": 30, "reps": args.reps, "fingerprint_s": round(fingerprint_s, 2)}

    # the baseline: a new table without the tracks (the build with everything is the warm-up)
    ht = build()
    torch.cuda.synchronize()
    for label, gone in (("rebuild1", gone1), ("rebuild100", gone100)):
        ts = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            other = build(gone)
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
            del other
        out[label + "_store_ms"] = round(float(np.median(ts)), 1)

    table0, counts0 = ht.table.clone(), ht.counts.clone()
    names0, hpid0 = list(ht.names), ht.hashesperid.copy()
    nb, depth = ht.table.shape
    valid = int(torch.clamp(ht.counts, max=depth).sum())
    bytes_prefix, bytes_full = 4 * nb + 4 * valid, 4 * nb * depth + 4 * nb
    out.update(db_hashes=ht.totalhashes(), buckets_used=int(torch.count_nonzero(ht.counts)),
               buckets_overfull=int((ht.counts > depth).sum()), bytes_prefix=bytes_prefix,
               bytes_full=bytes_full, hbm_tbs=args.hbm_tbs)

    def restore():
        ht.table.copy_(table0)
        ht.counts.copy_(counts0)
        ht.names, ht.hashesperid = list(names0), hpid0.copy()

    quiet = open(os.devnull, "w")
    stdout = sys.stdout

    def hbm(nbytes, ms):
        return round(nbytes / (ms * 1e-3) / (args.hbm_tbs * 1e12), 4)

    for label, gone in (("remove1", gone1), ("remove100", gone100)):
        # the whole method, as a user calls it
        sys.stdout = quiet
        try:
            host, _, _ = clock(lambda: ht.remove_batch([names[i] for i in gone]), restore)
        finally:
            sys.stdout = stdout
        out[label + "_ms"] = round(host, 3)
        # the launch alone (the id map already on the device), the two read shapes alternating
        in_set = torch.zeros(N, dtype=torch.uint8, device=dev)
        in_set[torch.tensor(gone, device=dev)] = 1
        removed = torch.empty(N, dtype=torch.int32, device=dev)
        runs = {False: [], True: []}
        for r in range(2 * (args.reps + 1)):
            full = bool(r % 2)
            restore()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            check(lib().mfpa_audfprint_remove(ptr(ht.table), ptr(ht.counts), ht.hashbits, ht.maxtimebits, depth, ptr(in_set), N,
                                              ops.MAINTAIN_FULL_ROWS if full else 0, ptr(removed), stream()), "mfpa_audfprint_remove")
            e1.record()
            torch.cuda.synchronize()
            if r >= 2:
                runs[full].append(e0.elapsed_time(e1))
        if int(counts0.max()) <= depth:                                        # no bucket overflowed: every hash was stored
            assert removed[gone].tolist() == [int(hpid0[i]) for i in gone]
        for full, key in ((False, ""), (True, "_full")):
            ms = float(np.median(runs[full]))
            out[label + key + "_dev_ms"] = round(ms, 4)
            out[label + key + "_dev_runs"] = [round(x, 4) for x in runs[full]]
            out[label + key + "_hbm_fraction"] = hbm(bytes_full if full else bytes_prefix, ms)
    restore()

    host, _, _ = clock(lambda: ht.retrieve(names[gone1[0]]))
    out["retrieve1_ms"] = round(host, 3)
    if int(counts0.max()) <= depth:
        assert len(ht.retrieve(names[gone1[0]])) == int(hpid0[gone1[0]])
    # the count walk and its scans alone (half of a retrieve's reads), the two read shapes alternating
    rank = torch.full((gone1[0] + 1,), -1, dtype=torch.int32, device=dev)
    rank[gone1[0]] = 0
    work = torch.empty(1 << 12, dtype=torch.int32, device=dev)
    offsets = torch.empty(2, dtype=torch.int32, device=dev)
    runs = {False: [], True: []}
    for r in range(2 * (args.reps + 1)):
        full = bool(r % 2)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(lib().mfpa_audfprint_retrieve_count(ptr(ht.table), ptr(ht.counts), ht.hashbits, ht.maxtimebits, depth, ptr(rank),
                                                  rank.numel(), 1, ops.MAINTAIN_FULL_ROWS if full else 0, ptr(work), ptr(offsets),
                                                  stream()), "mfpa_audfprint_retrieve_count")
        e1.record()
        torch.cuda.synchronize()
        if r >= 2:
            runs[full].append(e0.elapsed_time(e1))
    for full, key in ((False, ""), (True, "_full")):
        ms = float(np.median(runs[full]))
        out["retrieve1_count" + key + "_dev_ms"] = round(ms, 4)
        out["retrieve1_count" + key + "_dev_runs"] = [round(x, 4) for x in runs[full]]
        out["retrieve1_count" + key + "_hbm_fraction"] = hbm(bytes_full if full else bytes_prefix, ms)
    host, _, _ = clock(lambda: ht.retrieve_batch([names[i] for i in gone100], on_device=True))
    out["retrieve100_ms"] = round(host, 3)
    out["gpu"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
