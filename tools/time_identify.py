#!/usr/bin/env python3
"""Timing of the identification experiment (testing/audfprint_exps.compute_accuracy_batch) on one MI355X.

Builds a database of synthetic 30-s tracks, then matches 8-s excerpts with shifts = 4, without denoising and with the UNet
(formula weights), and prints one JSON line:
  matcher_qps        queries/s of Matcher.match_batch alone (hash lists precomputed on the device)
  identify_qps       queries/s of the whole run (4 x find_peaks + landmarks per analyzer, twice, plus two matches)
  oracle_cpu_qps     the test oracle's numpy matcher (tests/_identify_oracle.py) on this host, on a subset

--exact / --time-range set Matcher.exact_count / find_time_range for the matcher timing and for the whole run.
--matcher-only stops after the matcher timing; --repeat N takes it N times (matcher_qps_runs; matcher_qps is their median);
--all-modes adds matcher_qps_modes: the same timing for the default, exact, time-range, both, and for the default counts
with hashesfor = 0 (the second gather and sort plus one window: what every extended mode pays before its windows).

Usage:  python tools/time_identify.py [--tracks 2000] [--queries 10000] [--batch 256] [--oracle-queries 50]
                                      [--exact] [--time-range] [--matcher-only] [--repeat 1] [--all-modes]
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

from musicfpaugment_amd import synth  # noqa: E402
from musicfpaugment_amd.afp.audfprint.audfprint_match import Matcher  # noqa: E402
from musicfpaugment_amd.afp.audfprint.peak_extractor import Audfprint_peaks  # noqa: E402
from musicfpaugment_amd.testing.audfprint_exps import compute_accuracy_batch, create_fp_database_batch  # noqa: E402
from musicfpaugment_amd.training.unet import UNet  # noqa: E402
from musicfpaugment_amd.training.weights import formula_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=2000)
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--oracle-queries", type=int, default=50)
    ap.add_argument("--exact", action="store_true")
    ap.add_argument("--time-range", action="store_true")
    ap.add_argument("--matcher-only", action="store_true")
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--all-modes", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    t0 = time.perf_counter()
    tracks = torch.from_numpy(synth.batch(args.tracks, seed=20000, n=240000))
    t_synth = time.perf_counter() - t0
    t0 = time.perf_counter()
    ht = create_fp_database_batch(tracks, ["trk%05d" % i for i in range(args.tracks)], batch=64)
    torch.cuda.synchronize()
    t_db = time.perf_counter() - t0
    rng = np.random.default_rng(0)
    owner = rng.integers(0, args.tracks, args.queries)
    start = rng.integers(0, 240000 - 64000, args.queries)
    built = min(args.queries, 4 * args.batch) if args.matcher_only else args.queries      # the matcher timing reads the first batches only
    queries = torch.stack([tracks[o, s:s + 64000] for o, s in zip(owner[:built].tolist(), start[:built].tolist())])

    an1 = Audfprint_peaks(None, device=dev)
    an1.shifts = 4
    net = UNet(1, 1)
    net.load_state_dict(formula_state_dict(0))
    an2 = Audfprint_peaks(None, denoising=True, denoising_model="unet", unet=net.to(dev).eval(), device=dev)
    an2.shifts = 4

    # matcher alone: hash lists of the first batches precomputed, then matched repeatedly
    m = Matcher()
    m.exact_count, m.find_time_range = args.exact, args.time_range
    nb = min(args.queries, 4 * args.batch)
    lists = []
    with torch.no_grad():
        for s in range(0, nb, args.batch):
            lists.append(an1.hashes_batch(queries[s:s + args.batch].to(dev).contiguous()))
    reps = 3

    def qps(matcher, **kw):
        matcher.match_batch(ht, *lists[0], k=1, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            for uq, n in lists:
                matcher.match_batch(ht, uq, n, k=1, **kw)
        torch.cuda.synchronize()
        return reps * nb / (time.perf_counter() - t0)

    runs = [qps(m) for _ in range(max(1, args.repeat))]
    matcher_qps = float(np.median(runs))
    extra = {"exact_count": args.exact, "find_time_range": args.time_range, "matcher_qps_runs": [round(r, 1) for r in runs]}
    if args.all_modes:
        modes = {}
        for name, ex, tr, kw in (("default", False, False, {}), ("exact", True, False, {}), ("time_range", False, True, {}),
                                 ("both", True, True, {}), ("default_hashesfor0", False, False, {"hashesfor": 0})):
            mm = Matcher()
            mm.exact_count, mm.find_time_range, mm.hit_capacity = ex, tr, m.hit_capacity
            modes[name] = [round(qps(mm, **kw), 1) for _ in range(max(1, args.repeat))]
        extra["matcher_qps_modes"] = modes
    hits = []
    for uq, n in lists:
        _, info = m.match_batch(ht, uq, n, k=1)
        hits.append(info[:, 0].cpu())
    hits = torch.cat(hits).double()
    if args.matcher_only:
        print(json.dumps({
            "tracks": args.tracks, "track_seconds": 30, "queries": args.queries, "query_seconds": 8, "shifts": 4,
            "db_build_s": round(t_db, 2), "synth_s": round(t_synth, 2), "db_hashes": ht.totalhashes(),
            "hits_per_query_mean": round(float(hits.mean()), 1), "hits_per_query_max": int(hits.max()),
            "matcher_qps": round(matcher_qps, 1), **extra, "gpu": torch.cuda.get_device_name(0)}))
        return

    compute_accuracy_batch(queries[: args.batch], owner[: args.batch], ht, an1, an2, batch=args.batch)   # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = compute_accuracy_batch(queries, owner, ht, an1, an2, batch=args.batch, matcher=m)
    torch.cuda.synchronize()
    t_run = time.perf_counter() - t0

    sys.path.insert(0, os.path.join(REPO, "tests"))
    import _identify_oracle as io_
    table = ht.table.cpu().numpy().view(np.uint32)
    counts = ht.counts.cpu().numpy()
    uq, n = lists[0]
    uq, n = uq.cpu().numpy(), n.cpu().numpy()
    k = min(args.oracle_queries, len(n))
    t0 = time.perf_counter()
    for i in range(k):
        io_.match(table, counts, ht.hashesperid, uq[i, : n[i]])
    oracle_qps = k / (time.perf_counter() - t0)
    print(json.dumps({
        "tracks": args.tracks, "track_seconds": 30, "queries": args.queries, "query_seconds": 8, "shifts": 4,
        "db_build_s": round(t_db, 2), "synth_s": round(t_synth, 2), "db_hashes": ht.totalhashes(),
        "hits_per_query_mean": round(float(hits.mean()), 1), "hits_per_query_max": int(hits.max()),
        "matcher_qps": round(matcher_qps, 1), **extra, "identify_qps": round(args.queries / t_run, 1),
        "matcher_share_of_run": round((2 * args.queries / matcher_qps) / t_run, 4),
        "oracle_cpu_qps": round(oracle_qps, 2), "accuracy": res, "gpu": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
