#!/usr/bin/env python3
"""Timing of the identification experiment (testing/audfprint_exps.compute_accuracy_batch) on one MI355X.

Builds a database of synthetic 30-s tracks, then matches 8-s excerpts with shifts = 4, without denoising and with the UNet
(formula weights), and prints one JSON line:
  matcher_qps        queries/s of Matcher.match_batch alone (hash lists precomputed on the device)
  identify_qps       queries/s of the whole run (4 x find_peaks + landmarks per analyzer, twice, plus two matches)
  oracle_cpu_qps     the test oracle's numpy matcher (tests/_identify_oracle.py) on this host, on a subset

Usage:  python tools/time_identify.py [--tracks 2000] [--queries 10000] [--batch 256] [--oracle-queries 50]
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
    queries = torch.stack([tracks[o, s:s + 64000] for o, s in zip(owner.tolist(), start.tolist())])

    an1 = Audfprint_peaks(None, device=dev)
    an1.shifts = 4
    net = UNet(1, 1)
    net.load_state_dict(formula_state_dict(0))
    an2 = Audfprint_peaks(None, denoising=True, denoising_model="unet", unet=net.to(dev).eval(), device=dev)
    an2.shifts = 4

    # matcher alone: hash lists of the first batches precomputed, then matched repeatedly
    m = Matcher()
    nb = min(args.queries, 4 * args.batch)
    lists = []
    with torch.no_grad():
        for s in range(0, nb, args.batch):
            lists.append(an1.hashes_batch(queries[s:s + args.batch].to(dev).contiguous()))
    m.match_batch(ht, *lists[0], k=1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps = 3
    for _ in range(reps):
        for uq, n in lists:
            m.match_batch(ht, uq, n, k=1)
    torch.cuda.synchronize()
    matcher_qps = reps * nb / (time.perf_counter() - t0)
    hits = []
    for uq, n in lists:
        _, info = m.match_batch(ht, uq, n, k=1)
        hits.append(info[:, 0].cpu())
    hits = torch.cat(hits).double()

    compute_accuracy_batch(queries[: args.batch], owner[: args.batch], ht, an1, an2, batch=args.batch)   # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = compute_accuracy_batch(queries, owner, ht, an1, an2, batch=args.batch)
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
        "matcher_qps": round(matcher_qps, 1), "identify_qps": round(args.queries / t_run, 1),
        "matcher_share_of_run": round((2 * args.queries / matcher_qps) / t_run, 4),
        "oracle_cpu_qps": round(oracle_qps, 2), "accuracy": res, "gpu": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
