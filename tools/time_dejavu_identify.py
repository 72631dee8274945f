#!/usr/bin/env python3
"""Timing of the Dejavu identification experiment (testing/dejavu_exps.compute_accuracy_batch) on one MI355X.

Builds a database of synthetic 30-s tracks (synth.track: tone bursts in every 8-s window), then matches 8-s excerpts
without denoising and with the UNet (formula weights),
and prints one JSON line:
  store_s              create_fp_database_batch: fingerprints of every track, the store and the directory
  matcher_qps          queries/s of DeviceDatabase.match_batch alone (hashes precomputed on the device)
  identify_qps         queries/s of the whole run (fingerprints by both instances, then two matches per query)
  matcher_share_of_run the two matches' share of that run
  hits_per_query_*     (sid, diff) keys per query, i.e. matching rows x query offsets
  oracle_cpu_qps       the test oracle (tests/_dejavu_oracle.py) on this host, on a subset

Usage:  python tools/time_dejavu_identify.py [--tracks 2000] [--queries 10000] [--batch 256] [--oracle-queries 50]
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
from musicfpaugment_amd.afp.dejavu.dejavu import Dejavu  # noqa: E402
from musicfpaugment_amd.constants import afp_settings  # noqa: E402
from musicfpaugment_amd.testing.dejavu_exps import _clip_hashes, compute_accuracy_batch, create_fp_database_batch  # noqa: E402
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
    tracks = torch.from_numpy(np.stack([synth.track(20000 + i, 240000) for i in range(args.tracks)]))
    t_synth = time.perf_counter() - t0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    db = create_fp_database_batch(tracks, ["trk%05d" % i for i in range(args.tracks)], batch=64)
    n_rows = db.get_num_fingerprints()
    torch.cuda.synchronize()
    t_db = time.perf_counter() - t0
    rng = np.random.default_rng(0)
    owner = rng.integers(0, args.tracks, args.queries)
    start = rng.integers(0, 240000 - 64000, args.queries)
    queries = torch.stack([tracks[o, s:s + 64000] for o, s in zip(owner.tolist(), start.tolist())])

    net = UNet(1, 1)
    net.load_state_dict(formula_state_dict(0))
    djv1 = Dejavu({"database": db}, afp_settings["dejavu"], device=dev)
    djv2 = Dejavu({"database": db}, afp_settings["dejavu"], denoising=True, denoising_model="unet", unet=net.to(dev).eval(),
                  device=dev)

    # matcher alone: hashes of the first batches precomputed, then matched repeatedly
    nb = min(args.queries, 4 * args.batch)
    lists = []
    with torch.no_grad():
        for s in range(0, nb, args.batch):
            lists.append(_clip_hashes(djv1, queries[s:s + args.batch].to(dev).contiguous(), "queries"))
    db.match_batch(*lists[0], k=1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps = 3
    for _ in range(reps):
        for dig, t1, n in lists:
            db.match_batch(dig, t1, n, k=1)
    torch.cuda.synchronize()
    matcher_qps = reps * nb / (time.perf_counter() - t0)
    hits = torch.cat([db.match_batch(*x, k=1)[1][:, 0].cpu() for x in lists]).double()

    gt = owner + 1
    compute_accuracy_batch(queries[: args.batch], gt[: args.batch], db, djv1, djv2, batch=args.batch)   # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = compute_accuracy_batch(queries, gt, db, djv1, djv2, batch=args.batch)
    torch.cuda.synchronize()
    t_run = time.perf_counter() - t0

    sys.path.insert(0, os.path.join(REPO, "tests"))
    import _dejavu_oracle as do
    idx = do.index(db.table.cpu().numpy())
    dig, t1, n = (x.cpu().numpy() for x in lists[0])
    k = min(args.oracle_queries, len(n))
    t0 = time.perf_counter()
    for i in range(k):
        do.recognize(idx, [(bytes(dig[i, j]), int(t1[i, j])) for j in range(n[i])])
    oracle_qps = k / (time.perf_counter() - t0)
    print(json.dumps({
        "tracks": args.tracks, "track_seconds": 30, "queries": args.queries, "query_seconds": 8,
        "store_s": round(t_db, 2), "synth_s": round(t_synth, 2), "db_rows": n_rows,
        "db_distinct_hashes": int(torch.unique(db.table[:, :3], dim=0).shape[0]),
        "hits_per_query_mean": round(float(hits.mean()), 1), "hits_per_query_max": int(hits.max()),
        "matcher_qps": round(matcher_qps, 1), "identify_qps": round(args.queries / t_run, 1),
        "matcher_share_of_run": round((2 * args.queries / matcher_qps) / t_run, 4),
        "oracle_cpu_qps": round(oracle_qps, 2), "accuracy": res, "gpu": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
