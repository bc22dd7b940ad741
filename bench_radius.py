#!/usr/bin/env python3
"""bench_radius.py — every row within a radius of each query (DeviceIndex.radius_brute / radius_count,
tk_index_radius_brute) against the exact k nearest (knn_brute_dist) on the GloVe-shaped index bench.py measures
(bench.build_index), --nq queries (1 000).  Each query's radius is its own k-th smallest part value from
knn_brute_dist(k), k = 10 / 100 / 1000, so every list holds k rows (more where the k-th value is tied) and the
lengths are known.  One JSON line per k; every time is the host clock around the whole call (each ends with its
result on the host), the median of --runs runs, the calls alternating within a run:
  search_ms      radius_brute, sorted: count pass, fill pass, segmented sort, decode, copy
  unsorted_ms    radius_brute(sort=False)
  count_ms       radius_count: the count pass alone
  knn_ms         knn_brute_dist(k) on the same queries — a sampled pass plus one full pass
  group_ms       radius_brute(group=) with 10 random groups, every query its own (selectivity 0.1), the radii unchanged
  knn_group_ms   knn_brute_dist(k, group=) beside it
  total / group_total   entries returned; first_k_equal: every list's first k ids are knn_brute_dist's

    python bench_radius.py --out profiles/r24/bench_radius.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--k", type=int, nargs="+", default=[10, 100, 1000])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--n", type=int, default=1183514)
    ap.add_argument("--n-clusters", type=int, default=1087)
    ap.add_argument("--cache-dir", default=os.environ.get("TMPDIR", "/tmp"))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import bench
    from tinyknn_amd import _lib
    assert _lib.device_count() >= 1, "bench_radius.py needs a GPU"
    device = torch.device("cuda", 0)
    bargs = argparse.Namespace(n=args.n, d=100, n_clusters=args.n_clusters, seed=10, build_probes=1, metric="angular",
                               data="glove-like", fit_sample=min(100000, args.n), cache_dir=args.cache_dir)
    ivf, cent = bench.build_index(bargs, device)
    qs = bench.synth_queries(cent, args.nq, bargs.seed + 1, kind="glove-like")
    qn, _ = ivf._prepare(qs.copy())
    dev = ivf.device_index()
    N, nq = ivf.data.shape[0], args.nq
    rng = np.random.default_rng(0)
    sink = None
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        sink = open(args.out, "a")

    def clock(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        return 1e3 * (time.perf_counter() - t0), out

    groups = rng.integers(0, 10, N).astype(np.int32)
    ivf.set_groups(groups)
    group = rng.integers(0, 10, nq).astype(np.int32)
    for k in args.k:
        ids, part = dev.knn_brute_dist(qn, k)                           # (warm, and the radii)
        radius = part[:, k - 1].copy()
        call = dict(search=lambda: dev.radius_brute(qn, radius),
                    unsorted=lambda: dev.radius_brute(qn, radius, sort=False),
                    count=lambda: dev.radius_count(qn, radius),
                    knn=lambda: dev.knn_brute_dist(qn, k),
                    group=lambda: dev.radius_brute(qn, radius, group=group),
                    knn_group=lambda: dev.knn_brute_dist(qn, k, group=group))
        got = {w: f() for w, f in call.items()}                         # (warm: workspaces, code objects)
        took = {w: [] for w in call}
        for _ in range(args.runs):                                      # alternating
            for w, f in call.items():
                took[w].append(clock(f)[0])
        lims, rids, _ = got["search"]
        first_k = all(np.array_equal(rids[lims[i]:lims[i] + k], ids[i]) for i in range(nq))
        med = {w: float(np.median(t)) for w, t in took.items()}
        line = dict(bench="radius", k=k, nq=nq, rows=int(N), total=int(lims[-1]), group_total=int(got["group"][0][-1]),
                    longest=int(np.diff(lims).max()), first_k_equal=bool(first_k),
                    counts_equal=bool(np.array_equal(got["count"], np.diff(lims))),
                    unsorted_lims_equal=bool(np.array_equal(got["unsorted"][0], lims)),
                    **{f"{w}_ms": m for w, m in med.items()},
                    search_over_knn=med["search"] / med["knn"], count_over_knn=med["count"] / med["knn"],
                    unsorted_over_knn=med["unsorted"] / med["knn"], group_over_knn_group=med["group"] / med["knn_group"],
                    runs=args.runs, **{f"{w}_ms_runs": t for w, t in took.items()})
        print(json.dumps(line), flush=True)
        if sink:
            sink.write(json.dumps(line) + "\n")
            sink.flush()
    if sink:
        sink.close()
    ivf.set_groups(None)


if __name__ == "__main__":
    main()
