#!/usr/bin/env python3
"""bench_knn_probe.py — the exact k nearest rows of the probed lists (IVF.knn_probe, DeviceIndex.knn_probe, DESIGN
§3.21) beside the three calls around it, on the GloVe-shaped index bench.py measures (bench.build_index): k = 10,
P = 1 / 10 / 50, --nq queries (1, 1 000 and 10 000).  One JSON line per (nq, P); every time is the host clock around the
whole call (each ends with its result on the host), the median of --runs runs, the calls alternating within a run:
  probe_ms      knn_probe(k, P): coarse stage, pairs by list, distance pass, select pass, copy
  radius_ms     radius_probe(n_probes=P, sort=False) at each query's own k-th knn_probe distance: the same candidates
                walked query-major (the yardstick: radius_over_probe = radius_ms / probe_ms)
  batch_ms      query_batch(k, P): the same lists ranked by PQ estimates
  brute_ms      knn_brute(k): all N rows (it does not depend on P; measured in the same runs)
  recall_probe / recall_batch    Recall10@10 of knn_probe and of query_batch against knn_brute
--trace runs one warm 10 000-query call at P = 10 and nothing else (for a kernel-stats trace of its own).

    python bench_knn_probe.py --out profiles/r26/bench_knn_probe.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def recall_of(truth, ids):
    """share of the truth's ids per row that `ids` holds"""
    return float(np.mean([np.isin(t[t >= 0], g).mean() for t, g in zip(truth, ids)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 1000, 10000])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--probes", type=int, nargs="+", default=[1, 10, 50])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--n", type=int, default=1183514)
    ap.add_argument("--n-clusters", type=int, default=1087)
    ap.add_argument("--cache-dir", default=os.environ.get("TMPDIR", "/tmp"))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import bench
    from tinyknn_amd import _lib
    assert _lib.device_count() >= 1, "bench_knn_probe.py needs a GPU"
    device = torch.device("cuda", 0)
    sink = None
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        sink = open(args.out, "a")

    def clock(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        return 1e3 * (time.perf_counter() - t0), out

    bargs = argparse.Namespace(n=args.n, d=100, n_clusters=args.n_clusters, seed=10, build_probes=1, metric="angular",
                               data="glove-like", fit_sample=min(100000, args.n), cache_dir=args.cache_dir)
    ivf, cent = bench.build_index(bargs, device)
    dev = ivf.device_index()
    k = args.k
    if args.trace:
        qn, qp = ivf._prepare(bench.synth_queries(cent, 10000, bargs.seed + 1, kind="glove-like").copy())
        dev.knn_probe(qn, qp, k, 10)
        print(json.dumps(dict(bench="knn_probe", leg="trace", nq=10000, k=k, n_probes=10,
                              probe_ms=clock(lambda: dev.knn_probe(qn, qp, k, 10))[0], tile=dev.knn_probe_tile())))
        return
    for nq in args.nq:
        qn, qp = ivf._prepare(bench.synth_queries(cent, nq, bargs.seed + 1, kind="glove-like").copy())
        for P in args.probes:
            ids, dist = dev.knn_probe(qn, qp, k, P, return_distances=True)
            radius = dist[:, k - 1].copy()
            call = dict(probe=lambda: dev.knn_probe(qn, qp, k, P),
                        radius=lambda: dev.radius_probe(qn, qp, radius, P, sort=False),
                        batch=lambda: dev.query_batch(qn, qp, k, P),
                        brute=lambda: dev.knn_brute(qn, k))
            got = {w: f() for w, f in call.items()}                         # (warm: workspaces, code objects)
            took = {w: [] for w in call}
            for _ in range(args.runs):                                      # alternating
                for w, f in call.items():
                    took[w].append(clock(f)[0])
            med = {w: float(np.median(t)) for w, t in took.items()}
            line = dict(bench="knn_probe", nq=nq, k=k, n_probes=P, rows=int(ivf.data.shape[0]), tile=dev.knn_probe_tile(),
                        recall_probe=recall_of(got["brute"], got["probe"]), recall_batch=recall_of(got["brute"], got["batch"]),
                        radius_total=int(got["radius"][0][-1]), ids_equal=bool(np.array_equal(got["probe"], ids)))
            line.update({f"{w}_ms": m for w, m in med.items()})
            line.update(radius_over_probe=med["radius"] / med["probe"], brute_over_probe=med["brute"] / med["probe"],
                        runs=args.runs)
            line.update({f"{w}_ms_runs": t for w, t in took.items()})
            print(json.dumps(line), flush=True)
            if sink:
                sink.write(json.dumps(line) + "\n")
                sink.flush()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
