#!/usr/bin/env python3
"""bench_knn_brute_matrix.py — knn_brute(matrix=True) (brute_matrix.hip), the exact search over all rows
of a half store on the f16 matrix cores, beside the only call the parent has for the same question, in one process:

  glove      the GloVe-shaped index bench.py measures (1 183 514 x 100): knn_brute(matrix=True) on the half store
             against knn_brute on the float32 store of the same rows; Recall10@10 of each call's ids against the
             other's and the largest |dist_m - part| / B over the rows both return for the first 200 queries
  f16_1536, f16_3072   200 000 x d half (bench_knn_probe_wide.py's generated index, 256 lists): against
             knn_probe(matrix=True, n_probes = n_lists), which must return the same ids and distance bytes; then
             Recall10@10 of knn_probe(P), knn_probe(P, matrix=True) and query_batch(k, P) against the new truth

k = 10, 1 000 queries for both calls, 10 000 for the new call alone (and for both on glove).  One JSON line per (index,
nq): the host clock around the whole call (it ends in a synchronise), medians of --runs runs, the two calls alternating,
every shape warmed.  --trace LEG runs one warm 10 000-query call of the new kind on that index and nothing else (for a
kernel-stats run of its own).

    python bench_knn_brute_matrix.py --out profiles/r29/bench_knn_brute_matrix.jsonl
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
LEGS = {"f16_3072": 3072, "f16_1536": 1536, "glove": 100}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", nargs="+", default=list(LEGS), choices=sorted(LEGS))
    ap.add_argument("--nq", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--n-lists", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--probes", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--trace", default="")
    ap.add_argument("--cache-dir", default=os.environ.get("TMPDIR", "/tmp"))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import bench
    from bench_knn_probe_matrix import recall_of, worst_ratio
    from bench_knn_probe_wide import build
    from tinyknn_amd import _lib
    assert _lib.device_count() >= 1, "bench_knn_brute_matrix.py needs a GPU"

    def clock(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        return 1e3 * (time.perf_counter() - t0)

    k, P = args.k, args.probes
    for leg in ([args.trace] if args.trace else args.legs):
        d = LEGS[leg]
        t0 = time.perf_counter()
        dev32 = None
        if leg == "glove":
            bargs = argparse.Namespace(n=1183514, d=100, n_clusters=1087, seed=10, build_probes=1, metric="angular",
                                       data="glove-like", fit_sample=100000, cache_dir=args.cache_dir)
            ivf32, cent = bench.build_index(bargs, torch.device("cuda", 0))
            dev32 = ivf32.device_index()
            ivf = copy.copy(ivf32)
            ivf._dev = None
            draw = lambda nq, rng: bench.synth_queries(cent, nq, bargs.seed + 1, kind="glove-like").copy()   # noqa: E731
        else:
            ivf, cent = build(args.n, d, "float16", args.n_lists, 27)
            draw = lambda nq, rng: (cent[rng.randint(len(cent), size=nq)]                                    # noqa: E731
                                    + 0.5 * rng.randn(nq, d).astype(np.float32)).astype(np.float32)
        ivf.store = "float16"
        dev = ivf.device_index()
        L = len(ivf.ids)
        print(f"# {leg}: built in {time.perf_counter() - t0:.0f} s, store {dev.store}", file=sys.stderr, flush=True)
        rng = np.random.RandomState(29)
        for nq in ([10000] if args.trace else args.nq):
            qn, qp = ivf._prepare(draw(nq, rng))
            new = dev.knn_brute_dist(qn, k, matrix=True)                                    # (warm)
            if args.trace:
                print(json.dumps(dict(bench="knn_brute_matrix", leg=leg, trace=True, nq=nq,
                                      matrix_ms=clock(lambda: dev.knn_brute(qn, k, matrix=True)))))
                continue
            call = dict(matrix=lambda: dev.knn_brute(qn, k, matrix=True))
            line = dict(bench="knn_brute_matrix", leg=leg, d=d, rows=len(ivf.data), nq=nq, k=k, runs=args.runs)
            if dev32 is not None:
                call["parent"] = lambda: dev32.knn_brute(qn, k)
                old = dev32.knn_brute_dist(qn, k)
                line.update(parent="knn_brute on the float32 store", recall_matrix_vs_parent=recall_of(old[0], new[0]),
                            recall_parent_vs_matrix=recall_of(new[0], old[0]),
                            worst_err_over_B=worst_ratio(qn, ivf.data, d, old, new))
            elif nq <= 1000:
                call["parent"] = lambda: dev.knn_probe(qn, qp, k, L, matrix=True)
                old = dev.knn_probe(qn, qp, k, L, return_distances=True, matrix=True)
                truth = new[0]
                line.update(parent="knn_probe(matrix=True, n_probes=n_lists)", same_ids=bool(np.array_equal(old[0], new[0])),
                            same_distance_bytes=old[1].tobytes() == new[1].tobytes(),
                            recall_knn_probe=recall_of(truth, dev.knn_probe(qn, qp, k, P)),
                            recall_knn_probe_matrix=recall_of(truth, dev.knn_probe(qn, qp, k, P, matrix=True)),
                            recall_query_batch=recall_of(truth, dev.query_batch(qn, qp, k, P)), n_probes=P)
            took = {w: [] for w in call}
            for _ in range(args.runs):                                                      # alternating
                for w, f in call.items():
                    took[w].append(clock(f))
            line.update(matrix_ms=float(np.median(took["matrix"])), matrix_ms_runs=took["matrix"])
            if "parent" in took:
                pm = float(np.median(took["parent"]))
                line.update(parent_ms=pm, parent_over_matrix=pm / line["matrix_ms"], parent_ms_runs=took["parent"],
                            parent_spread_ms=max(took["parent"]) - min(took["parent"]),
                            faster_by_more_than_the_spread=bool(pm - line["matrix_ms"] > max(took["parent"]) - min(took["parent"])))
            print(json.dumps(line), flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as sink:
                    sink.write(json.dumps(line) + "\n")
        del dev, ivf, dev32


if __name__ == "__main__":
    main()
