#!/usr/bin/env python3
"""bench_knn_probe_matrix.py — knn_probe(matrix=True) (probe_matrix.hip) beside the exact knn_probe on the
same half-store index in the same process: 200 000 x 3 072 and 200 000 x 1 536 half (bench_knn_probe_wide.py's generated
index: 256 lists around random centres) and the GloVe-shaped index bench.py measures, built with store="float16";
P = 10, k = 10, 1 000 and 10 000 queries.  One JSON line per (index, nq): the host clock around the whole call, medians
of --runs runs, the two calls alternating; Recall10@10 of each call against the other; and the largest
|dist_m - dist| / B over the rows both return for the first 200 queries, B = (2d + 8) 2^-24 (|x|^2 + |y|^2 + 2S) +
2^-21 S with S = sum |x_t y_t|.  --trace LEG runs one warm 10 000-query call of each kind on that index and nothing else
(for a kernel-stats run of its own).

    python bench_knn_probe_matrix.py --out profiles/r28/bench_knn_probe_matrix.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
LEGS = {"f16_3072": 3072, "f16_1536": 1536, "glove_f16": 100}


def recall_of(truth, ids):
    return float(np.mean([np.isin(t[t >= 0], g).mean() for t, g in zip(truth, ids)]))


def worst_ratio(qn, data, d, exact, matrix, rows=200):
    """the largest |dist_m - dist| / B over the ids both calls return for the first `rows` queries"""
    worst = 0.0
    for i in range(min(rows, len(qn))):
        both, ia, ib = np.intersect1d(exact[0][i], matrix[0][i], return_indices=True)
        ia, ib = ia[both >= 0], ib[both >= 0]
        if not len(ia):
            continue
        x = qn[i].astype(np.float64)
        Y = data[exact[0][i][ia]].astype(np.float16).astype(np.float64)
        S = (np.abs(x) * np.abs(Y)).sum(axis=1)
        B = (2 * d + 8) * 2.0 ** -24 * ((x ** 2).sum() + (Y ** 2).sum(axis=1) + 2 * S) + 2.0 ** -21 * S
        err = np.abs(matrix[1][i][ib].astype(np.float64) - exact[1][i][ia].astype(np.float64))
        worst = max(worst, float((err / B).max()))
    return worst


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
    from bench_knn_probe_wide import build
    from tinyknn_amd import _lib
    assert _lib.device_count() >= 1, "bench_knn_probe_matrix.py needs a GPU"

    def clock(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        return 1e3 * (time.perf_counter() - t0)

    k, P = args.k, args.probes
    for leg in ([args.trace] if args.trace else args.legs):
        d = LEGS[leg]
        t0 = time.perf_counter()
        if leg == "glove_f16":
            bargs = argparse.Namespace(n=1183514, d=100, n_clusters=1087, seed=10, build_probes=1, metric="angular",
                                       data="glove-like", fit_sample=100000, cache_dir=args.cache_dir)
            ivf, cent = bench.build_index(bargs, torch.device("cuda", 0))
            ivf._dev = None                                             # (the float32 device copy of the build)
            draw = lambda nq, rng: bench.synth_queries(cent, nq, bargs.seed + 1, kind="glove-like").copy()   # noqa: E731
        else:
            ivf, cent = build(args.n, d, "float16", args.n_lists, 27)
            draw = lambda nq, rng: (cent[rng.randint(len(cent), size=nq)]                                    # noqa: E731
                                    + 0.5 * rng.randn(nq, d).astype(np.float32)).astype(np.float32)
        ivf.store = "float16"
        dev = ivf.device_index()
        print(f"# {leg}: built in {time.perf_counter() - t0:.0f} s, store {dev.store}", file=sys.stderr, flush=True)
        rng = np.random.RandomState(28)
        for nq in ([10000] if args.trace else args.nq):
            qn, qp = ivf._prepare(draw(nq, rng))
            call = dict(exact=lambda: dev.knn_probe(qn, qp, k, P), matrix=lambda: dev.knn_probe(qn, qp, k, P, matrix=True))
            exact = dev.knn_probe(qn, qp, k, P, return_distances=True)                      # (warm)
            matrix = dev.knn_probe(qn, qp, k, P, return_distances=True, matrix=True)
            if args.trace:
                print(json.dumps(dict(bench="knn_probe_matrix", leg=leg, trace=True, nq=nq,
                                      exact_ms=clock(call["exact"]), matrix_ms=clock(call["matrix"]))))
                continue
            took = {w: [] for w in call}
            for _ in range(args.runs):                                                      # alternating
                for w, f in call.items():
                    took[w].append(clock(f))
            med = {w: float(np.median(t)) for w, t in took.items()}
            line = dict(bench="knn_probe_matrix", leg=leg, d=d, store=dev.store, rows=len(ivf.data), nq=nq, k=k, n_probes=P,
                        exact_ms=med["exact"], matrix_ms=med["matrix"], exact_over_matrix=med["exact"] / med["matrix"],
                        exact_spread_ms=max(took["exact"]) - min(took["exact"]),
                        recall_matrix_vs_exact=recall_of(exact[0], matrix[0]),
                        recall_exact_vs_matrix=recall_of(matrix[0], exact[0]),
                        worst_err_over_B=worst_ratio(qn, ivf.data, d, exact, matrix), runs=args.runs,
                        exact_ms_runs=took["exact"], matrix_ms_runs=took["matrix"])
            print(json.dumps(line), flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as sink:
                    sink.write(json.dumps(line) + "\n")
        del dev, ivf


if __name__ == "__main__":
    main()
