#!/usr/bin/env python3
"""bench_knn_brute_wide.py — knn_brute(wide=True) (brute_wide.hip), the exact search over all rows of a
float32 store of any d <= 4096, beside the calls the parent has for the same question, in one process:

  f32_1536, f32_3072   200 000 x d float32 (bench_knn_probe_wide.py's generated index, 256 lists): against
             knn_probe(n_probes = n_lists), the parent's only exact route there.  That call ranks by the rescoring's
             distance, not by part, so Recall10@10 of each call's ids against the other's is reported, not byte
             equality.  For information: knn_brute(matrix=True) on the half store of the same rows.
  glove      the GloVe-shaped index bench.py measures (1 183 514 x 100): against the default knn_brute, which must
             return the same ids and distance bytes; the ratio of the times is reported and nothing asked of it.

k = 10, 1 000 and 10 000 queries.  One JSON line per (index, nq): the host clock around the whole call (it ends in a
synchronise), medians of --runs runs, the calls alternating, every shape warmed.  --trace LEG runs one warm
10 000-query call of the new kind on that index and nothing else (for a kernel-stats run of its own).

    python bench_knn_brute_wide.py --out profiles/r31/bench_knn_brute_wide.jsonl
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
LEGS = {"f32_1536": 1536, "f32_3072": 3072, "glove": 100}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", nargs="+", default=list(LEGS), choices=sorted(LEGS))
    ap.add_argument("--nq", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--n-lists", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--trace", default="")
    ap.add_argument("--cache-dir", default=os.environ.get("TMPDIR", "/tmp"))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import bench
    from bench_knn_probe_matrix import recall_of
    from bench_knn_probe_wide import build
    from tinyknn_amd import _lib
    assert _lib.device_count() >= 1, "bench_knn_brute_wide.py needs a GPU"

    def clock(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        return 1e3 * (time.perf_counter() - t0)

    k = args.k
    for leg in ([args.trace] if args.trace else args.legs):
        d = LEGS[leg]
        t0 = time.perf_counter()
        dev16 = None
        if leg == "glove":
            bargs = argparse.Namespace(n=1183514, d=100, n_clusters=1087, seed=10, build_probes=1, metric="angular",
                                       data="glove-like", fit_sample=100000, cache_dir=args.cache_dir)
            ivf, cent = bench.build_index(bargs, torch.device("cuda", 0))
            draw = lambda nq, rng: bench.synth_queries(cent, nq, bargs.seed + 1, kind="glove-like").copy()   # noqa: E731
        else:
            ivf, cent = build(args.n, d, "float32", args.n_lists, 27)
            draw = lambda nq, rng: (cent[rng.randint(len(cent), size=nq)]                                    # noqa: E731
                                    + 0.5 * rng.randn(nq, d).astype(np.float32)).astype(np.float32)
            if not args.trace:
                ivf16 = copy.copy(ivf)
                ivf16._dev, ivf16.store = None, "float16"
                dev16 = ivf16.device_index()
        dev = ivf.device_index()
        L = len(ivf.ids)
        print(f"# {leg}: built in {time.perf_counter() - t0:.0f} s, store {dev.store}", file=sys.stderr, flush=True)
        rng = np.random.RandomState(31)
        for nq in ([10000] if args.trace else args.nq):
            qn, qp = ivf._prepare(draw(nq, rng))
            new = dev.knn_brute_dist(qn, k, wide=True)                                      # (warm)
            if args.trace:
                print(json.dumps(dict(bench="knn_brute_wide", leg=leg, trace=True, nq=nq,
                                      wide_ms=clock(lambda: dev.knn_brute(qn, k, wide=True)))))
                continue
            call = dict(wide=lambda: dev.knn_brute(qn, k, wide=True))
            line = dict(bench="knn_brute_wide", leg=leg, d=d, rows=len(ivf.data), nq=nq, k=k, runs=args.runs)
            if leg == "glove":
                call["parent"] = lambda: dev.knn_brute(qn, k)
                old = dev.knn_brute_dist(qn, k)
                line.update(parent="knn_brute", same_ids=bool(np.array_equal(old[0], new[0])),
                            same_distance_bytes=old[1].tobytes() == new[1].tobytes())
            else:
                call["parent"] = lambda: dev.knn_probe(qn, qp, k, L)
                call["half_matrix"] = lambda: dev16.knn_brute(qn, k, matrix=True)
                old = dev.knn_probe(qn, qp, k, L)
                call["half_matrix"]()                                                       # (warm)
                line.update(parent="knn_probe(n_probes=n_lists)", recall_wide_vs_parent=recall_of(old, new[0]),
                            recall_parent_vs_wide=recall_of(new[0], old))
            took = {w: [] for w in call}
            for _ in range(args.runs):                                                      # alternating
                for w, f in call.items():
                    took[w].append(clock(f))
            pm, spread = float(np.median(took["parent"])), max(took["parent"]) - min(took["parent"])
            line.update(wide_ms=float(np.median(took["wide"])), wide_ms_runs=took["wide"], parent_ms=pm,
                        parent_ms_runs=took["parent"], parent_spread_ms=spread)
            line.update(parent_over_wide=pm / line["wide_ms"],
                        faster_by_more_than_the_spread=bool(pm - line["wide_ms"] > spread))
            if "half_matrix" in took:
                line.update(half_matrix_ms=float(np.median(took["half_matrix"])))
            print(json.dumps(line), flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as sink:
                    sink.write(json.dumps(line) + "\n")
        del dev, ivf, dev16


if __name__ == "__main__":
    main()
