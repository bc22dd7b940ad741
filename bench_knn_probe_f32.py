#!/usr/bin/env python3
"""bench_knn_probe_f32.py — knn_probe(wide=True) (probe_f32.hip) beside the exact knn_probe on the same
float32 index in the same process: 200 000 x 1 536 and 200 000 x 3 072 float32 (bench_knn_probe_wide.py's generated
index: 256 lists around random centres) and the GloVe-shaped float32 index bench.py measures; P = 10, k = 10, 1 000 and
10 000 queries.  One JSON line per (index, nq): the host clock around the whole call, medians of --runs runs after one
warm call each, the two calls alternating; Recall10@10 of each call against the other; and the largest |part - D| / B
over the rows wide=True returns for the first 200 queries, D the float64 distance and
B = (d + 4) 2^-23 (|x|^2 + |y|^2 + 2 sum |x_t y_t|).  --trace LEG runs one warm 10 000-query call of each kind on that
index and nothing else (for a kernel-stats run of its own).
At the GloVe shape (d = 100) the call is bound by its tables, selection and host passes; measured there (MI355X,
profiles/r33): still a gain, 2.48 against 3.84 ms at 10 000 queries, against 9.97 / 18.04 ms at 200 000 x 1 536.

    python bench_knn_probe_f32.py --out profiles/r33/bench_knn_probe_f32.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
LEGS = {"f32_1536": 1536, "f32_3072": 3072, "glove_f32": 100}


def recall_of(truth, ids):
    return float(np.mean([np.isin(t[t >= 0], g).mean() for t, g in zip(truth, ids)]))


def worst_ratio(qn, data, d, wide, rows=200):
    """the largest |part - D| / B over the ids wide=True returns for the first `rows` queries"""
    worst = 0.0
    for i in range(min(rows, len(qn))):
        live = wide[0][i] >= 0
        if not live.any():
            continue
        x, Y = qn[i].astype(np.float64), data[wide[0][i][live]].astype(np.float64)
        D = ((x - Y) ** 2).sum(axis=1)
        B = (d + 4) * 2.0 ** -23 * ((x ** 2).sum() + (Y ** 2).sum(axis=1) + 2 * (np.abs(x) * np.abs(Y)).sum(axis=1))
        worst = max(worst, float((np.abs(wide[1][i][live].astype(np.float64) - D) / B).max()))
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
    assert _lib.device_count() >= 1, "bench_knn_probe_f32.py needs a GPU"

    def clock(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        return 1e3 * (time.perf_counter() - t0)

    k, P = args.k, args.probes
    for leg in ([args.trace] if args.trace else args.legs):
        d = LEGS[leg]
        t0 = time.perf_counter()
        if leg == "glove_f32":
            bargs = argparse.Namespace(n=1183514, d=100, n_clusters=1087, seed=10, build_probes=1, metric="angular",
                                       data="glove-like", fit_sample=100000, cache_dir=args.cache_dir)
            ivf, cent = bench.build_index(bargs, torch.device("cuda", 0))
            draw = lambda nq, rng: bench.synth_queries(cent, nq, bargs.seed + 1, kind="glove-like").copy()   # noqa: E731
        else:
            ivf, cent = build(args.n, d, None, args.n_lists, 27)
            draw = lambda nq, rng: (cent[rng.randint(len(cent), size=nq)]                                    # noqa: E731
                                    + 0.5 * rng.randn(nq, d).astype(np.float32)).astype(np.float32)
        dev = ivf.device_index()
        print(f"# {leg}: built in {time.perf_counter() - t0:.0f} s, store {dev.store}, exact tile {dev.knn_probe_tile()}",
              file=sys.stderr, flush=True)
        rng = np.random.RandomState(33)
        for nq in ([10000] if args.trace else args.nq):
            qn, qp = ivf._prepare(draw(nq, rng))
            call = dict(exact=lambda: dev.knn_probe(qn, qp, k, P), wide=lambda: dev.knn_probe(qn, qp, k, P, wide=True))
            exact = dev.knn_probe(qn, qp, k, P, return_distances=True)                      # (warm)
            wide = dev.knn_probe(qn, qp, k, P, return_distances=True, wide=True)
            if args.trace:
                print(json.dumps(dict(bench="knn_probe_f32", leg=leg, trace=True, nq=nq,
                                      exact_ms=clock(call["exact"]), wide_ms=clock(call["wide"]))))
                continue
            took = {w: [] for w in call}
            for _ in range(args.runs):                                                      # alternating
                for w, f in call.items():
                    took[w].append(clock(f))
            med = {w: float(np.median(t)) for w, t in took.items()}
            line = dict(bench="knn_probe_f32", leg=leg, d=d, store=dev.store, rows=len(ivf.data), nq=nq, k=k, n_probes=P,
                        tile=list(_lib.PROBE_F32_TILE), slab=_lib.PROBE_F32_DS,
                        exact_ms=med["exact"], wide_ms=med["wide"], exact_over_wide=med["exact"] / med["wide"],
                        exact_spread_ms=max(took["exact"]) - min(took["exact"]),
                        wide_spread_ms=max(took["wide"]) - min(took["wide"]),
                        recall_wide_vs_exact=recall_of(exact[0], wide[0]),
                        recall_exact_vs_wide=recall_of(wide[0], exact[0]),
                        worst_err_over_B=worst_ratio(qn, ivf.data, d, wide), runs=args.runs,
                        exact_ms_runs=took["exact"], wide_ms_runs=took["wide"])
            print(json.dumps(line), flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as sink:
                    sink.write(json.dumps(line) + "\n")
        del dev, ivf


if __name__ == "__main__":
    main()
