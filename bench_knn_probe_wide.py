#!/usr/bin/env python3
"""bench_knn_probe_wide.py — knn_probe on wide vectors (probe_dist_wide_kernel) beside the yardstick of
bench_knn_probe.py, radius_probe(n_probes=P, sort=False) at each query's own k-th distance, on generated indexes of about
1.2 GB: 200 000 x 1 536 float32 and 200 000 x 3 072 half, 256 lists around random centres, P = 10, k = 10, 1 000 and
10 000 queries.  One JSON line per (index, nq): the host clock around the whole call, medians of --runs alternating runs.
--trace LEG runs one warm 10 000-query call on that index and nothing else (for a kernel-stats run of its own).

    python bench_knn_probe_wide.py --out profiles/r27/bench_knn_probe_wide.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
LEGS = {"f32_1536": (1536, None), "f16_3072": (3072, "float16")}


def build(n, d, store, n_lists, seed):
    """(ivf, centres): rows 0.5 * N(0, 1) around n_lists centres N(0, 1), the centres set by hand, the PQ rotated to 64
    dims by a matrix that costs O(d) to draw and fitted on 20 000 rows"""
    from tinyknn_amd import IVF, FastPQ
    from tinyknn_amd.fast_pq import dpad
    from tinyknn_amd.utils import pad2
    rng = np.random.RandomState(seed)
    cent = rng.randn(n_lists, d).astype(np.float32)
    X = cent[rng.randint(n_lists, size=n)]
    for a in range(0, n, 20000):                                        # (in place: X is 1.2 - 2.4 GB)
        X[a:a + 20000] += 0.5 * rng.randn(len(X[a:a + 20000]), d).astype(np.float32)
    ivf = IVF("euclidean", n_lists, FastPQ(2))
    ivf.all_centers = cent
    pq = ivf.pq
    P = pad2(X[:20000], 16, dpad * 2)
    pq.R = np.ascontiguousarray(np.linalg.qr(rng.randn(P.shape[1], 64))[0].T)
    P = P @ pq.R.T
    pq.centers = np.array(pq._fit_code(P), dtype=np.float32).transpose(1, 0, 2).reshape(16, P.shape[1])
    pq.sqrt_n_blocks = np.sqrt(P.shape[1] // 2)
    ivf.build(X, n_probes=1, device=False)
    ivf.store = store
    return ivf, cent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", nargs="+", default=sorted(LEGS), choices=sorted(LEGS))
    ap.add_argument("--nq", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--n-lists", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--probes", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--trace", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from tinyknn_amd import _lib
    assert _lib.device_count() >= 1, "bench_knn_probe_wide.py needs a GPU"

    def clock(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        return 1e3 * (time.perf_counter() - t0)

    k, P = args.k, args.probes
    for leg in ([args.trace] if args.trace else args.legs):
        d, store = LEGS[leg]
        t0 = time.perf_counter()
        ivf, cent = build(args.n, d, store, args.n_lists, 27)
        dev = ivf.device_index()
        print(f"# {leg}: built in {time.perf_counter() - t0:.0f} s, store {dev.store}, tile {dev.knn_probe_tile()}",
              file=sys.stderr, flush=True)
        rng = np.random.RandomState(28)
        for nq in ([10000] if args.trace else args.nq):
            Q = cent[rng.randint(len(cent), size=nq)] + 0.5 * rng.randn(nq, d).astype(np.float32)
            qn, qp = ivf._prepare(Q.astype(np.float32))
            ids, dist = dev.knn_probe(qn, qp, k, P, return_distances=True)          # (warm)
            if args.trace:
                print(json.dumps(dict(bench="knn_probe_wide", leg=leg, trace=True, nq=nq,
                                      probe_ms=clock(lambda: dev.knn_probe(qn, qp, k, P)))))
                continue
            radius = dist[:, k - 1].copy()
            call = dict(probe=lambda: dev.knn_probe(qn, qp, k, P),
                        radius=lambda: dev.radius_probe(qn, qp, radius, P, sort=False))
            total = int(call["radius"]()[0][-1])                                    # (warm)
            took = {w: [] for w in call}
            for _ in range(args.runs):                                              # alternating
                for w, f in call.items():
                    took[w].append(clock(f))
            med = {w: float(np.median(t)) for w, t in took.items()}
            line = dict(bench="knn_probe_wide", leg=leg, d=d, store=dev.store, rows=args.n, n_lists=args.n_lists, nq=nq,
                        k=k, n_probes=P, tile=dev.knn_probe_tile(), radius_total=total, probe_ms=med["probe"],
                        radius_ms=med["radius"], radius_over_probe=med["radius"] / med["probe"], runs=args.runs,
                        probe_ms_runs=took["probe"], radius_ms_runs=took["radius"])
            print(json.dumps(line), flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as sink:
                    sink.write(json.dumps(line) + "\n")
        del dev, ivf


if __name__ == "__main__":
    main()
