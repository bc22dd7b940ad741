#!/usr/bin/env python3
"""bench_radius_matrix.py — radius_search(matrix=True) (radius_matrix.hip), every row within a radius over
all rows of a half store on the f16 matrix cores, beside the calls that can answer the same question, in one process:

  f16_1536, f16_3072   200 000 x d half (bench_knn_probe_wide.py's generated index, 256 lists)
  glove                the GloVe-shaped index bench.py measures (1 183 514 x 100), as a half store; and, for orientation,
                       radius_search on the float32 store of the same rows

Per (index, nq, k) the radius of a query is its k-th dist_m (knn_brute_dist(matrix=True)), k = 10 / 100 / 1 000, and
  matrix   radius_brute(matrix=True), the default stage: one tile pass wherever the lists fit
  refill   the same call with RADIUS_MATRIX_STAGE = 1: every tile goes through the second pass — what staging saves
  parent   radius_probe(n_probes = n_lists): the only route the parent has on a wide half store (the rescoring's
           distance, not dist_m: its lists may differ at the boundary)
  knn      knn_brute_dist(k, matrix=True), for orientation
One JSON line each: the host clock around the whole call (it ends in a synchronise), medians of --runs runs, the calls
alternating, every shape warmed; the first k entries of --check lists are compared with knn_brute_dist's ids and bytes.
--trace LEG runs one warm 10 000-query call of the new kind (k = 100) on that index and nothing else (for a
kernel-stats run of its own).

    python bench_radius_matrix.py --out profiles/r30/bench_radius_matrix.jsonl
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
    ap.add_argument("--ks", type=int, nargs="+", default=[10, 100, 1000])
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--n-lists", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--check", type=int, default=50)
    ap.add_argument("--parent-nq", type=int, default=10000, help="the parent's route is timed up to this many queries")
    ap.add_argument("--trace", default="")
    ap.add_argument("--cache-dir", default=os.environ.get("TMPDIR", "/tmp"))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import bench
    from bench_knn_probe_wide import build
    from tinyknn_amd import _lib
    assert _lib.device_count() >= 1, "bench_radius_matrix.py needs a GPU"

    def clock(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        return 1e3 * (time.perf_counter() - t0)

    def staged(dev, stage, f):
        dev.RADIUS_MATRIX_STAGE = stage
        try:
            return f()
        finally:
            dev.RADIUS_MATRIX_STAGE = 0

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
        rng = np.random.RandomState(30)
        for nq in ([10000] if args.trace else args.nq):
            qn, qp = ivf._prepare(draw(nq, rng))
            kmax = 100 if args.trace else max(args.ks)
            truth = dev.knn_brute_dist(qn, kmax, matrix=True)
            for k in ([100] if args.trace else args.ks):
                r = truth[1][:, k - 1].copy()
                lims, ids, dist = dev.radius_brute(qn, r, matrix=True)                          # (warm)
                if args.trace:
                    print(json.dumps(dict(bench="radius_matrix", leg=leg, trace=True, nq=nq, k=k, total=int(lims[-1]),
                                          matrix_ms=clock(lambda: dev.radius_brute(qn, r, matrix=True)))))
                    continue
                same = all(np.array_equal(ids[lims[i]:lims[i] + k], truth[0][i, :k])
                           and dist[lims[i]:lims[i] + k].tobytes() == truth[1][i, :k].tobytes()
                           for i in range(min(args.check, nq)))
                again = staged(dev, 1, lambda: dev.radius_brute(qn, r, matrix=True))
                line = dict(bench="radius_matrix", leg=leg, d=d, rows=len(ivf.data), nq=nq, k=k, runs=args.runs,
                            total=int(lims[-1]), longest=int(np.diff(lims).max()), first_k_are_knn_brute_dist=bool(same),
                            refill_same_bytes=all(a.tobytes() == b.tobytes() for a, b in zip(again, (lims, ids, dist))))
                call = dict(matrix=lambda: dev.radius_brute(qn, r, matrix=True),
                            refill=lambda: staged(dev, 1, lambda: dev.radius_brute(qn, r, matrix=True)),
                            knn=lambda: dev.knn_brute_dist(qn, k, matrix=True))
                if nq <= args.parent_nq:
                    call["parent"] = lambda: dev.radius_probe(qn, qp, r, L)
                    line.update(parent="radius_search(n_probes=n_lists)", parent_total=int(call["parent"]()[0][-1]))
                if dev32 is not None:
                    call["float32"] = lambda: dev32.radius_brute(qn, r)
                    line.update(float32_total=int(call["float32"]()[0][-1]))
                took = {w: [] for w in call}
                for w, f in call.items():                                                       # every shape warmed
                    f()
                for _ in range(args.runs):                                                      # alternating
                    for w, f in call.items():
                        took[w].append(clock(f))
                for w, t in took.items():
                    line.update({f"{w}_ms": float(np.median(t)), f"{w}_ms_runs": t})
                line.update(refill_over_matrix=line["refill_ms"] / line["matrix_ms"])
                if "parent" in took:
                    spread = max(took["parent"]) - min(took["parent"])
                    line.update(parent_over_matrix=line["parent_ms"] / line["matrix_ms"], parent_spread_ms=spread,
                                faster_by_more_than_the_spread=bool(line["parent_ms"] - line["matrix_ms"] > spread))
                print(json.dumps(line), flush=True)
                if args.out:
                    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                    with open(args.out, "a") as sink:
                        sink.write(json.dumps(line) + "\n")
        del dev, ivf, dev32


if __name__ == "__main__":
    main()
