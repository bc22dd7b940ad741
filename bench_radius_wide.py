#!/usr/bin/env python3
"""bench_radius_wide.py — radius_search(wide=True) (radius_wide.hip), every row within a radius over all
rows of a float32 store of any d <= 4096, beside the calls that can answer the same question, in one process:

  f32_1536, f32_3072   200 000 x d float32 (bench_knn_probe_wide.py's generated index, 256 lists)
  glove                the GloVe-shaped index bench.py measures (1 183 514 x 100), float32

Per (index, nq, k) the radius of a query is its k-th part (knn_brute_dist(wide=True)), k = 10 / 100 / 1 000, and
  wide     radius_brute(wide=True), the default stage: one tile pass wherever the lists fit
  unsorted the same call with sort=False
  count    radius_count(wide=True): the count pass alone
  refill   radius_brute(wide=True) with RADIUS_WIDE_STAGE = 1: every tile goes through the second pass
  parent   the wide indexes: radius_probe(n_probes = n_lists), the only route the parent has there (the rescoring's
           distance, not part: its lists may differ at the boundary); glove: the default radius_brute, which must return
           the same bytes
  knn      knn_brute_dist(k, wide=True), for orientation
One JSON line each: the host clock around the whole call (it ends in a synchronise), medians of --runs runs, the calls
alternating, every shape warmed; the first k entries of --check lists are compared with knn_brute_dist's ids and bytes.
--trace LEG runs one warm 10 000-query call of the new kind (k = 100) on that index and nothing else (for a
kernel-stats run of its own).

    python bench_radius_wide.py --out profiles/r32/bench_radius_wide.jsonl
"""
import argparse
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
    ap.add_argument("--ks", type=int, nargs="+", default=[10, 100, 1000])
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--n-lists", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--check", type=int, default=50)
    ap.add_argument("--trace", default="")
    ap.add_argument("--cache-dir", default=os.environ.get("TMPDIR", "/tmp"))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import bench
    from bench_knn_probe_wide import build
    from tinyknn_amd import _lib
    assert _lib.device_count() >= 1, "bench_radius_wide.py needs a GPU"

    def clock(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        return 1e3 * (time.perf_counter() - t0)

    def staged(dev, stage, f):
        dev.RADIUS_WIDE_STAGE = stage
        try:
            return f()
        finally:
            dev.RADIUS_WIDE_STAGE = 0

    def emit(line):
        print(json.dumps(line), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as sink:
                sink.write(json.dumps(line) + "\n")

    def index(leg):
        if leg == "glove":
            bargs = argparse.Namespace(n=1183514, d=100, n_clusters=1087, seed=10, build_probes=1, metric="angular",
                                       data="glove-like", fit_sample=100000, cache_dir=args.cache_dir)
            ivf, cent = bench.build_index(bargs, torch.device("cuda", 0))
            return ivf, lambda nq, rng: bench.synth_queries(cent, nq, bargs.seed + 1, kind="glove-like").copy()
        ivf, cent = build(args.n, LEGS[leg], "float32", args.n_lists, 27)
        return ivf, lambda nq, rng: (cent[rng.randint(len(cent), size=nq)]
                                     + 0.5 * rng.randn(nq, LEGS[leg]).astype(np.float32)).astype(np.float32)

    def timed(call):
        took = {w: [] for w in call}
        for f in call.values():                                                             # every shape warmed
            f()
        for _ in range(args.runs):                                                          # alternating
            for w, f in call.items():
                took[w].append(clock(f))
        return took

    for leg in ([args.trace] if args.trace else args.legs):
        d = LEGS[leg]
        t0 = time.perf_counter()
        ivf, draw = index(leg)
        dev = ivf.device_index()
        L = len(ivf.ids)
        print(f"# {leg}: built in {time.perf_counter() - t0:.0f} s, store {dev.store}", file=sys.stderr, flush=True)
        rng = np.random.RandomState(32)
        for nq in ([10000] if args.trace else args.nq):
            qn, qp = ivf._prepare(draw(nq, rng))
            truth = dev.knn_brute_dist(qn, 100 if args.trace else max(args.ks), wide=True)
            for k in ([100] if args.trace else args.ks):
                r = truth[1][:, k - 1].copy()
                lims, ids, part = dev.radius_brute(qn, r, wide=True)                            # (warm)
                if args.trace:
                    print(json.dumps(dict(bench="radius_wide", leg=leg, trace=True, nq=nq, k=k, total=int(lims[-1]),
                                          wide_ms=clock(lambda: dev.radius_brute(qn, r, wide=True)))))
                    continue
                same = all(np.array_equal(ids[lims[i]:lims[i] + k], truth[0][i, :k])
                           and part[lims[i]:lims[i] + k].tobytes() == truth[1][i, :k].tobytes()
                           for i in range(min(args.check, nq)))
                again = staged(dev, 1, lambda: dev.radius_brute(qn, r, wide=True))
                line = dict(bench="radius_wide", leg=leg, d=d, rows=len(ivf.data), nq=nq, k=k, runs=args.runs,
                            total=int(lims[-1]), longest=int(np.diff(lims).max()), first_k_are_knn_brute_dist=bool(same),
                            refill_same_bytes=all(a.tobytes() == b.tobytes() for a, b in zip(again, (lims, ids, part))))
                call = dict(wide=lambda: dev.radius_brute(qn, r, wide=True),
                            unsorted=lambda: dev.radius_brute(qn, r, wide=True, sort=False),
                            count=lambda: dev.radius_count(qn, r, wide=True),
                            refill=lambda: staged(dev, 1, lambda: dev.radius_brute(qn, r, wide=True)),
                            knn=lambda: dev.knn_brute_dist(qn, k, wide=True))
                if leg == "glove":
                    call["parent"] = lambda: dev.radius_brute(qn, r)
                    line.update(parent="radius_search", parent_same_bytes=all(
                        a.tobytes() == b.tobytes() for a, b in zip(call["parent"](), (lims, ids, part))))
                else:
                    call["parent"] = lambda: dev.radius_probe(qn, qp, r, L)
                    line.update(parent="radius_search(n_probes=n_lists)", parent_total=int(call["parent"]()[0][-1]))
                took = timed(call)
                for w, t in took.items():
                    line.update({f"{w}_ms": float(np.median(t)), f"{w}_ms_runs": t})
                spread = max(took["parent"]) - min(took["parent"])
                line.update(refill_over_wide=line["refill_ms"] / line["wide_ms"],
                            parent_over_wide=line["parent_ms"] / line["wide_ms"], parent_spread_ms=spread,
                            faster_by_more_than_the_spread=bool(line["parent_ms"] - line["wide_ms"] > spread))
                emit(line)
        del dev, ivf


if __name__ == "__main__":
    main()
