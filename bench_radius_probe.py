#!/usr/bin/env python3
"""bench_radius_probe.py — the radius search over the probed lists (IVF.radius_search(n_probes=P),
DeviceIndex.radius_probe) beside the call over all rows (radius_brute) and the k-NN query of the same
probes (query_batch(k, P)), on the GloVe-shaped index bench.py measures (bench.build_index).  --nq queries (1 000 and
10 000); each query's radius is its own k-th smallest `part` value from knn_brute_dist(k), k = 10 / 100 / 1000, so the
brute list holds k rows; P = 1 / 10 / 50.  One JSON line per (nq, k, P); every time is the host clock around the whole
call (each ends with its result on the host), the median of --runs runs, the calls alternating within a run:
  probe_ms       radius_probe, sorted: coarse stage, count pass, fill pass, segmented sort, decode, copy
  unsorted_ms    radius_probe(sort=False)
  count_ms       radius_probe_count: coarse stage and count pass
  brute_ms       radius_brute on the same queries and radii (it does not depend on P; measured in the same runs)
  knn_ms         query_batch(k, P) (null where the index refuses the sizes)
  recall         share of radius_brute's hits that radius_probe lists
  total / brute_total   entries returned
Two more legs at --leg-k / --leg-probes (100 / 10), 1 000 queries: "group" — both calls under group= with 10 random
groups, every query its own (selectivity 0.1), the radii unchanged — and, with --b2, "b2" — an index built with
build(n_probes=2), every row in two lists.

    python bench_radius_probe.py --b2 --out profiles/r25/bench_radius_probe.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def recall_of(brute, probe, N):
    """share of the brute call's (query, row) hits among the probed call's"""
    def keys(res):
        lims, ids, _ = res
        return np.repeat(np.arange(len(lims) - 1, dtype=np.int64), np.diff(lims)) * N + ids
    b = keys(brute)
    return float(np.isin(b, keys(probe)).mean()) if len(b) else 1.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--k", type=int, nargs="+", default=[10, 100, 1000])
    ap.add_argument("--probes", type=int, nargs="+", default=[1, 10, 50])
    ap.add_argument("--leg-k", type=int, default=100)
    ap.add_argument("--leg-probes", type=int, default=10)
    ap.add_argument("--b2", action="store_true")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--n", type=int, default=1183514)
    ap.add_argument("--n-clusters", type=int, default=1087)
    ap.add_argument("--cache-dir", default=os.environ.get("TMPDIR", "/tmp"))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import bench
    from tinyknn_amd import _lib
    assert _lib.device_count() >= 1, "bench_radius_probe.py needs a GPU"
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

    def emit(line):
        print(json.dumps(line), flush=True)
        if sink:
            sink.write(json.dumps(line) + "\n")
            sink.flush()

    def index(build_probes):
        bargs = argparse.Namespace(n=args.n, d=100, n_clusters=args.n_clusters, seed=10, build_probes=build_probes,
                                   metric="angular", data="glove-like", fit_sample=min(100000, args.n),
                                   cache_dir=args.cache_dir)
        ivf, cent = bench.build_index(bargs, device)
        return ivf, cent, bargs

    def measure(leg, ivf, dev, qn, qp, k, P, **kw):
        N, nq = ivf.data.shape[0], len(qn)
        _, part = dev.knn_brute_dist(qn, k)                             # (warm, and the radii)
        radius = part[:, k - 1].copy()

        def knn():
            try:
                return dev.query_batch(qn, qp, k, P)
            except (AssertionError, _lib.TinyKnnHipError):
                return None
        call = dict(probe=lambda: dev.radius_probe(qn, qp, radius, P, **kw),
                    unsorted=lambda: dev.radius_probe(qn, qp, radius, P, sort=False, **kw),
                    count=lambda: dev.radius_probe_count(qn, qp, radius, P, **kw),
                    brute=lambda: dev.radius_brute(qn, radius, **kw))
        if not kw and knn() is not None:
            call["knn"] = knn
        got = {w: f() for w, f in call.items()}                         # (warm: workspaces, code objects)
        took = {w: [] for w in call}
        for _ in range(args.runs):                                      # alternating
            for w, f in call.items():
                took[w].append(clock(f)[0])
        med = {w: float(np.median(t)) for w, t in took.items()}
        lims = got["probe"][0]
        line = dict(bench="radius_probe", leg=leg, nq=nq, k=k, n_probes=P, rows=int(N), total=int(lims[-1]),
                    brute_total=int(got["brute"][0][-1]), longest=int(np.diff(lims).max()),
                    recall=recall_of(got["brute"], got["probe"], N),
                    counts_equal=bool(np.array_equal(got["count"], np.diff(lims))),
                    unsorted_lims_equal=bool(np.array_equal(got["unsorted"][0], lims)), knn_ms=None)
        line.update({f"{w}_ms": m for w, m in med.items()})
        line.update(probe_over_brute=med["probe"] / med["brute"], runs=args.runs)
        line.update({f"{w}_ms_runs": t for w, t in took.items()})
        emit(line)

    ivf, cent, bargs = index(1)
    dev = ivf.device_index()
    rng = np.random.default_rng(0)
    for nq in args.nq:
        qs = bench.synth_queries(cent, nq, bargs.seed + 1, kind="glove-like")
        qn, qp = ivf._prepare(qs.copy())
        for k in args.k:
            for P in args.probes:
                measure("plain", ivf, dev, qn, qp, k, P)
    qs = bench.synth_queries(cent, 1000, bargs.seed + 1, kind="glove-like")
    qn, qp = ivf._prepare(qs.copy())
    ivf.set_groups(rng.integers(0, 10, ivf.data.shape[0]).astype(np.int32))
    measure("group", ivf, dev, qn, qp, args.leg_k, args.leg_probes, group=rng.integers(0, 10, 1000).astype(np.int32))
    ivf.set_groups(None)
    if args.b2:
        dev.close()
        del ivf, dev
        ivf, cent, bargs = index(2)
        qs = bench.synth_queries(cent, 1000, bargs.seed + 1, kind="glove-like")
        qn, qp = ivf._prepare(qs.copy())
        measure("b2", ivf, ivf.device_index(), qn, qp, args.leg_k, args.leg_probes)
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
