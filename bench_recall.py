#!/usr/bin/env python3
"""bench_recall.py — Recall10@10 of restricted queries against the restricted exact search (DeviceIndex.knn_brute with
allowed= / group= / tags= / between=, tk_index_knn_brute_ex) on the GloVe-shaped index bench.py measures
(bench.build_index), and what the restriction costs the exact search itself.
One JSON line per (restriction, selectivity), selectivity 0.5 / 0.1 / 0.01 / 0.001, over --nq queries, k 10:
  recall_np10 / recall_np50   mean over the queries of |query_batch's ids ∩ truth| / (truth ids that are not -1), for
                 query_batch(n_probes=10) and n_probes=50 under the same restriction
  answered_np10 / answered_np50   the share of query_batch's k slots that hold an id (the rest are -1)
  passing        the mean number of rows a query's restriction passes
  brute_ms       the restricted knn_brute call for the --nq queries: host clock around the call (it ends in a device
                 synchronise and the copy of the ids), median of --runs runs alternating with ...
  brute_ms_none  ... the unrestricted call (tk_index_knn_brute, the kernels as they were) on the same queries
How the restrictions reach a selectivity s: allowed — one random mask of share s for every query; group — round(1 / s)
random groups, every query its own; tags — four tags carried by a share 0.5 / 0.1 / 0.01 / 0.001 of the rows, every
query the one of share s; between — one uniform float32 column, every query its own window of width s.

    python bench_recall.py --out profiles/r20/bench_recall.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

SHARES = (0.5, 0.1, 0.01, 0.001)


def recall(got, truth):
    """mean over the queries of |got ∩ truth| / (ids of truth that are not -1); queries without a true id left out"""
    per = [len(set(g[g >= 0]) & set(t[t >= 0])) / (t >= 0).sum() for g, t in zip(got, truth) if (t >= 0).any()]
    return float(np.mean(per))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--cache-dir", default=os.environ.get("TMPDIR", "/tmp"))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import bench
    from tinyknn_amd import _lib
    assert _lib.device_count() >= 1, "bench_recall.py needs a GPU"
    device = torch.device("cuda", 0)
    bargs = argparse.Namespace(n=1183514, d=100, n_clusters=1087, seed=10, build_probes=1, metric="angular",
                               data="glove-like", fit_sample=100000, cache_dir=args.cache_dir)
    ivf, cent = bench.build_index(bargs, device)
    qs = bench.synth_queries(cent, args.nq, bargs.seed + 1, kind="glove-like")
    qn, qp = ivf._prepare(qs.copy())
    dev = ivf.device_index()
    N, nq, k = ivf.data.shape[0], args.nq, args.k
    rng = np.random.default_rng(0)
    sink = None
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        sink = open(args.out, "a")

    # the rows' attributes: four tags of the four shares, one uniform column; groups are set per share below
    u = rng.random((N, len(SHARES)))
    row_tags = np.zeros(N, dtype=np.uint64)
    for b, s in enumerate(SHARES):
        row_tags |= (u[:, b] < s).astype(np.uint64) << np.uint64(b)
    ivf.set_tags(row_tags)
    column = rng.random(N).astype(np.float32)
    ivf.set_values(column)

    def restriction(kind, b, s):
        """(keywords of knn_brute / query_batch, mean passing rows)"""
        if kind == "allowed":
            mask = rng.random(N) < s
            return dict(allowed=mask), float(mask.sum())
        if kind == "group":
            n_groups = int(round(1 / s))
            groups = rng.integers(0, n_groups, N).astype(np.int32)
            ivf.set_groups(groups)
            group = rng.integers(0, n_groups, nq).astype(np.int32)
            return dict(group=group), float(np.bincount(groups, minlength=n_groups)[group].mean())
        if kind == "tags":
            return dict(tags=1 << b, tags_mode="any"), float((row_tags >> np.uint64(b) & np.uint64(1)).sum())
        lo = (rng.random(nq) * (1 - s)).astype(np.float32)
        hi = (lo + np.float32(s)).astype(np.float32)
        order = np.sort(column)
        passing = np.searchsorted(order, hi, "right") - np.searchsorted(order, lo, "left")
        return dict(between=(lo, hi)), float(passing.mean())

    def timed(**kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev.knn_brute(qn, k, **kw)
        return 1e3 * (time.perf_counter() - t0)

    dev.knn_brute(qn, k)                                            # (warm: workspaces, code objects)
    for kind in ("allowed", "group", "tags", "between"):
        for b, s in enumerate(SHARES):
            kw, passing = restriction(kind, b, s)
            truth = dev.knn_brute(qn, k, **kw)                      # (warm for the timed calls, too)
            took, took_none = [], []
            for _ in range(args.runs):                              # alternating
                took.append(timed(**kw))
                took_none.append(timed())
            got = {p: dev.query_batch(qn, qp, k, p, **kw) for p in (10, 50)}
            line = dict(bench="recall", restriction=kind, selectivity=s, nq=nq, k=k, rows=int(N), passing=passing,
                        truth_answered=float((truth >= 0).mean()),
                        **{f"recall_np{p}": recall(g, truth) for p, g in got.items()},
                        **{f"answered_np{p}": float((g >= 0).mean()) for p, g in got.items()},
                        brute_ms=float(np.median(took)), brute_ms_none=float(np.median(took_none)),
                        brute_ms_runs=took, brute_ms_none_runs=took_none, runs=args.runs)
            print(json.dumps(line), flush=True)
            if sink:
                sink.write(json.dumps(line) + "\n")
                sink.flush()
    # the unrestricted figure beside them, by the same arithmetic
    truth = dev.knn_brute(qn, k)
    line = dict(bench="recall", restriction="none", selectivity=1.0, nq=nq, k=k, rows=int(N), passing=float(N),
                **{f"recall_np{p}": recall(dev.query_batch(qn, qp, k, p), truth) for p in (10, 50)})
    print(json.dumps(line), flush=True)
    if sink:
        sink.write(json.dumps(line) + "\n")
        sink.close()
    ivf.set_values(None)
    ivf.set_tags(None)
    ivf.set_groups(None)


if __name__ == "__main__":
    main()
