#!/usr/bin/env python3
"""bench_group_exact.py — the exact search inside a query's own group (DeviceIndex.knn_group, tk_index_knn_group)
against the restricted exact search over all rows (knn_brute(group=)) and the grouped index query, on the GloVe-shaped
index bench.py measures (bench.build_index): --nq queries (10 000) spread over 100 / 1 000 / 10 000 random groups, k 10.
One JSON line per number of groups; every time is the host clock around the call (each ends with its ids on the host),
the median of --runs runs, the calls alternating within a run:
  group_ms       knn_group
  brute_ms       knn_brute(group=) on the same queries — the call the parent commit has for an exact answer
  np10_ms / np50_ms   query_batch(group=, n_probes=10 / 50) on the prepared queries
  recall_*       Recall10@10 of each against knn_brute(group=): mean of |ids ∩ truth| / (truth ids that are not -1);
                 for knn_group the ids a different distance formula ranks differently at a tie of the tenth place
  answered_*     the share of the k slots that hold an id
  table_ms / table_bytes / stored_bytes   making the rows by group (first knn_group call after set_groups, minus a
                 later call) and what stays of it; the stored-row map's bytes
  sample_*       50 sampled queries of knn_group against numpy: the ids of lexsort((row, einsum distance)) over the
                 group's rows, the largest distance error in ulp
and one line for a batch that mixes small and large groups (half the rows in --small-groups groups, half in 5):
  plain_ms / routed_ms   IVF.query_batch(group=, n_probes=10) without and with exact_below=T on RAW queries (both
                 include the host's preparation of the queries), recall and answered of each against knn_brute(group=)

    python bench_group_exact.py --out profiles/r21/bench_group_exact.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def recall(got, truth):
    """mean over the queries of |got ∩ truth| / (ids of truth that are not -1); queries without a true id left out"""
    per = [len(set(g[g >= 0]) & set(t[t >= 0])) / (t >= 0).sum() for g, t in zip(got, truth) if (t >= 0).any()]
    return float(np.mean(per))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--groups", type=int, nargs="+", default=[100, 1000, 10000])
    ap.add_argument("--small-groups", type=int, default=1000)
    ap.add_argument("--exact-below", type=int, default=5000)
    ap.add_argument("--n", type=int, default=1183514)
    ap.add_argument("--n-clusters", type=int, default=1087)
    ap.add_argument("--cache-dir", default=os.environ.get("TMPDIR", "/tmp"))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import bench
    from tinyknn_amd import _lib
    assert _lib.device_count() >= 1, "bench_group_exact.py needs a GPU"
    device = torch.device("cuda", 0)
    bargs = argparse.Namespace(n=args.n, d=100, n_clusters=args.n_clusters, seed=10, build_probes=1, metric="angular",
                               data="glove-like", fit_sample=min(100000, args.n), cache_dir=args.cache_dir)
    ivf, cent = bench.build_index(bargs, device)
    qs = bench.synth_queries(cent, args.nq, bargs.seed + 1, kind="glove-like")
    qn, qp = ivf._prepare(qs.copy())
    dev = ivf.device_index()
    data = np.asarray(ivf.data)
    N, nq, k = data.shape[0], args.nq, args.k
    rng = np.random.default_rng(0)
    sink = None
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        sink = open(args.out, "a")

    def emit(line):
        print(json.dumps(line), flush=True)
        if sink:
            sink.write(json.dumps(line) + "\n")
            sink.flush()

    def clock(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        return 1e3 * (time.perf_counter() - t0), out

    def sample_check(ids, dist, group, groups):
        """50 queries against numpy's einsum over their group's rows"""
        equal, ulp = 0, 0.0
        pick = rng.choice(nq, size=min(50, nq), replace=False)
        for i in pick:
            rows = np.flatnonzero(groups == group[i])
            diff = data[rows] - qn[i]
            dv = np.einsum("ij,ij->i", diff, diff)
            order = np.lexsort((rows, dv))[:k]
            want = np.full(k, -1, dtype=np.int64)
            want[:len(order)] = rows[order]
            equal += int(np.array_equal(want, ids[i]))
            live = ids[i] >= 0
            if live.any():
                d2 = data[ids[i][live]] - qn[i]
                e = np.einsum("ij,ij->i", d2, d2)
                ulp = max(ulp, float(np.max(np.abs(dist[i][live] - e) / np.spacing(np.maximum(e, dist[i][live])))))
        return equal, len(pick), ulp

    dev.knn_brute(qn[:64], k)                                           # (warm: code objects)
    for n_groups in args.groups:
        groups = rng.integers(0, n_groups, N).astype(np.int32)
        ivf.set_groups(groups)
        group = rng.integers(0, n_groups, nq).astype(np.int32)
        first_ms, _ = clock(lambda: dev.knn_group(qn, k, group))        # makes both tables
        info = dev.group_rows()
        truth = dev.knn_brute(qn, k, group=group)
        for p in (10, 50):
            dev.query_batch(qn, qp, k, p, group=group)                  # (warm: the group table, workspaces)
        took = dict(group=[], brute=[], np10=[], np50=[])
        for _ in range(args.runs):                                      # alternating
            took["group"].append(clock(lambda: dev.knn_group(qn, k, group))[0])
            took["brute"].append(clock(lambda: dev.knn_brute(qn, k, group=group))[0])
            took["np10"].append(clock(lambda: dev.query_batch(qn, qp, k, 10, group=group))[0])
            took["np50"].append(clock(lambda: dev.query_batch(qn, qp, k, 50, group=group))[0])
        ids, dist = dev.knn_group(qn, k, group, return_distances=True)
        got = dict(group=ids, np10=dev.query_batch(qn, qp, k, 10, group=group),
                   np50=dev.query_batch(qn, qp, k, 50, group=group))
        equal, checked, ulp = sample_check(ids, dist, group, groups)
        med = {w: float(np.median(t)) for w, t in took.items()}
        emit(dict(bench="group_exact", groups=n_groups, nq=nq, k=k, rows=int(N),
                  rows_per_group=float(np.bincount(groups, minlength=n_groups)[group].mean()),
                  **{f"{w}_ms": m for w, m in med.items()}, speedup_vs_brute=med["brute"] / med["group"],
                  **{f"recall_{w}": recall(g, truth) for w, g in got.items()},
                  **{f"answered_{w}": float((g >= 0).mean()) for w, g in got.items()},
                  truth_answered=float((truth >= 0).mean()),
                  table_ms=first_ms - med["group"], table_bytes=info["bytes"], table_groups=info["groups"],
                  stored_bytes=(N + 31) // 32 * 4, sample_ids_equal=equal, sample_checked=checked, sample_max_ulp=ulp,
                  runs=args.runs, **{f"{w}_ms_runs": t for w, t in took.items()}))

    # a batch that mixes small and large groups
    small = args.small_groups
    groups = np.where(rng.random(N) < 0.5, rng.integers(0, small, N), small + rng.integers(0, 5, N)).astype(np.int32)
    ivf.set_groups(groups)
    group = np.where(rng.random(nq) < 0.5, rng.integers(0, small, nq), small + rng.integers(0, 5, nq)).astype(np.int32)
    T = args.exact_below
    sizes = dev.group_sizes(group)
    truth = dev.knn_brute(qn, k, group=group)
    call = dict(plain=lambda: ivf.query_batch(qs, k, 10, group=group),
                routed=lambda: ivf.query_batch(qs, k, 10, group=group, exact_below=T))
    got = {w: f() for w, f in call.items()}                             # (warm)
    took = dict(plain=[], routed=[])
    for _ in range(args.runs):
        for w, f in call.items():
            took[w].append(clock(f)[0])
    emit(dict(bench="group_exact_mixed", nq=nq, k=k, rows=int(N), small_groups=small, large_groups=5, exact_below=T,
              routed_queries=int((sizes < T).sum()), rows_per_small_group=float(sizes[sizes < T].mean()),
              rows_per_large_group=float(sizes[sizes >= T].mean()),
              **{f"{w}_ms": float(np.median(t)) for w, t in took.items()},
              **{f"recall_{w}": recall(g, truth) for w, g in got.items()},
              **{f"recall_{w}_small": recall(g[sizes < T], truth[sizes < T]) for w, g in got.items()},
              **{f"answered_{w}": float((g >= 0).mean()) for w, g in got.items()},
              runs=args.runs, **{f"{w}_ms_runs": t for w, t in took.items()}))
    if sink:
        sink.close()
    ivf.set_groups(None)


if __name__ == "__main__":
    main()
