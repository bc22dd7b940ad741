#!/usr/bin/env python3
"""bench_between_exact.py — the exact search inside a query's value range (DeviceIndex.knn_between,
tk_index_knn_between) against the restricted exact search over all rows (knn_brute(between=)), the ranged index query
and the exact search inside a group of the same size, on the GloVe-shaped index bench.py measures (bench.build_index):
--nq queries (10 000), k 10, one int64 "timestamp" column drawn uniformly, every query with its own window of
selectivity 0.1 / 0.01 / 0.001 / 0.0001.  One JSON line per selectivity; every time is the host clock around the call
(each ends with its ids on the host), the median of --runs runs, the calls alternating within a run:
  between_ms     knn_between
  brute_ms       knn_brute(between=) on the same queries — the call the parent commit has for an exact answer
  np10_ms / np50_ms   query_batch(between=, n_probes=10 / 50) on the prepared queries
  group_ms       knn_group with round(1 / selectivity) random groups: spans of the same mean length walked by the same
                 kernel body, ascending by row id instead of in value order — the gap to between_ms is what the value
                 order costs (scattered row reads, the span lookup)
  recall_*       Recall10@10 of each against knn_brute(between=): mean of |ids ∩ truth| / (truth ids that are not -1)
  answered_*     the share of the k slots that hold an id
  table_ms / table_bytes   making the rows by value (first knn_between call after set_values, minus a later call) and
                 what stays of it
  sample_*       50 sampled queries of knn_between against numpy: the ids of lexsort((row, einsum distance)) over the
                 window's rows, the largest distance error in ulp
then one line for two columns, the first wide (selectivity 0.1) and the second narrow (0.001), every query bounding
both — col1_share is the share of queries that walk the narrow column — beside the narrow column alone; and one line
for a batch that mixes windows of selectivity ~0.0005 and ~0.1:
  plain_ms / routed_ms   IVF.query_batch(between=, n_probes=10) without and with exact_below=T on RAW queries (both
                 include the host's preparation of the queries), recall and answered of each against knn_brute(between=)

    python bench_between_exact.py --out profiles/r22/bench_between_exact.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
SPAN = 2**40            # the timestamps lie in [0, SPAN)


def recall(got, truth):
    """mean over the queries of |got ∩ truth| / (ids of truth that are not -1); queries without a true id left out"""
    per = [len(set(g[g >= 0]) & set(t[t >= 0])) / (t >= 0).sum() for g, t in zip(got, truth) if (t >= 0).any()]
    return float(np.mean(per)) if per else float("nan")


def windows(rng, nq, selectivity):
    """(lo, hi) int64: per query a window holding `selectivity` of a uniform column (an array: one per query)"""
    width = (SPAN * np.broadcast_to(selectivity, (nq,))).astype(np.int64)
    lo = (rng.random(nq) * (SPAN - width)).astype(np.int64)
    return lo, lo + width


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--selectivity", type=float, nargs="+", default=[0.1, 0.01, 0.001, 0.0001])
    ap.add_argument("--exact-below", type=int, default=5000)
    ap.add_argument("--n", type=int, default=1183514)
    ap.add_argument("--n-clusters", type=int, default=1087)
    ap.add_argument("--cache-dir", default=os.environ.get("TMPDIR", "/tmp"))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import bench
    from tinyknn_amd import _lib
    assert _lib.device_count() >= 1, "bench_between_exact.py needs a GPU"
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

    def sample_check(ids, dist, stamps, lo, hi):
        """50 queries against numpy's einsum over their window's rows"""
        equal, ulp = 0, 0.0
        pick = rng.choice(nq, size=min(50, nq), replace=False)
        for i in pick:
            rows = np.flatnonzero((stamps >= lo[i]) & (stamps <= hi[i]))
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
    stamps = rng.integers(0, SPAN, N).astype(np.int64)
    for s in args.selectivity:
        ivf.set_values(stamps)                                          # (again: the table's build is timed per line)
        between = windows(rng, nq, s)
        first_ms, _ = clock(lambda: dev.knn_between(qn, k, between))    # makes the rows by value (and the stored map)
        info = dev.value_rows()
        length, _ = dev.range_sizes(between)
        n_groups = max(1, int(round(1 / s)))
        groups = rng.integers(0, n_groups, N).astype(np.int32)
        ivf.set_groups(groups)
        group = rng.integers(0, n_groups, nq).astype(np.int32)
        dev.knn_group(qn, k, group)                                     # (warm: the rows by group)
        truth = dev.knn_brute(qn, k, between=between)
        for p in (10, 50):
            dev.query_batch(qn, qp, k, p, between=between)              # (warm: the value table, workspaces)
        took = dict(between=[], group=[], brute=[], np10=[], np50=[])
        for _ in range(args.runs):                                      # alternating
            took["between"].append(clock(lambda: dev.knn_between(qn, k, between))[0])
            took["group"].append(clock(lambda: dev.knn_group(qn, k, group))[0])
            took["brute"].append(clock(lambda: dev.knn_brute(qn, k, between=between))[0])
            took["np10"].append(clock(lambda: dev.query_batch(qn, qp, k, 10, between=between))[0])
            took["np50"].append(clock(lambda: dev.query_batch(qn, qp, k, 50, between=between))[0])
        ids, dist = dev.knn_between(qn, k, between, return_distances=True)
        got = dict(between=ids, np10=dev.query_batch(qn, qp, k, 10, between=between),
                   np50=dev.query_batch(qn, qp, k, 50, between=between))
        equal, checked, ulp = sample_check(ids, dist, stamps, *between)
        med = {w: float(np.median(t)) for w, t in took.items()}
        emit(dict(bench="between_exact", selectivity=s, nq=nq, k=k, rows=int(N), rows_per_window=float(length.mean()),
                  groups=n_groups, rows_per_group=float(np.bincount(groups, minlength=n_groups)[group].mean()),
                  **{f"{w}_ms": m for w, m in med.items()}, speedup_vs_brute=med["brute"] / med["between"],
                  between_over_group=med["between"] / med["group"],
                  **{f"recall_{w}": recall(g, truth) for w, g in got.items()},
                  **{f"answered_{w}": float((g >= 0).mean()) for w, g in got.items()},
                  truth_answered=float((truth >= 0).mean()),
                  table_ms=first_ms - med["between"], table_bytes=info["bytes"], table_columns=info["columns"],
                  sample_ids_equal=equal, sample_checked=checked, sample_max_ulp=ulp,
                  runs=args.runs, **{f"{w}_ms_runs": t for w, t in took.items()}))
    ivf.set_groups(None)

    # two columns: the first wide, the second narrow; every query bounds both
    second = rng.integers(0, SPAN, N).astype(np.int64)
    wide, narrow = windows(rng, nq, 0.1), windows(rng, nq, 0.001)
    both = (np.stack([wide[0], narrow[0]], axis=1), np.stack([wide[1], narrow[1]], axis=1))
    ivf.set_values(np.stack([stamps, second], axis=1))
    first_ms, _ = clock(lambda: dev.knn_between(qn, k, both))
    info = dev.value_rows()
    length, col = dev.range_sizes(both)
    two = [clock(lambda: dev.knn_between(qn, k, both))[0] for _ in range(args.runs)]
    truth = dev.knn_brute(qn, k, between=both)
    ids = dev.knn_between(qn, k, both)
    ivf.set_values(second)
    dev.knn_between(qn, k, narrow)
    one = [clock(lambda: dev.knn_between(qn, k, narrow))[0] for _ in range(args.runs)]
    emit(dict(bench="between_exact_two_columns", nq=nq, k=k, rows=int(N), selectivity=[0.1, 0.001],
              col1_share=float((col == 1).mean()), rows_per_window=float(length.mean()),
              two_columns_ms=float(np.median(two)), narrow_alone_ms=float(np.median(one)),
              recall_between=recall(ids, truth), answered_between=float((ids >= 0).mean()),
              table_ms=first_ms - float(np.median(two)), table_bytes=info["bytes"], table_columns=info["columns"],
              runs=args.runs, two_columns_ms_runs=two, narrow_alone_ms_runs=one))

    # a batch that mixes narrow and wide windows
    ivf.set_values(stamps)
    between = windows(rng, nq, np.where(rng.random(nq) < 0.5, 0.0005, 0.1))
    T = args.exact_below
    length, _ = dev.range_sizes(between)
    truth = dev.knn_brute(qn, k, between=between)
    call = dict(plain=lambda: ivf.query_batch(qs, k, 10, between=between),
                routed=lambda: ivf.query_batch(qs, k, 10, between=between, exact_below=T))
    got = {w: f() for w, f in call.items()}                             # (warm)
    took = dict(plain=[], routed=[])
    for _ in range(args.runs):
        for w, f in call.items():
            took[w].append(clock(f)[0])
    emit(dict(bench="between_exact_mixed", nq=nq, k=k, rows=int(N), selectivity=[0.0005, 0.1], exact_below=T,
              routed_queries=int((length < T).sum()), rows_per_narrow_window=float(length[length < T].mean()),
              rows_per_wide_window=float(length[length >= T].mean()),
              **{f"{w}_ms": float(np.median(t)) for w, t in took.items()},
              **{f"recall_{w}": recall(g, truth) for w, g in got.items()},
              **{f"recall_{w}_narrow": recall(g[length < T], truth[length < T]) for w, g in got.items()},
              **{f"answered_{w}": float((g >= 0).mean()) for w, g in got.items()},
              runs=args.runs, **{f"{w}_ms_runs": t for w, t in took.items()}))
    if sink:
        sink.close()
    ivf.set_values(None)


if __name__ == "__main__":
    main()
