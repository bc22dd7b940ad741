#!/usr/bin/env python3
"""bench_per_group.py — at most m rows of any group per query (per_group_ptr=, tk_index_query_batch_dev_ex6, the capped
rescoring kernels of rescore.hip) on the GloVe-shaped index bench.py measures (bench.build_index): pipelined
query_batch_dev calls of --nq queries, n_probes 10, k 10, as bench_groups.py (pipeline 2, pairs of calls).
Two group assignments — "oct": groups of 8 consecutive rows (chunks of one document), "random": 1000 random groups —
and m = 1 and 3.  Prints one JSON line per point, every rate the median of --runs alternating runs:
  qps_uncapped   the call without a cap: queries/s, host clock around --steps calls ending in a device synchronise
  qps_capped     the call with per_group_ptr= (every query capped at m)
  qps_overfetch  what a caller does without the feature: the uncapped call with k = --overfetch (40), the ids copied to
                 the host and collapsed there in numpy (the first m of a group, the first k of those); the host part
                 alone is collapse_ms per batch.  Not the same query: k sets the heap length, so the candidates differ.
  parity_*       rows of that leg's output equal to the CPU reference over a sample of --parity-sample queries:
                 the capped leg and the over-fetch leg against tests/per_group_reference.py::capped_batch, the uncapped
                 leg against tests/allowed_reference.py::guarded_batch
  short_rows     rows of the capped answer with fewer than k ids
--legs uncapped runs the first leg alone; it needs nothing this feature added, so the same file times the parent commit.

    python bench_per_group.py --steps 20 --out profiles/r19/bench_per_group.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def collapse(ids, groups, m, k):
    """The host collapse of over-fetched rows: per row the first m ids of every group, the first k of those, -1 padded"""
    live = ids != -1
    g = np.where(live, groups[np.where(live, ids, 0)], -1 - np.arange(ids.shape[1])[None, :])   # (a -1 is nobody's group)
    same = g[:, :, None] == g[:, None, :]
    earlier = np.tril(np.ones((ids.shape[1],) * 2, dtype=bool), -1)
    keep = live & ((same & earlier[None]).sum(axis=2) < m)
    pos = np.cumsum(keep, axis=1) - 1
    keep &= pos < k
    out = np.full((len(ids), k), -1, dtype=np.int64)
    r, c = np.nonzero(keep)
    out[r, pos[r, c]] = ids[r, c]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--n-probes", type=int, default=10)
    ap.add_argument("--caps", type=int, nargs="+", default=[1, 3])
    ap.add_argument("--overfetch", type=int, default=40)
    ap.add_argument("--legs", choices=["all", "uncapped"], default="all")
    ap.add_argument("--parity-sample", type=int, default=50)
    ap.add_argument("--cache-dir", default=os.environ.get("TMPDIR", "/tmp"))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import bench
    from allowed_reference import guarded_batch, reference_index
    from tinyknn_amd import _lib
    assert _lib.device_count() >= 1, "bench_per_group.py needs a GPU"
    device = torch.device("cuda", 0)
    bargs = argparse.Namespace(n=1183514, d=100, n_clusters=1087, seed=10, build_probes=1, metric="angular",
                               data="glove-like", fit_sample=100000, cache_dir=args.cache_dir)
    ivf, cent = bench.build_index(bargs, device)
    qs = bench.synth_queries(cent, args.nq, bargs.seed + 1, kind="glove-like")
    qn, qp = ivf._prepare(qs.copy())
    dev = ivf.device_index()
    ref = reference_index(ivf)
    N = ivf.data.shape[0]
    qn_t = torch.from_numpy(np.ascontiguousarray(qn)).to(device)
    qp_t = torch.from_numpy(np.ascontiguousarray(qp)).to(device)
    is64 = int(qp.dtype != np.float32)
    kmax = max(args.k, args.overfetch)
    outs = [torch.full((args.nq, kmax), -1, dtype=torch.int64, device=device) for _ in range(args.steps)]
    sink = open(args.out, "a") if args.out else None
    dev.set_pipeline(2)
    dev.set_coalesce(2)

    def calls(k, cap_t):
        """--steps calls of --nq queries between two drains -> seconds"""
        kw = {} if cap_t is None else dict(per_group_ptr=cap_t.data_ptr())
        for i in range(args.warmup):
            dev.query_batch_dev(qn_t.data_ptr(), qp_t.data_ptr(), is64, args.nq, k, args.n_probes,
                                outs[i % len(outs)].data_ptr(), **kw)
        dev.join()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for out in outs:
            dev.query_batch_dev(qn_t.data_ptr(), qp_t.data_ptr(), is64, args.nq, k, args.n_probes, out.data_ptr(), **kw)
        dev.join()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def rows_of(out, k):
        return out.cpu().numpy().reshape(-1)[:args.nq * k].reshape(args.nq, k)

    def overfetch(groups, m):
        """the device calls with k = --overfetch, then every batch copied back and collapsed -> (seconds, host seconds)"""
        t = calls(args.overfetch, None)
        t0 = time.perf_counter()
        for out in outs:
            got = collapse(rows_of(out, args.overfetch), groups, m, args.k)
        return t + (time.perf_counter() - t0), time.perf_counter() - t0, got

    rng = np.random.default_rng(0)
    sample = rng.permutation(args.nq)[:args.parity_sample]
    want_plain = guarded_batch(None, ref, qn[sample], args.k, args.n_probes)
    if args.legs == "uncapped":
        rates = [args.steps * args.nq / calls(args.k, None) for _ in range(args.runs)]
        got = rows_of(outs[-1], args.k)
        line = dict(bench="per_group", legs="uncapped", nq=args.nq, n_probes=args.n_probes, k=args.k, steps=args.steps,
                    runs=args.runs, qps_uncapped=float(np.median(rates)), qps_uncapped_runs=rates,
                    parity_uncapped=int((want_plain == got[sample]).all(axis=1).sum()), parity_sample=len(sample))
        print(json.dumps(line), flush=True)
        if sink:
            sink.write(json.dumps(line) + "\n")
        return
    from per_group_reference import capped_batch
    points = [("oct", (np.arange(N) // 8).astype(np.int32)), ("random", rng.integers(0, 1000, N).astype(np.int32))]
    for kind, groups in points:
        ivf.set_groups(groups)
        for m in args.caps:
            cap_t = torch.full((args.nq,), m, dtype=torch.int32, device=device)
            legs = dict(qps_uncapped=[], qps_capped=[], qps_overfetch=[])
            host = []
            for _ in range(args.runs):                                  # alternating
                legs["qps_uncapped"].append(args.steps * args.nq / calls(args.k, None))
                legs["qps_capped"].append(args.steps * args.nq / calls(args.k, cap_t))
                t, th, by_host = overfetch(groups, m)
                legs["qps_overfetch"].append(args.steps * args.nq / t)
                host.append(1e3 * th / args.steps)
            want = capped_batch(None, ref, qn[sample], m, groups, args.k, args.n_probes)[0]
            calls(args.k, None)
            plain = rows_of(outs[-1], args.k)
            calls(args.k, cap_t)
            got = rows_of(outs[-1], args.k)
            line = dict(bench="per_group", assignment=kind, m=m, nq=args.nq, n_probes=args.n_probes, k=args.k,
                        overfetch=args.overfetch, steps=args.steps, runs=args.runs,
                        **{name: float(np.median(v)) for name, v in legs.items()},
                        **{name + "_runs": v for name, v in legs.items()},
                        collapse_ms=float(np.median(host)),
                        parity_uncapped=int((want_plain == plain[sample]).all(axis=1).sum()),
                        parity_capped=int((want == got[sample]).all(axis=1).sum()),
                        parity_overfetch=int((want == by_host[sample]).all(axis=1).sum()), parity_sample=len(sample),
                        changed_rows=int((got != plain).any(axis=1).sum()),
                        short_rows=int((got == -1).any(axis=1).sum()), rows=int(N))
            print(json.dumps(line), flush=True)
            if sink:
                sink.write(json.dumps(line) + "\n")
                sink.flush()
    ivf.set_groups(None)


if __name__ == "__main__":
    main()
