#!/usr/bin/env python3
"""bench_groups.py — every query of a batch restricted to its own group of rows (IVF.set_groups, group_ptr=,
tk_index_query_batch_dev_ex3) on the GloVe-shaped index bench.py measures (bench.build_index): pipelined
query_batch_dev calls of --nq queries, n_probes 10, k 10, as bench_allow.py (pipeline 2, pairs of calls).
Per group count G (2, 10, 100, 1000 random groups, and 10 groups of whole lists) the queries are spread evenly over
the groups.  Prints one JSON line per point, every rate the median of --runs alternating runs:
  qps            one grouped call per step: queries/s, host clock around --steps calls ending in a device synchronise
  qps_plain      the same with tk_index_set_plain_scan(2) (grouped calls on the matrix-core scan + re-scans)
  flagged        queries the plain path flagged for the exact re-scan in one batch of that mode
  qps_split      (G = 10, 100) the same queries the way an index without groups serves them: one allowed= call per
                 group over that group's queries, the G sets made beforehand
  parity / parity_plain / parity_split   rows of that leg's output equal to the CPU reference
                 (tests/groups_reference.py) over a sample of --parity-sample queries
  table_bytes / row_bytes   the group table in list-position order / the groups by row id
The group pass's own kernel time comes from a profiler run of this script (group_pass_kernel in the kernel trace;
--only G restricts the run to one group count and adds four calls with one batch in flight, and four allowed= calls
over one group's rows beside them, so that the trace holds single launches of both passes).

    python bench_groups.py --steps 20 --out profiles/r09/bench_groups.jsonl
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--n-probes", type=int, default=10)
    ap.add_argument("--groups", type=int, nargs="+", default=[2, 10, 100, 1000])
    ap.add_argument("--split", type=int, nargs="*", default=[10, 100])
    ap.add_argument("--only", type=int, default=0, help="one group count, the grouped exact leg alone (profiler runs)")
    ap.add_argument("--parity-sample", type=int, default=50)
    ap.add_argument("--cache-dir", default=os.environ.get("TMPDIR", "/tmp"))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import bench
    from allowed_reference import reference_index
    from groups_reference import grouped_batch
    from tinyknn_amd import _lib
    assert _lib.device_count() >= 1, "bench_groups.py needs a GPU"
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
    esz = qp.dtype.itemsize
    outs = [torch.full((args.nq, args.k), -1, dtype=torch.int64, device=device) for _ in range(args.steps)]
    sink = open(args.out, "a") if args.out else None

    def settings(plain):
        dev.set_pipeline(2)
        dev.set_coalesce(2)
        dev.set_plain_scan(plain)

    def grouped(group_t, plain):
        """--steps grouped calls of --nq queries between two drains"""
        settings(plain)
        gp = None if group_t is None else group_t.data_ptr()
        for i in range(args.warmup):
            dev.query_batch_dev(qn_t.data_ptr(), qp_t.data_ptr(), is64, args.nq, args.k, args.n_probes,
                                outs[i % len(outs)].data_ptr(), group_ptr=gp)
        dev.join()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for out in outs:
            dev.query_batch_dev(qn_t.data_ptr(), qp_t.data_ptr(), is64, args.nq, args.k, args.n_probes,
                                out.data_ptr(), group_ptr=gp)
        dev.join()
        torch.cuda.synchronize()
        return args.steps * args.nq / (time.perf_counter() - t0)

    def split(spans, asets):
        """the same queries, sorted by group: per step one allowed= call per group over that group's rows"""
        settings(True)

        def step(out):
            for (o, n), aset in zip(spans, asets):
                if n:
                    dev.query_batch_dev(qn_t.data_ptr() + o * qn.shape[1] * 4, qp_t.data_ptr() + o * qp.shape[1] * esz,
                                        is64, n, args.k, args.n_probes, out.data_ptr() + o * args.k * 8, allowed=aset)
        step(outs[0])
        dev.join()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for out in outs:
            step(out)
        dev.join()
        torch.cuda.synchronize()
        return args.steps * args.nq / (time.perf_counter() - t0)

    def single(plain, n=1, **restriction):
        """n calls with one batch in flight, each drained: one pass launch per call of --nq queries"""
        dev.set_pipeline(1)
        dev.set_coalesce(1)
        dev.set_plain_scan(plain)
        for _ in range(n):
            dev.query_batch_dev(qn_t.data_ptr(), qp_t.data_ptr(), is64, args.nq, args.k, args.n_probes,
                                outs[0].data_ptr(), **restriction)
            dev.join()
            torch.cuda.synchronize()
        stats = dev.plain_stats()
        dev.set_plain_scan(True)
        return stats

    def flagged(group_t):
        return single("always", group_ptr=group_t.data_ptr())["flagged_queries"]

    rng = np.random.default_rng(0)
    points = [("random", G, rng.integers(0, G, N).astype(np.int32)) for G in args.groups]
    by_list = np.zeros(N, dtype=np.int32)
    for li, l in enumerate(rng.permutation(len(ivf.ids))):          # whole lists per group
        by_list[np.asarray(ivf.ids[l], dtype=np.int64)] = li % 10
    points.append(("lists", 10, by_list))
    if args.only:
        points = [p for p in points if p[0] == "random" and p[1] == args.only]
    sample = rng.permutation(args.nq)[:args.parity_sample]
    # the queries sorted by group (query i has group i * G // nq), so that the split leg's calls take contiguous rows
    for kind, G, groups in points:
        group = (np.arange(args.nq, dtype=np.int64) * G // args.nq).astype(np.int32)
        group_t = torch.from_numpy(group).to(device)
        ivf.set_groups(groups)
        if args.only:
            # for a kernel trace: pair launches inside the pipelined run, then four single launches of the group pass
            # (exact scan) and, beside them, of the allow pass over the set groups == 0
            qps = grouped(group_t, True)
            single(True, 4, group_ptr=group_t.data_ptr())
            aset = dev.allow(groups == 0)
            single(True, 4, allowed=aset)
            aset.close()
            print(json.dumps(dict(bench="groups", groups=G, qps=qps)), flush=True)
            continue
        do_split = kind == "random" and G in args.split
        asets, spans = [], []
        if do_split:
            asets = [dev.allow(groups == g) for g in range(G)]
            bounds = np.searchsorted(group, np.arange(G + 1))
            spans = [(int(bounds[g]), int(bounds[g + 1] - bounds[g])) for g in range(G)]
        legs = dict(qps=[], qps_plain=[], qps_none=[], qps_split=[])
        for _ in range(args.runs):                                 # alternating
            legs["qps"].append(grouped(group_t, True))
            legs["qps_plain"].append(grouped(group_t, "always"))
            legs["qps_none"].append(grouped(None, True))
            if do_split:
                legs["qps_split"].append(split(spans, asets))
        # every leg's last output against the reference over the sample (the split leg over all rows against the
        # grouped call as well)
        want = grouped_batch(None, ref, qn[sample], group[sample], groups, args.k, args.n_probes)

        def same(rows):
            return int((want == rows[sample]).all(axis=1).sum())
        if do_split:
            split(spans, asets)
            by_sets = outs[-1].cpu().numpy()
        grouped(group_t, "always")
        by_plain = outs[-1].cpu().numpy()
        grouped(group_t, True)
        got = outs[-1].cpu().numpy()
        nflag = flagged(group_t)
        t = dev.group_table()
        for a in asets:
            a.close()
        line = dict(bench="groups", assignment=kind, groups=G, nq=args.nq, n_probes=args.n_probes, k=args.k,
                    steps=args.steps, runs=args.runs,
                    **{name: float(np.median(v)) if v else None for name, v in legs.items()},
                    **{name + "_runs": v for name, v in legs.items() if v},
                    flagged=int(nflag), parity=same(got), parity_plain=same(by_plain),
                    parity_split=same(by_sets) if do_split else None, parity_sample=len(sample),
                    split_equal=bool((by_sets == got).all()) if do_split else None,
                    table_bytes=t["bytes"], row_bytes=t["row_bytes"], rows=int(N))
        print(json.dumps(line), flush=True)
        if sink:
            sink.write(json.dumps(line) + "\n")
            sink.flush()
    ivf.set_groups(None)


if __name__ == "__main__":
    main()
