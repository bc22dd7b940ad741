#!/usr/bin/env python3
"""bench_allow.py — queries restricted to an allowed set of rows (DeviceIndex.allow, tk_index_query_batch_dev_allow)
on the GloVe-shaped index bench.py measures (bench.build_index): pipelined query_batch_dev calls of --nq queries,
n_probes 10, k 10, as bench.py's headline (pipeline 2, pairs of calls).  Per selectivity (1.0, 0.5, 0.1, 0.01) one
random-id set and one cluster-correlated set (whole lists allowed), and the unrestricted calls for reference.
Prints one JSON line per point:
  qps            queries/s, host clock around --steps calls ending in a device synchronise
  qps_plain      the same with tk_index_set_plain_scan(2) (restricted calls on the matrix-core scan + re-scans)
  flagged        queries the plain path flagged for the exact re-scan in one batch of that mode
  recall10       Recall10@10 against the exact neighbours WITHIN the set (numpy over the allowed rows, a sample)
  parity         rows equal to the guarded CPU reference (tests/allowed_reference.py) over a sample
The allow pass's own kernel time comes from a profiler run of this script (allow_pass_kernel in the kernel trace).

    python bench_allow.py --steps 20 --out profiles/r07/bench_allow.jsonl
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
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--n-probes", type=int, default=10)
    ap.add_argument("--sel", type=float, nargs="+", default=[1.0, 0.5, 0.1, 0.01])
    ap.add_argument("--recall-sample", type=int, default=100)
    ap.add_argument("--parity-sample", type=int, default=50)
    ap.add_argument("--cache-dir", default=os.environ.get("TMPDIR", "/tmp"))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import bench
    from allowed_reference import guarded_batch, reference_index
    from tinyknn_amd import _lib
    assert _lib.device_count() >= 1, "bench_allow.py needs a GPU"
    device = torch.device("cuda", 0)
    bargs = argparse.Namespace(n=1183514, d=100, n_clusters=1087, seed=10, build_probes=1, metric="angular",
                               data="glove-like", fit_sample=100000, cache_dir=args.cache_dir)
    ivf, cent = bench.build_index(bargs, device)
    qs = bench.synth_queries(cent, args.nq, bargs.seed + 1, kind="glove-like")
    qn, qp = ivf._prepare(qs.copy())
    dev = ivf.device_index()
    ref = reference_index(ivf)
    N = ivf.data.shape[0]
    data = np.asarray(ivf.data, dtype=np.float32)
    qn_t = torch.from_numpy(np.ascontiguousarray(qn)).to(device)
    qp_t = torch.from_numpy(np.ascontiguousarray(qp)).to(device)
    is64 = int(qp.dtype != np.float32)
    outs = [torch.full((args.nq, args.k), -1, dtype=torch.int64, device=device) for _ in range(args.steps)]
    sink = open(args.out, "a") if args.out else None

    def timed(aset, plain):
        dev.set_pipeline(2)
        dev.set_coalesce(2)
        dev.set_plain_scan(plain)
        for i in range(args.warmup):
            dev.query_batch_dev(qn_t.data_ptr(), qp_t.data_ptr(), is64, args.nq, args.k, args.n_probes,
                                outs[i % len(outs)].data_ptr(), allowed=aset)
        dev.join()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for out in outs:
            dev.query_batch_dev(qn_t.data_ptr(), qp_t.data_ptr(), is64, args.nq, args.k, args.n_probes,
                                out.data_ptr(), allowed=aset)
        dev.join()
        torch.cuda.synchronize()
        return args.steps * args.nq / (time.perf_counter() - t0)

    def flagged(aset):
        dev.set_pipeline(1)
        dev.set_coalesce(1)
        dev.set_plain_scan("always")
        dev.query_batch_dev(qn_t.data_ptr(), qp_t.data_ptr(), is64, args.nq, args.k, args.n_probes,
                            outs[0].data_ptr(), allowed=aset)
        n = dev.plain_stats()["flagged_queries"]
        dev.set_plain_scan(True)
        return n

    rng = np.random.default_rng(0)
    lists_by_size = rng.permutation(len(ivf.ids))
    points = [("none", 1.0, None)]
    for sel in args.sel:
        points.append(("random", sel, rng.random(N) < sel))
        # whole lists until the share is reached
        m = np.zeros(N, dtype=bool)
        for li in lists_by_size:
            if m.sum() >= sel * N:
                break
            m[ivf.ids[li]] = True
        points.append(("lists", sel, m))
    sample = rng.permutation(args.nq)
    for kind, sel, mask in points:
        aset = None if mask is None else dev.allow(mask)
        qps = timed(aset, True)
        qps_plain = timed(aset, "always")
        nflag = flagged(aset)
        got = outs[-1].cpu().numpy()
        rec = par = None
        if mask is not None:
            rows = np.flatnonzero(mask)
            hits = 0
            rs = sample[:args.recall_sample]
            for i in rs:
                if len(rows) == 0:
                    continue
                d = ((data[rows] - qn[i]) ** 2).sum(axis=1)
                true = rows[np.argsort(d, kind="stable")[:args.k]]
                hits += len(np.intersect1d(true, got[i][got[i] != -1]))
            rec = hits / float(len(rs) * min(args.k, max(len(rows), 1)))
            ps = sample[:args.parity_sample]
            want = guarded_batch(None, ref, qn[ps], args.k, args.n_probes, allowed=mask)
            par = int((want == got[ps]).all(axis=1).sum())
            aset.close()
        line = dict(bench="allow", set=kind, selectivity=sel, allowed_rows=None if mask is None else int(mask.sum()),
                    nq=args.nq, n_probes=args.n_probes, k=args.k, steps=args.steps, qps=qps, qps_plain=qps_plain,
                    flagged=int(nflag), recall10=rec, parity=par,
                    parity_sample=None if mask is None else len(sample[:args.parity_sample]))
        print(json.dumps(line), flush=True)
        if sink:
            sink.write(json.dumps(line) + "\n")
            sink.flush()


if __name__ == "__main__":
    main()
