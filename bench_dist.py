#!/usr/bin/env python3
"""bench_dist.py — the cost of returning the rescoring's exact distances beside the ids on the
GloVe-shaped index bench.py measures (bench.build_index).  Prints one JSON line per point:
  pipelined   query_batch_dev calls of --nq queries, n_probes 10, k 10, pipeline 2 and pairs of calls as bench.py's
              headline runs them: ids only against dist_ptr=, in alternating runs (queries/s of the median window of
              each run, as bench.timed_rate); `same` = the last calls' ids were identical in both modes
  per_call    IVF.query_batch(..., return_distances=True) against the ids-only call at --per-call sizes: host clock
              per call (median of --reps), preparation and copies included; `same` = identical ids

    python bench_dist.py --runs 3 --out profiles/r07/bench_dist.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3, help="alternating (ids only, distances) runs of the pipelined leg")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--n-probes", type=int, default=10)
    ap.add_argument("--per-call", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--cache-dir", default=os.environ.get("TMPDIR", "/tmp"))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import bench
    from tinyknn_amd import _lib
    assert _lib.device_count() >= 1, "bench_dist.py needs a GPU"
    device = torch.device("cuda", 0)
    bargs = argparse.Namespace(n=1183514, d=100, n_clusters=1087, seed=10, build_probes=1, metric="angular",
                               data="glove-like", fit_sample=100000, cache_dir=args.cache_dir)
    ivf, cent = bench.build_index(bargs, device)
    qs = bench.synth_queries(cent, args.nq, bargs.seed + 1, kind="glove-like")
    qn, qp = ivf._prepare(qs.copy())
    dev = ivf.device_index()
    is64 = int(qp.dtype != np.float32)
    stream = torch.cuda.current_stream().cuda_stream
    sink = open(args.out, "a") if args.out else None

    def emit(line):
        print(json.dumps(line), flush=True)
        if sink:
            sink.write(json.dumps(line) + "\n")
            sink.flush()

    # ---- pipelined calls, as the headline
    batches = []
    for _ in range(4):
        batches.append(dict(q=torch.from_numpy(np.ascontiguousarray(qn)).to(device),
                            qp=torch.from_numpy(np.ascontiguousarray(qp)).to(device),
                            out=torch.full((args.nq, args.k), -1, dtype=torch.int64, device=device),
                            dist=torch.full((args.nq, args.k), -1.0, dtype=torch.float32, device=device)))
    dev.set_pipeline(2)
    dev.set_coalesce(2)
    dev.reserve(2 * args.nq, args.k, args.n_probes)

    def rate(with_dist):
        n = [0]

        def step(ev=None):
            b = batches[n[0] % len(batches)]
            n[0] += 1
            dev.query_batch_dev(b["q"].data_ptr(), b["qp"].data_ptr(), is64, args.nq, args.k, args.n_probes,
                                b["out"].data_ptr(), stream=stream, done_event=ev,
                                dist_ptr=b["dist"].data_ptr() if with_dist else None)

        for _ in range(48):
            step()
        dev.join(stream)
        torch.cuda.synchronize()
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.windows + 1)]
        for e in evs:
            e.record()
        torch.cuda.synchronize()
        evs[0].record()
        for w in range(args.windows):
            for i in range(args.steps):
                step(evs[w + 1].cuda_event if i == args.steps - 1 else None)
        dev.join(stream)
        torch.cuda.synchronize()
        ms = sorted(evs[w].elapsed_time(evs[w + 1]) for w in range(1, args.windows))
        return args.nq / (ms[len(ms) // 2] / args.steps * 1e-3)

    ids_only, with_dist = [], []
    for r in range(args.runs):
        ids_only.append(rate(False))
        ref = [b["out"].cpu().numpy().copy() for b in batches]
        with_dist.append(rate(True))
        same = all(np.array_equal(b["out"].cpu().numpy(), x) for b, x in zip(batches, ref))
        emit(dict(bench="dist", leg="pipelined", run=r, nq=args.nq, k=args.k, n_probes=args.n_probes,
                  qps_ids=ids_only[-1], qps_dist=with_dist[-1], same=same))
    mi, md = float(np.median(ids_only)), float(np.median(with_dist))
    emit(dict(bench="dist", leg="pipelined", summary=True, qps_ids_median=mi, qps_dist_median=md,
              cost_pct=100.0 * (mi - md) / mi))
    dev.set_coalesce(1)
    dev.set_pipeline(1)

    # ---- IVF.query_batch per call
    for nq in args.per_call:
        x = qs[:nq]
        t_ids, t_dist = [], []
        for r in range(args.reps + 3):
            t0 = time.perf_counter()
            a = ivf.query_batch(x, args.k, n_probes=args.n_probes)
            t1 = time.perf_counter()
            b, _ = ivf.query_batch(x, args.k, n_probes=args.n_probes, return_distances=True)
            t2 = time.perf_counter()
            if r >= 3:
                t_ids.append(t1 - t0)
                t_dist.append(t2 - t1)
        emit(dict(bench="dist", leg="per_call", nq=nq, k=args.k, n_probes=args.n_probes, reps=args.reps,
                  ms_ids=1e3 * float(np.median(t_ids)), ms_dist=1e3 * float(np.median(t_dist)),
                  same=bool(np.array_equal(a, b))))


if __name__ == "__main__":
    main()
