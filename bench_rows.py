#!/usr/bin/env python3
"""bench_rows.py — neighbours of stored rows (IVF.query_rows / knn_graph, rows.hip) on the GloVe-shaped index bench.py
measures (bench.build_index): --nq stored rows per call, n_probes 10, k 10, pipelined query_batch_dev calls in pairs
(pipeline 2, pairs of calls, as bench.py's headline).  One JSON line per leg:
  ext / exclude   queries/s of query_batch_dev fed the gathered rows as external queries, without and with
                  exclude_ptr: --reps alternating runs of --steps calls each (host clock around calls that end in a
                  device synchronise), median and min..max of each
  flagged         queries of one batch the plain path flags for the exact re-scan, without and with the exclusion
  gather          gather_queries_dev alone per --nq rows (float32 store; --half: and the half store), device events
  table           the row-position table: bytes, and the wall time of the call that makes it over the same call after
  knn_graph       IVF.knn_graph over every row, wall time (--graph)
  parity          rows of a sample equal to the CPU reference (tests/rows_reference.py), per leg
The exclusion pass's own kernel time comes from a profiler run of this script (exclude_pass_kernel in the trace).

    python bench_rows.py --steps 20 --graph --half --out profiles/r08/bench_rows.jsonl
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--n-probes", type=int, default=10)
    ap.add_argument("--n", type=int, default=1183514)
    ap.add_argument("--parity-sample", type=int, default=50)
    ap.add_argument("--graph", action="store_true", help="time IVF.knn_graph over every row")
    ap.add_argument("--half", action="store_true", help="time the gather on a half store too")
    ap.add_argument("--cache-dir", default=os.environ.get("TMPDIR", "/tmp"))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import bench
    from allowed_reference import reference_index
    from rows_reference import excluded_batch
    from tinyknn_amd import _lib
    from tinyknn_amd.ivf import DeviceIndex
    assert _lib.device_count() >= 1, "bench_rows.py needs a GPU"
    device = torch.device("cuda", 0)
    bargs = argparse.Namespace(n=args.n, d=100, n_clusters=1087, seed=10, build_probes=1, metric="angular",
                               data="glove-like", fit_sample=100000, cache_dir=args.cache_dir)
    ivf, _ = bench.build_index(bargs, device)
    dev = ivf.device_index()
    ref = reference_index(ivf)
    N, k, P, nq = ivf.data.shape[0], args.k, args.n_probes, args.nq
    rng = np.random.default_rng(0)
    rows = rng.choice(N, nq, replace=False).astype(np.int64)
    sink = open(args.out, "a") if args.out else None

    def emit(**line):
        line = dict(bench="rows", nq=nq, n_probes=P, k=k, **line)
        print(json.dumps(line), flush=True)
        if sink:
            sink.write(json.dumps(line) + "\n")
            sink.flush()

    rows_t = torch.from_numpy(rows).to(device)
    is64 = int(dev.rotated())
    qn_t = torch.empty((nq, dev.d), dtype=torch.float32, device=device)
    qp_t = torch.empty((nq, dev.dq), dtype=torch.float64 if is64 else torch.float32, device=device)
    outs = [torch.full((nq, k), -1, dtype=torch.int64, device=device) for _ in range(args.steps)]

    # (f) the table: the first excluding call of the layout makes it; the same call again does not
    small = np.ascontiguousarray(rows[:16])

    def small_call():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev.query_rows(small, k, P)
        return time.perf_counter() - t0
    dev.query_rows(small, k, P, exclude_self=False)         # (workspaces sized, code objects loaded)
    assert not dev.row_table()["built"]
    first, again = small_call(), min(small_call() for _ in range(3))
    tab = dev.row_table()
    emit(leg="table", N=int(N), stored=tab["entries"], bytes=tab["bytes"], build_ms=1e3 * (first - again),
         call_with_build_ms=1e3 * first, call_ms=1e3 * again)

    # (d) the gather alone
    def gather_ms(d, reps=20):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        st = torch.cuda.current_stream().cuda_stream
        for _ in range(3):
            d.gather_queries_dev(rows_t.data_ptr(), nq, qn_t.data_ptr(), qp_t.data_ptr(), st)
        ev[0].record()
        for _ in range(reps):
            d.gather_queries_dev(rows_t.data_ptr(), nq, qn_t.data_ptr(), qp_t.data_ptr(), st)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / reps
    emit(leg="gather", store="float32", ms_per_call=gather_ms(dev))
    if args.half:
        hdev = DeviceIndex(ivf, store="float16")
        emit(leg="gather", store="float16", ms_per_call=gather_ms(hdev))
        hdev.close()
    dev.gather_queries_dev(rows_t.data_ptr(), nq, qn_t.data_ptr(), qp_t.data_ptr(),
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()

    # (a), (b) queries/s without and with the exclusion, alternating
    def timed(exclude):
        ex = rows_t.data_ptr() if exclude else None
        for i in range(args.warmup):
            dev.query_batch_dev(qn_t.data_ptr(), qp_t.data_ptr(), is64, nq, k, P, outs[i % len(outs)].data_ptr(),
                                exclude_ptr=ex)
        dev.join()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for out in outs:
            dev.query_batch_dev(qn_t.data_ptr(), qp_t.data_ptr(), is64, nq, k, P, out.data_ptr(), exclude_ptr=ex)
        dev.join()
        torch.cuda.synchronize()
        return args.steps * nq / (time.perf_counter() - t0)

    dev.set_pipeline(2)
    dev.set_coalesce(2)
    dev.set_plain_scan(True)
    runs = {False: [], True: []}
    got = {}
    for _ in range(args.reps):
        for exclude in (False, True):
            runs[exclude].append(timed(exclude))
            got[exclude] = outs[-1].cpu().numpy()
    state = dev.plain_stats()["state"]
    dev.set_pipeline(1)
    dev.set_coalesce(1)

    # (c) what the plain path flags in one batch
    def flagged(exclude):
        dev.set_plain_scan("always")
        dev.query_batch_dev(qn_t.data_ptr(), qp_t.data_ptr(), is64, nq, k, P, outs[0].data_ptr(),
                            exclude_ptr=rows_t.data_ptr() if exclude else None)
        torch.cuda.synchronize()
        n = dev.plain_stats()["flagged_queries"]
        dev.set_plain_scan(True)
        return int(n)
    nflag = {e: flagged(e) for e in (False, True)}

    # (g) parity of a sample, per leg
    ps = rng.permutation(nq)[:args.parity_sample]
    qn = qn_t.cpu().numpy()
    qp = qp_t.cpu().numpy() if is64 else None
    for exclude, leg in ((False, "ext"), (True, "exclude")):
        want = excluded_batch(None, ref, qn[ps], rows[ps] if exclude else None, k, P,
                              q_pq=None if qp is None else qp[ps])
        r = sorted(runs[exclude])
        emit(leg=leg, steps=args.steps, reps=args.reps, qps=r[len(r) // 2], qps_min=r[0], qps_max=r[-1],
             flagged=nflag[exclude], plain_state_after=state,
             returned_itself=int((got[exclude] == rows[:, None]).any(axis=1).sum()),
             parity=int((want == got[exclude][ps]).all(axis=1).sum()), parity_sample=len(ps))

    # (e) the whole graph
    if args.graph:
        ivf.knn_graph(k, P, chunk=nq)[:1]               # (buffers, workspaces)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ids = ivf.knn_graph(k, P, chunk=nq)
        dt = time.perf_counter() - t0
        gs = rng.permutation(N)[:args.parity_sample].astype(np.int64)
        gq, gp = dev.gather_queries(gs)
        want = excluded_batch(None, ref, gq, gs, k, P, q_pq=gp if is64 else None)
        emit(leg="knn_graph", N=int(N), chunk=nq, seconds=dt, rows_per_s=N / dt,
             returned_itself=int((ids == np.arange(N)[:, None]).any(axis=1).sum()),
             parity=int((want == ids[gs]).all(axis=1).sum()), parity_sample=len(gs))


if __name__ == "__main__":
    main()
