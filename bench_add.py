#!/usr/bin/env python3
"""bench_add.py — IVF.add (tk_index_add_rows: new rows merged into the built lists in place) on the GloVe-shaped
index bench.py measures (bench.build_index: 1 183 514 x 100 angular, 1 087 clusters, built with IVF.build on the
device).  For kp = 1 and 2 lists per row and 1 000 / 10 000 / 100 000 added rows (drawn like the index's rows),
each point starting from the same built index, two JSON lines.  path "host": the index IVF.build made, grown by
IVF.add and compared with IVF.build over all rows (whose order inside a list is numpy's unstable argsort's, so a
query whose heap meets tied estimates may keep other ids); path "resident": the same rows in HBM built by
tk_index_build_dev, grown by DeviceIndex.add (assignment and codes on the device) and compared with
tk_index_build_dev over all rows — the same layout byte for byte.
  add_ms          host: IVF.add end to end (normalisation, assignment, PQ labels, the device merge, the refresh of
                  the host copy); resident: DeviceIndex.add end to end
  add_device_ms   host: the device merge alone (DeviceIndex.add / tk_index_add_rows)
  add_host_ms     host: the refresh of the host copy from the device (export_lists)
  build_ms        host: IVF.build(device=True) over all N + n rows
  rebuild_dev_ms  resident: tk_index_build_dev over all N + n rows already in HBM
  lists_identical resident: the exported lists (sizes, codes, ids) of the grown and the rebuilt index are equal
  qps_grown / qps_fresh   pipelined query_batch_dev calls of --nq queries (pipeline 2, pairs of calls, n_probes 10,
                  k 10, as bench.py's headline) on the grown index and on the fresh one
  ids_identical   query rows whose ids are equal between the two (of nq)

    python bench_add.py --out profiles/r07/bench_add.jsonl
"""
import argparse
import copy
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def snapshot(ivf):
    """A copy of a host-built index that add() may grow without touching the original (add replaces the list
    entries and IVF.data, it never writes into their arrays); no device copy yet."""
    s = copy.copy(ivf)
    s.ids, s.pq_transformed_points = list(ivf.ids), list(ivf.pq_transformed_points)
    s._dev = None
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--n-probes", type=int, default=10)
    ap.add_argument("--adds", type=int, nargs="+", default=[1000, 10000, 100000])
    ap.add_argument("--kp", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--cache-dir", default=os.environ.get("TMPDIR", "/tmp"))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import bench
    from tinyknn_amd import IVF, FastPQ, _lib
    from tinyknn_amd.ivf import DeviceIndex
    assert _lib.device_count() >= 1, "bench_add.py needs a GPU"
    device = torch.device("cuda", 0)
    bargs = argparse.Namespace(n=1183514, d=100, n_clusters=1087, seed=10, build_probes=1, metric="angular",
                               data="glove-like", fit_sample=100000, cache_dir=None)
    X, _ = bench.synth_cached(bargs)
    base1, cent = bench.build_index(bargs, device)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    rng = np.random.RandomState(bargs.seed + 7)
    extra = max(args.adds)
    Xn = (cent[rng.randint(len(cent), size=extra)] + 0.7 * rng.randn(extra, bargs.d)).astype(np.float32)
    qs = bench.synth_queries(cent, args.nq, bargs.seed + 1, kind="glove-like")
    qn, qp = base1._prepare(qs.copy())
    qn_t = torch.from_numpy(np.ascontiguousarray(qn)).to(device)
    qp_t = torch.from_numpy(np.ascontiguousarray(qp)).to(device)
    is64 = int(qp.dtype != np.float32)
    outs = [torch.full((args.nq, args.k), -1, dtype=torch.int64, device=device) for _ in range(args.steps)]
    sink = open(args.out, "a") if args.out else None

    def emit(line):
        print(json.dumps(line), flush=True)
        if sink:
            sink.write(json.dumps(line) + "\n")
            sink.flush()

    def resident(rows, kp):
        """(index, ms): tk_index_build_dev over raw rows copied into HBM first (it normalises them); only the build
        is timed."""
        d = DeviceIndex.resident(base1, len(rows), bargs.d)
        assert hip.hipMemcpy(d.data_ptr, rows.ctypes.data, rows.nbytes, 1) == 0
        t0 = time.perf_counter()
        d.build_dev(base1.all_centers, kp)
        return d, 1e3 * (time.perf_counter() - t0)

    def qps(dev):
        dev.set_pipeline(2)
        dev.set_coalesce(2)
        for i in range(args.warmup):
            dev.query_batch_dev(qn_t.data_ptr(), qp_t.data_ptr(), is64, args.nq, args.k, args.n_probes,
                                outs[i % len(outs)].data_ptr())
        dev.join()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for out in outs:
            dev.query_batch_dev(qn_t.data_ptr(), qp_t.data_ptr(), is64, args.nq, args.k, args.n_probes,
                                out.data_ptr())
        dev.join()
        torch.cuda.synchronize()
        r = args.steps * args.nq / (time.perf_counter() - t0)
        return r, outs[-1].cpu().numpy()

    for kp in args.kp:
        if kp == 1:
            base = base1
        else:
            base = IVF(bargs.metric, bargs.n_clusters, FastPQ(2))
            base.all_centers, base.pq = base1.all_centers, base1.pq
            base.build(X, n_probes=kp, device=True)
        for n in args.adds:
            grown = snapshot(base)
            dev = grown.device_index()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            grown.add(Xn[:n])
            add_ms = 1e3 * (time.perf_counter() - t0)
            parts = dict(grown.last_add_ms)
            Xall = np.concatenate([X, Xn[:n]])
            fresh = IVF(bargs.metric, bargs.n_clusters, FastPQ(2))
            fresh.all_centers, fresh.pq = base.all_centers, base.pq
            t0 = time.perf_counter()
            fresh.build(Xall, n_probes=kp, device=True)
            build_ms = 1e3 * (time.perf_counter() - t0)
            q_grown, ids_grown = qps(dev)
            dev.close()
            fd = fresh.device_index()
            q_fresh, ids_fresh = qps(fd)
            fd.close()
            line = dict(bench="add", path="host", kp=kp, n_index=len(X), n_add=n, add_ms=add_ms,
                        add_device_ms=parts.get("device"), add_host_ms=parts.get("host"), build_ms=build_ms,
                        qps_grown=q_grown, qps_fresh=q_fresh, nq=args.nq, n_probes=args.n_probes, k=args.k,
                        steps=args.steps, ids_identical=int((ids_grown == ids_fresh).all(axis=1).sum()))
            emit(line)
            # the resident form: vectors in HBM, built by tk_index_build_dev; grown by DeviceIndex.add (assignment and
            # codes on the device) against tk_index_build_dev over all N + n rows — the same layout, byte for byte
            rdev, _ = resident(X, kp)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rdev.add(Xn[:n], kp, normalise=True, all_centers=base.all_centers)
            add_ms = 1e3 * (time.perf_counter() - t0)
            rfresh, rebuild_ms = resident(Xall, kp)
            q_grown, ids_grown = qps(rdev)
            q_fresh, ids_fresh = qps(rfresh)
            same = all(np.array_equal(u, v) for u, v in zip(rdev.export_lists(), rfresh.export_lists()))
            rdev.close()
            rfresh.close()
            emit(dict(bench="add", path="resident", kp=kp, n_index=len(X), n_add=n, add_ms=add_ms,
                      rebuild_dev_ms=rebuild_ms, add_over_rebuild_dev=add_ms / rebuild_ms, lists_identical=same,
                      qps_grown=q_grown, qps_fresh=q_fresh, nq=args.nq, n_probes=args.n_probes, k=args.k,
                      steps=args.steps, ids_identical=int((ids_grown == ids_fresh).all(axis=1).sum())))


if __name__ == "__main__":
    main()
