#!/usr/bin/env python3
"""bench_update.py — IVF.update (tk_index_update_rows: stored rows replaced in place, ids kept) against the route it
replaces, remove(ids) then add(X), on the GloVe-shaped index bench.py measures (bench.build_index: 1 183 514 x 100
angular, 1 087 clusters, built with IVF.build on the device) — the index and protocol of bench_add.py and
bench_remove.py.  For kp = 1 and 2 lists per row and 1 000 / 10 000 / 100 000 replaced rows (a seeded random choice
of distinct ids, fresh rows from the generator), two JSON lines per point.  path "host": the index IVF.build made,
changed by IVF.update, or by IVF.remove + IVF.add (the device calls, then the host copy refreshed); path "resident":
the same rows in HBM built by tk_index_build_dev, changed by DeviceIndex.update, or by DeviceIndex.remove +
DeviceIndex.add.  Both routes start from the same index, made again for every run, in the same process, the runs
alternating; the medians of --reps runs are reported with their smallest and largest run.
  update_ms / update_device_ms / update_host_ms    IVF.update (DeviceIndex.update) end to end, the device call alone,
                    the refresh of the host copy (resident: 0)
  remove_add_ms / remove_add_device_ms / remove_add_host_ms   the same for remove(ids) then add(X), both calls summed
  *_min / *_max     the spread of the --reps runs behind each median
  lists_identical   the updated index's exported lists (sizes, codes, ids), list_columns and twin table equal a fresh
                    upload (tk_index_set_lists) of the reference lists of tests/update_reference.py; the rows'
                    assignment and labels are read off the remove + add index (the parent's code)
  vector_bytes_update / vector_bytes_remove_add / n_after_*   the vector store after either route, and its rows
  qps_updated / qps_fresh   pipelined query_batch_dev calls of --nq queries (pipeline 2, pairs of calls, n_probes 10,
                    k 10, as bench.py's headline) on the updated index and on the fresh upload
  ids_identical     query rows whose ids are equal between the two (of nq)

    python bench_update.py --out profiles/r14/bench_update.jsonl
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def lists_of(state):
    """export_state's flat arrays as update_reference's snapshot: (ids per list, labels per list, list_columns, zero)"""
    from tinyknn_amd._transform import unpack
    sizes, codes, ids, cols, zero = state
    coff = np.concatenate([[0], np.cumsum((sizes + 15) // 16)])
    ioff = np.concatenate([[0], np.cumsum(sizes)])
    lab = unpack(codes)
    return ([ids[ioff[i]:ioff[i + 1]] for i in range(len(sizes))],
            [lab[16 * coff[i]:16 * coff[i] + sizes[i]] for i in range(len(sizes))], cols, zero)


def flat(lists, zero):
    """update_reference's lists as upload() takes them: (sizes, packed codes, ids, list_columns)"""
    from tinyknn_amd._transform import transform_data
    ids_l, lab_l, cols = lists
    sizes = np.array([len(a) for a in ids_l], dtype=np.int64)
    coff = np.concatenate([[0], np.cumsum((sizes + 15) // 16)])
    lab = np.repeat(zero[None], 16 * int(coff[-1]), axis=0)
    for i in range(len(sizes)):
        lab[16 * coff[i]:16 * coff[i] + sizes[i]] = lab_l[i]
    return sizes, transform_data(np.ascontiguousarray(lab)), np.concatenate(ids_l), cols


def spread(name, runs):
    return {name: float(np.median(runs)), name + "_min": float(min(runs)), name + "_max": float(max(runs))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--n-probes", type=int, default=10)
    ap.add_argument("--updates", type=int, nargs="+", default=[1000, 10000, 100000])
    ap.add_argument("--kp", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import bench
    from bench_remove import export_state, snapshot, upload
    from update_reference import assignment_of_added, updated_data, updated_lists
    from tinyknn_amd import IVF, FastPQ, _lib
    from tinyknn_amd.ivf import DeviceIndex
    assert _lib.device_count() >= 1, "bench_update.py needs a GPU"
    device = torch.device("cuda", 0)
    bargs = argparse.Namespace(n=1183514, d=100, n_clusters=1087, seed=10, build_probes=1, metric="angular",
                               data="glove-like", fit_sample=100000, cache_dir=None)
    X, _ = bench.synth_cached(bargs)
    base1, cent = bench.build_index(bargs, device)
    N, d = len(X), bargs.d
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
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

    def qps(dev):
        dev.set_pipeline(2)
        dev.set_coalesce(2)
        for i in range(max(args.warmup, args.steps)):
            dev.query_batch_dev(qn_t.data_ptr(), qp_t.data_ptr(), is64, args.nq, args.k, args.n_probes,
                                outs[i % len(outs)].data_ptr())
        dev.join()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for out in outs:
            dev.query_batch_dev(qn_t.data_ptr(), qp_t.data_ptr(), is64, args.nq, args.k, args.n_probes, out.data_ptr())
        dev.join()
        torch.cuda.synchronize()
        r = args.steps * args.nq / (time.perf_counter() - t0)
        return r, outs[-1].cpu().numpy()

    def identical(dev, fresh, cols):
        parts = dict(exports_identical=all(np.array_equal(u, v) for u, v in zip(dev.export_lists(), fresh.export_lists())),
                     columns_identical=bool(np.array_equal(dev.list_columns(), cols)),
                     twins_identical=dev.twin_table_width() == fresh.twin_table_width()
                     and all(np.array_equal(np.sort(u, axis=-1), np.sort(v, axis=-1))
                             for u, v in zip(dev.twin_table(), fresh.twin_table())))
        return dict(lists_identical=all(parts.values()), twin_width=dev.twin_table_width(), **parts)

    def resident(base, kp):
        rd = DeviceIndex.resident(base, N, d)
        assert hip.hipMemcpy(rd.data_ptr, X.ctypes.data, X.nbytes, 1) == 0
        rd.build_dev(base.all_centers, kp)
        return rd

    def report(path, kp, n, t, dev_u, dev_ra, state, R, data0):
        """One point's line: the timings t, and the last run's two indexes (updated; removed + added) compared."""
        near, lab = assignment_of_added(lists_of(export_state(dev_ra)), N, n)
        new = dev_ra.read_rows(N + np.arange(n))
        want = updated_lists(lists_of(state), R, near, lab)
        fresh = upload(base_kp, flat(want, state[4]), updated_data(data0, R, new))
        same = identical(dev_u, fresh, want[2])
        same["vectors_identical"] = bool(np.array_equal(dev_u.read_rows(R), new))
        vb = dict(vector_bytes_update=dev_u.vector_bytes, vector_bytes_remove_add=dev_ra.vector_bytes,
                  n_after_update=dev_u.N, n_after_remove_add=dev_ra.N)
        dev_ra.close()
        q_u, ids_u = qps(dev_u)
        q_f, ids_f = qps(fresh)
        q_u2, _ = qps(dev_u)                          # (again, after the fresh one: the spread of the pair)
        dev_u.close()
        fresh.close()
        line = dict(bench="update", path=path, kp=kp, n_index=N, n_update=n, reps=args.reps)
        for key, runs in t.items():
            line.update(spread(key, runs))
        line.update(same)
        line.update(vb)
        line.update(qps_updated=q_u, qps_updated_again=q_u2, qps_fresh=q_f, nq=args.nq, n_probes=args.n_probes,
                    k=args.k, steps=args.steps, ids_identical=int((ids_u == ids_f).all(axis=1).sum()))
        emit(line)

    keys = ("update_ms", "update_device_ms", "update_host_ms", "remove_add_ms", "remove_add_device_ms",
            "remove_add_host_ms")
    for kp in args.kp:
        if kp == 1:
            base_kp = base1
        else:
            base_kp = IVF(bargs.metric, bargs.n_clusters, FastPQ(2))
            base_kp.all_centers, base_kp.pq = base1.all_centers, base1.pq
            base_kp.build(X, n_probes=kp, device=True)
        base = base_kp
        whole = snapshot(base).device_index()
        state = export_state(whole, base.list_columns)
        whole.close()
        rd = resident(base, kp)
        rstate = export_state(rd)
        rdata = rd.read_rows(np.arange(N))
        rd.close()
        for n in args.updates:
            R = np.random.RandomState(bargs.seed + n + kp).choice(N, n, replace=False).astype(np.int64)
            Xn = bench.synth_queries(cent, n, bargs.seed + 7 + n, kind="glove-like").astype(np.float32)
            # ---- host: the index IVF.build made, changed by IVF.update / by IVF.remove + IVF.add
            t = {key: [] for key in keys}
            for rep in range(args.reps):
                u = snapshot(base)
                u.data = base.data.copy()             # (update writes its rows in place)
                dev_u = u.device_index()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                u.update(R, Xn)
                t["update_ms"].append(1e3 * (time.perf_counter() - t0))
                t["update_device_ms"].append(u.last_update_ms["device"])
                t["update_host_ms"].append(u.last_update_ms["host"])
                v = snapshot(base)
                dev_ra = v.device_index()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                v.remove(R)
                v.add(Xn)
                t["remove_add_ms"].append(1e3 * (time.perf_counter() - t0))
                t["remove_add_device_ms"].append(v.last_remove_ms["device"] + v.last_add_ms["device"])
                t["remove_add_host_ms"].append(v.last_remove_ms["host"] + v.last_add_ms["host"])
                if rep + 1 < args.reps:
                    dev_u.close()
                    dev_ra.close()
            report("host", kp, n, t, dev_u, dev_ra, state, R, base.data)
            del u, v
            # ---- resident: vectors in HBM, built by tk_index_build_dev, changed by DeviceIndex.update / .remove + .add
            t = {key: [] for key in keys}
            for rep in range(args.reps):
                dev_u = resident(base, kp)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                dev_u.update(R, Xn, kp, normalise=True, all_centers=base.all_centers)
                ms = 1e3 * (time.perf_counter() - t0)
                t["update_ms"].append(ms)
                t["update_device_ms"].append(ms)
                t["update_host_ms"].append(0.0)
                dev_ra = resident(base, kp)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                dev_ra.remove(R)
                dev_ra.add(Xn, kp, normalise=True, all_centers=base.all_centers)
                ms = 1e3 * (time.perf_counter() - t0)
                t["remove_add_ms"].append(ms)
                t["remove_add_device_ms"].append(ms)
                t["remove_add_host_ms"].append(0.0)
                if rep + 1 < args.reps:
                    dev_u.close()
                    dev_ra.close()
            report("resident", kp, n, t, dev_u, dev_ra, rstate, R, rdata)


if __name__ == "__main__":
    main()
