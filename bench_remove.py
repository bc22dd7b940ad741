#!/usr/bin/env python3
"""bench_remove.py — IVF.remove (tk_index_remove_rows: rows deleted from the built lists in place) on the GloVe-shaped
index bench.py measures (bench.build_index: 1 183 514 x 100 angular, 1 087 clusters, built with IVF.build on the
device).  For kp = 1 and 2 lists per row and 1 000 / 10 000 / 100 000 removed rows (a seeded random choice), each
point starting from the same built index, two JSON lines.  path "host": the index IVF.build made, shrunk by
IVF.remove (the device compaction, then the host copy refreshed); path "resident": the same rows in HBM built by
tk_index_build_dev, shrunk by DeviceIndex.remove.  Both are compared with a fresh upload (tk_index_set_lists) of
their old lists filtered in numpy.
  remove_ms         host: IVF.remove end to end; resident: DeviceIndex.remove end to end
  remove_device_ms  host: the device compaction alone (DeviceIndex.remove / tk_index_remove_rows)
  remove_host_ms    host: the refresh of the host copy from the device (export_lists)
  lists_identical   the exported lists (sizes, codes, ids), list_columns and twin table width equal the fresh upload's
  qps_removed / qps_fresh / qps_allowed   pipelined query_batch_dev calls of --nq queries (pipeline 2, pairs of
                    calls, n_probes 10, k 10, as bench.py's headline) on the shrunk index, on the fresh upload, and on
                    the un-removed index with allowed= the survivors
  ids_identical     query rows whose ids are equal between the shrunk index and the fresh upload (of nq)

    python bench_remove.py --out profiles/r07/bench_remove.jsonl
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


def export_state(dev, cols=None):
    """(sizes, packed codes, ids, list_columns (cols, or the index's own), the zero vector's labels as the padding
    rows carry them)"""
    from tinyknn_amd._transform import unpack
    sizes, codes, ids = dev.export_lists()
    coff = np.concatenate([[0], np.cumsum((sizes + 15) // 16)])
    l = int(np.flatnonzero(sizes % 16)[0])
    zero = unpack(codes[coff[l]:coff[l + 1]])[sizes[l]]
    return sizes, codes, ids, dev.list_columns() if cols is None else cols, zero


def filtered(state, dead):
    """The lists of `state` with the dead rows dropped, in their old order, the zero vector's labels in the padding
    rows: (sizes, packed codes, ids, list_columns) — numpy only."""
    from tinyknn_amd._transform import transform_data, unpack
    sizes, codes, ids, cols, zero = state
    L, kp = cols.shape
    coff = np.concatenate([[0], np.cumsum((sizes + 15) // 16)])
    ioff = np.concatenate([[0], np.cumsum(sizes)])
    lst = np.repeat(np.arange(L), sizes)
    pos = np.arange(len(ids)) - ioff[lst]
    keep = ~dead[ids]
    col = np.concatenate([np.repeat(np.arange(kp), cols[i]) for i in range(L)])
    cols1 = np.zeros_like(cols)
    np.add.at(cols1, (lst[keep], col[keep]), 1)
    sizes1 = cols1.sum(axis=1)
    coff1 = np.concatenate([[0], np.cumsum((sizes1 + 15) // 16)])
    ioff1 = np.concatenate([[0], np.cumsum(sizes1)])
    ids1 = ids[keep]
    lst1 = lst[keep]
    lab = unpack(codes)
    lab1 = np.repeat(zero[None], 16 * int(coff1[-1]), axis=0)
    lab1[16 * coff1[lst1] + (np.arange(len(ids1)) - ioff1[lst1])] = lab[(16 * coff[lst] + pos)[keep]]
    return sizes1, transform_data(lab1), ids1, cols1


def upload(base, lists, data=None):
    """A fresh DeviceIndex (tk_index_set_lists) of `lists` with base's centres and codebook, and its vectors (or
    `data`)."""
    from tinyknn_amd.fast_pq import TransformedData
    from tinyknn_amd.ivf import DeviceIndex
    sizes, codes, ids, _ = lists
    coff = np.concatenate([[0], np.cumsum((sizes + 15) // 16)])
    ioff = np.concatenate([[0], np.cumsum(sizes)])
    d = base.data.shape[1]
    ref = copy.copy(base)
    ref._dev = None
    if data is not None:
        ref.data = data
    ref.pq_transformed_points = [TransformedData(int(sizes[i]), codes[coff[i]:coff[i + 1]]) if sizes[i]
                                 else np.empty((0, d)) for i in range(len(sizes))]
    ref.ids = [ids[ioff[i]:ioff[i + 1]] for i in range(len(sizes))]
    return DeviceIndex(ref)


def snapshot(ivf):
    """A copy of a host-built index that remove() may shrink without touching the original; no device copy yet."""
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
    ap.add_argument("--removes", type=int, nargs="+", default=[1000, 10000, 100000])
    ap.add_argument("--kp", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import bench
    from tinyknn_amd import IVF, FastPQ, _lib
    from tinyknn_amd.ivf import DeviceIndex
    assert _lib.device_count() >= 1, "bench_remove.py needs a GPU"
    device = torch.device("cuda", 0)
    bargs = argparse.Namespace(n=1183514, d=100, n_clusters=1087, seed=10, build_probes=1, metric="angular",
                               data="glove-like", fit_sample=100000, cache_dir=None)
    X, _ = bench.synth_cached(bargs)
    base1, cent = bench.build_index(bargs, device)
    N = len(X)
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

    def qps(dev, aset=None):
        """queries/s of the timed pass; the warm-up is a whole pass: the first calls on an index just made or just
        changed set up its workspaces and plain-scan verdicts"""
        dev.set_pipeline(2)
        dev.set_coalesce(2)
        for i in range(max(args.warmup, args.steps)):
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
        r = args.steps * args.nq / (time.perf_counter() - t0)
        return r, outs[-1].cpu().numpy()

    def identical(dev, fresh, cols):
        """lists_identical and its parts: exported lists, list_columns, twin table"""
        parts = dict(exports_identical=all(np.array_equal(u, v) for u, v in zip(dev.export_lists(), fresh.export_lists())),
                     columns_identical=bool(np.array_equal(dev.list_columns(), cols)),
                     twins_identical=dev.twin_table_width() == fresh.twin_table_width()
                     and all(np.array_equal(u, v) for u, v in zip(dev.twin_table(), fresh.twin_table())))
        return dict(lists_identical=all(parts.values()), twin_width=dev.twin_table_width(),
                    fresh_twin_width=fresh.twin_table_width(), **parts)

    for kp in args.kp:
        if kp == 1:
            base = base1
        else:
            base = IVF(bargs.metric, bargs.n_clusters, FastPQ(2))
            base.all_centers, base.pq = base1.all_centers, base1.pq
            base.build(X, n_probes=kp, device=True)
        whole = snapshot(base)
        wd = whole.device_index()                 # the un-removed index, for allowed= the survivors
        state = export_state(wd, base.list_columns)
        rd = DeviceIndex.resident(base, N, bargs.d)
        assert hip.hipMemcpy(rd.data_ptr, X.ctypes.data, X.nbytes, 1) == 0
        rd.build_dev(base.all_centers, kp)
        rstate = export_state(rd)
        rd.close()
        for n in args.removes:
            R = np.random.RandomState(bargs.seed + n + kp).choice(N, n, replace=False)
            dead = np.zeros(N, bool)
            dead[R] = True
            lists = filtered(state, dead)
            # ---- host: the index IVF.build made, shrunk by IVF.remove
            shrunk = snapshot(base)
            dev = shrunk.device_index()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            shrunk.remove(R)
            remove_ms = 1e3 * (time.perf_counter() - t0)
            parts = dict(shrunk.last_remove_ms)
            fresh = upload(base, lists)
            same = identical(dev, fresh, lists[3])
            q_removed, ids_removed = qps(dev)
            q_fresh, ids_fresh = qps(fresh)
            q_removed2, _ = qps(dev)                  # (again, after the fresh one: the spread of the pair)
            dev.close()
            fresh.close()
            aset = wd.allow(~dead)
            q_allowed, _ = qps(wd, aset)
            aset.close()
            emit(dict(bench="remove", path="host", kp=kp, n_index=N, n_remove=n, remove_ms=remove_ms,
                      remove_device_ms=parts.get("device"), remove_host_ms=parts.get("host"), **same,
                      qps_removed=q_removed, qps_removed_again=q_removed2, qps_fresh=q_fresh, qps_allowed=q_allowed, nq=args.nq,
                      n_probes=args.n_probes, k=args.k, steps=args.steps,
                      ids_identical=int((ids_removed == ids_fresh).all(axis=1).sum())))
            # ---- resident: vectors in HBM, built by tk_index_build_dev, shrunk by DeviceIndex.remove
            rd = DeviceIndex.resident(base, N, bargs.d)
            assert hip.hipMemcpy(rd.data_ptr, X.ctypes.data, X.nbytes, 1) == 0
            rd.build_dev(base.all_centers, kp)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rd.remove(R)
            remove_ms = 1e3 * (time.perf_counter() - t0)
            rlists = filtered(rstate, dead)
            fresh = upload(base, rlists, rd.read_rows(np.arange(N)))     # (the vectors as the device normalised them)
            same = identical(rd, fresh, rlists[3])
            q_removed, ids_removed = qps(rd)
            q_fresh, ids_fresh = qps(fresh)
            q_removed2, _ = qps(rd)
            rd.close()
            fresh.close()
            emit(dict(bench="remove", path="resident", kp=kp, n_index=N, n_remove=n, remove_ms=remove_ms,
                      remove_device_ms=remove_ms, remove_host_ms=0.0, **same,
                      qps_removed=q_removed, qps_removed_again=q_removed2, qps_fresh=q_fresh, qps_allowed=None, nq=args.nq,
                      n_probes=args.n_probes, k=args.k, steps=args.steps,
                      ids_identical=int((ids_removed == ids_fresh).all(axis=1).sum())))
        wd.close()


if __name__ == "__main__":
    main()
