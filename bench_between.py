#!/usr/bin/env python3
"""bench_between.py — every query of a batch restricted to the rows whose values lie in its ranges (IVF.set_values,
between_ptr=, tk_index_query_batch_dev_ex5) on the GloVe-shaped index bench.py measures (bench.build_index): pipelined
query_batch_dev calls of --nq queries in pairs, n_probes 10, k 10, as bench_tags.py.
Legs, one JSON line per leg:
  f32_1of64      one float32 column of uniform values; every query its own window of selectivity 1/64
  f32_0.1        ... of selectivity 0.1
  f32_0.5        ... of selectivity 0.5
  i64_newer      one int64 timestamp column; every query "newer than" its own t (one-sided, selectivity about 0.1)
  two_columns    two float32 columns, both bounded (selectivity about 0.1)
  four_columns   four float32 columns, all bounded (selectivity about 0.1)
  sorted_lists   one int64 column sorted with the list id: whole lists pass or fail (a tenth of the lists)
Every rate is the median of --runs alternating runs:
  qps            one ranged call per step: queries/s, host clock around --steps calls ending in a device synchronise
  qps_none       the same calls without a range array
  qps_tags       the same queries through tags= ("any", one tag per row and per query) at the leg's selectivity
  qps_group      the same queries through group= at the leg's selectivity
  parity         rows of the leg's output equal to the CPU reference (tests/between_reference.py) over a sample of
                 --parity-sample queries
  table_bytes / row_bytes / table_ms   the value table in list-position order, the keys by row id, and what the first
                 ranged call of a layout takes beyond a later one (table kernels + the device synchronise around them)
The range pass's own kernel time comes from a profiler run of this script with --trace: single launches, one batch in
flight, of the range pass over one, two and four columns and of the tag pass over the same queries.

    python bench_between.py --steps 20 --out profiles/r17/bench_between.jsonl
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

U64 = np.uint64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--n-probes", type=int, default=10)
    ap.add_argument("--trace", action="store_true", help="single launches of the range and tag passes (profiler runs)")
    ap.add_argument("--parity-sample", type=int, default=50)
    ap.add_argument("--cache-dir", default=os.environ.get("TMPDIR", "/tmp"))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import bench
    from allowed_reference import reference_index
    from between_reference import ranged_batch
    from tinyknn_amd import _lib
    from tinyknn_amd.ivf import query_ranges, value_kind
    assert _lib.device_count() >= 1, "bench_between.py needs a GPU"
    device = torch.device("cuda", 0)
    bargs = argparse.Namespace(n=1183514, d=100, n_clusters=1087, seed=10, build_probes=1, metric="angular",
                               data="glove-like", fit_sample=100000, cache_dir=args.cache_dir)
    ivf, cent = bench.build_index(bargs, device)
    qs = bench.synth_queries(cent, args.nq, bargs.seed + 1, kind="glove-like")
    qn, qp = ivf._prepare(qs.copy())
    dev = ivf.device_index()
    ref = reference_index(ivf)
    N, nq = ivf.data.shape[0], args.nq
    qn_t = torch.from_numpy(np.ascontiguousarray(qn)).to(device)
    qp_t = torch.from_numpy(np.ascontiguousarray(qp)).to(device)
    is64 = int(qp.dtype != np.float32)
    outs = [torch.full((nq, args.k), -1, dtype=torch.int64, device=device) for _ in range(args.steps)]
    sink = open(args.out, "a") if args.out else None

    def call(out, restriction):
        dev.query_batch_dev(qn_t.data_ptr(), qp_t.data_ptr(), is64, nq, args.k, args.n_probes, out.data_ptr(),
                            **restriction)

    def pipelined(**restriction):
        """--steps calls of --nq queries between two drains"""
        dev.set_pipeline(2)
        dev.set_coalesce(2)
        dev.set_plain_scan(True)
        for i in range(args.warmup):
            call(outs[i % len(outs)], restriction)
        dev.join()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for out in outs:
            call(out, restriction)
        dev.join()
        torch.cuda.synchronize()
        return args.steps * nq / (time.perf_counter() - t0)

    def single(n=1, **restriction):
        """n calls with one batch in flight, each drained: one pass launch per call -> seconds per call"""
        dev.set_pipeline(1)
        dev.set_coalesce(1)
        dev.set_plain_scan(True)
        took = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call(outs[0], restriction)
            dev.join()
            torch.cuda.synchronize()
            took.append(time.perf_counter() - t0)
        return took

    rng = np.random.default_rng(0)
    L = len(ivf.active_centers)

    def windows(cols, width):
        """per query and column a window [u, u + width] inside [0, 1)"""
        lo = rng.random((nq, cols)) * (1 - width)
        return lo, lo + width

    uniform = rng.random((N, 4)).astype(np.float32)
    stamps = rng.integers(0, 10**9, N).astype(np.int64)
    first = np.zeros(N, dtype=np.int64)         # the (lowest) list every row is stored in
    for l in reversed(range(L)):
        first[np.asarray(ivf.ids[l], dtype=np.int64)] = l
    newer = (0.9e9 + (rng.random(nq) - 0.5) * 1e8).astype(np.int64)
    l0 = rng.integers(0, L - L // 10, nq).astype(np.int64)
    # (leg, values, (lo, hi), one tag / group per row and per query out of `share`: the leg's selectivity as 1 / share)
    legs = [("f32_1of64", uniform[:, 0], windows(1, 1 / 64), 64),
            ("f32_0.1", uniform[:, 0], windows(1, 0.1), 10),
            ("f32_0.5", uniform[:, 0], windows(1, 0.5), 2),
            ("i64_newer", stamps, (newer[:, None], None), 10),
            ("two_columns", uniform[:, :2], windows(2, 0.1 ** 0.5), 10),
            ("four_columns", uniform, windows(4, 0.1 ** 0.25), 10),
            ("sorted_lists", first, (l0[:, None], (l0 + L // 10 - 1)[:, None]), 10)]
    sample = rng.permutation(nq)[:args.parity_sample]

    def keys_on_device(values, between):
        v = np.asarray(values)
        keys = query_ranges(between, nq, 1 if v.ndim == 1 else v.shape[1], value_kind(v.dtype))
        return torch.from_numpy(keys).to(device)

    def same_share(share):
        """tags and groups of the leg's selectivity: every row one of `share`, every query one"""
        row, q = rng.integers(0, share, N), rng.integers(0, share, nq)
        ivf.set_tags(U64(1) << row.astype(U64))
        ivf.set_groups(row.astype(np.int32))
        masks = torch.from_numpy((U64(1) << q.astype(U64)).view(np.int64)).to(device)
        return masks, torch.from_numpy(q.astype(np.int32)).to(device)

    if args.trace:
        masks, _ = same_share(10)
        for name, values, between, _ in (legs[1], legs[4], legs[5]):
            ivf.set_values(values)
            keys = keys_on_device(values, between)
            pipelined(between_ptr=keys.data_ptr())
            single(4, between_ptr=keys.data_ptr())
        single(4, tags_ptr=masks.data_ptr(), tags_mode="any")
        print(json.dumps(dict(bench="between", trace=True)), flush=True)
        return

    for name, values, between, share in legs:
        keys = keys_on_device(values, between)
        masks, group_t = same_share(share)
        ivf.set_values(values)
        first_call = single(1, between_ptr=keys.data_ptr())[0]         # makes the table
        later = float(np.median(single(3, between_ptr=keys.data_ptr())))
        rates = dict(qps=[], qps_none=[], qps_tags=[], qps_group=[])
        for _ in range(args.runs):                                  # alternating
            rates["qps"].append(pipelined(between_ptr=keys.data_ptr()))
            rates["qps_none"].append(pipelined())
            rates["qps_tags"].append(pipelined(tags_ptr=masks.data_ptr(), tags_mode="any"))
            rates["qps_group"].append(pipelined(group_ptr=group_t.data_ptr()))
        t = dev.value_table()
        pipelined(between_ptr=keys.data_ptr())
        got = outs[-1].cpu().numpy()
        lo, hi = between
        want = ranged_batch(None, ref, qn[sample], (None if lo is None else lo[sample], None if hi is None else hi[sample]),
                            values, args.k, args.n_probes)
        line = dict(bench="between", leg=name, cols=t["cols"], dtype=str(np.asarray(values).dtype), nq=nq,
                    n_probes=args.n_probes, k=args.k, steps=args.steps, runs=args.runs, share=share,
                    **{n: float(np.median(v)) for n, v in rates.items()}, **{n + "_runs": v for n, v in rates.items()},
                    parity=int((want == got[sample]).all(axis=1).sum()), parity_sample=len(sample),
                    answered=float((got != -1).mean()), table_bytes=t["bytes"], row_bytes=t["row_bytes"],
                    table_ms=1e3 * (first_call - later), rows=int(N))
        print(json.dumps(line), flush=True)
        if sink:
            sink.write(json.dumps(line) + "\n")
            sink.flush()
    ivf.set_values(None)
    ivf.set_tags(None)
    ivf.set_groups(None)


if __name__ == "__main__":
    main()
