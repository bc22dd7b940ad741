#!/usr/bin/env python3
"""bench_tags.py — every query of a batch restricted to the rows that carry its tags (IVF.set_tags, tags_ptr=,
tk_index_query_batch_dev_ex4) on the GloVe-shaped index bench.py measures (bench.build_index): pipelined
query_batch_dev calls of --nq queries in pairs, n_probes 10, k 10, as bench_groups.py.
Legs, each in both modes ("any", "all"), one JSON line per leg and mode:
  1of64_1bit     64 tags, every row one of them; every query one tag (selectivity 1/64)
  3of64_1bit     every row three tags; every query one tag
  3of64_4bit     every row three tags; every query four tags
Every rate is the median of --runs alternating runs:
  qps            one tagged call per step: queries/s, host clock around --steps calls ending in a device synchronise
  qps_none       the same calls without a tag array
  qps_group      the same queries through group= with 64 groups, one per row (the 1of64 assignment as groups)
  parity         rows of the leg's output equal to the CPU reference (tests/tags_reference.py) over a sample of
                 --parity-sample queries
  table_bytes / row_bytes / table_ms   the tag table in list-position order, the tags by row id, and what the first
                 tagged call of a layout takes beyond a later one (table kernel + the device synchronise around it)
The tag pass's own kernel time comes from a profiler run of this script with --trace: single launches, one batch in
flight, of the tag pass in both modes and of the group pass over the same queries.

    python bench_tags.py --steps 20 --out profiles/r16/bench_tags.jsonl
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
    ap.add_argument("--trace", action="store_true", help="single launches of the tag and group passes (profiler runs)")
    ap.add_argument("--parity-sample", type=int, default=50)
    ap.add_argument("--cache-dir", default=os.environ.get("TMPDIR", "/tmp"))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import bench
    from allowed_reference import reference_index
    from tags_reference import tagged_batch
    from tinyknn_amd import _lib
    assert _lib.device_count() >= 1, "bench_tags.py needs a GPU"
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
    outs = [torch.full((args.nq, args.k), -1, dtype=torch.int64, device=device) for _ in range(args.steps)]
    sink = open(args.out, "a") if args.out else None

    def on_device(masks):
        return torch.from_numpy(np.ascontiguousarray(masks, dtype=U64).view(np.int64)).to(device)

    def call(out, restriction):
        dev.query_batch_dev(qn_t.data_ptr(), qp_t.data_ptr(), is64, args.nq, args.k, args.n_probes, out.data_ptr(),
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
        return args.steps * args.nq / (time.perf_counter() - t0)

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
    one = rng.integers(0, 64, N)                                    # 64 tags, one per row — and the same as groups
    three = np.zeros(N, dtype=U64)
    for _ in range(3):
        three |= U64(1) << rng.integers(0, 64, N).astype(U64)
    q_one = U64(1) << rng.integers(0, 64, args.nq).astype(U64)
    q_four = np.zeros(args.nq, dtype=U64)
    for _ in range(4):
        q_four |= U64(1) << rng.integers(0, 64, args.nq).astype(U64)
    q_group = np.log2(q_one.astype(np.float64)).astype(np.int32)    # the query's one tag as its group
    legs = [("1of64_1bit", U64(1) << one.astype(U64), q_one), ("3of64_1bit", three, q_one), ("3of64_4bit", three, q_four)]
    group_t = torch.from_numpy(q_group).to(device)
    ivf.set_groups(one.astype(np.int32))
    sample = rng.permutation(args.nq)[:args.parity_sample]

    if args.trace:
        tags, masks = legs[0][1], on_device(legs[0][2])
        ivf.set_tags(tags)
        pipelined(tags_ptr=masks.data_ptr(), tags_mode="any")
        single(4, tags_ptr=masks.data_ptr(), tags_mode="any")
        single(4, tags_ptr=masks.data_ptr(), tags_mode="all")
        single(4, group_ptr=group_t.data_ptr())
        print(json.dumps(dict(bench="tags", trace=True)), flush=True)
        return

    for name, tags, q_masks in legs:
        masks = on_device(q_masks)
        ivf.set_tags(tags)
        first = single(1, tags_ptr=masks.data_ptr(), tags_mode="any")[0]          # makes the table
        later = float(np.median(single(3, tags_ptr=masks.data_ptr(), tags_mode="any")))
        rates = {m: dict(qps=[], qps_none=[], qps_group=[]) for m in ("any", "all")}
        for _ in range(args.runs):                                  # alternating
            for mode in ("any", "all"):
                rates[mode]["qps"].append(pipelined(tags_ptr=masks.data_ptr(), tags_mode=mode))
                rates[mode]["qps_none"].append(pipelined())
                rates[mode]["qps_group"].append(pipelined(group_ptr=group_t.data_ptr()))
        t = dev.tag_table()
        for mode in ("any", "all"):
            pipelined(tags_ptr=masks.data_ptr(), tags_mode=mode)
            got = outs[-1].cpu().numpy()
            want = tagged_batch(None, ref, qn[sample], q_masks[sample], mode, tags, args.k, args.n_probes)
            line = dict(bench="tags", leg=name, mode=mode, nq=args.nq, n_probes=args.n_probes, k=args.k,
                        steps=args.steps, runs=args.runs,
                        **{n: float(np.median(v)) for n, v in rates[mode].items()},
                        **{n + "_runs": v for n, v in rates[mode].items()},
                        parity=int((want == got[sample]).all(axis=1).sum()), parity_sample=len(sample),
                        answered=float((got != -1).mean()), table_bytes=t["bytes"], row_bytes=t["row_bytes"],
                        table_ms=1e3 * (first - later), rows=int(N))
            print(json.dumps(line), flush=True)
            if sink:
                sink.write(json.dumps(line) + "\n")
                sink.flush()
    ivf.set_tags(None)
    ivf.set_groups(None)


if __name__ == "__main__":
    main()
