#!/usr/bin/env python3
"""bench_store.py — the half store of the rescoring vectors (store="float16") against the
float32 store on the GloVe-shaped index bench.py measures (bench.build_index): ONE IVF, two device indexes.
Prints one JSON line per point:
  bytes       the vectors' bytes in HBM under both stores
  pipelined   query_batch_dev calls of --nq queries, n_probes 10, k 10, pipeline 2 and pairs of calls as bench.py's
              headline runs them: float32 store against half store in alternating runs (queries/s of the median
              window of each run, as bench.timed_rate); `same_as_twin` = the half index's last ids were those of the
              float32 twin (a float32 index holding float32(float16(x)))
  stage       the final rescoring alone, ms per --nq queries with one batch in flight (set_profiling /
              last_profile()["rescore"]), both stores, alternating
  recall      Recall10@10 of both stores against knn_brute of the float32 index, and the share of queries whose id
              rows are identical under the two stores (reported: the rounding is the format's, 2^-11 relative)

    python bench_store.py --runs 3 --out profiles/r07/bench_store.jsonl
"""
import argparse
import copy
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3, help="alternating (float32, float16) runs of each leg")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--n-probes", type=int, default=10)
    ap.add_argument("--recall-queries", type=int, default=1000)
    ap.add_argument("--cache-dir", default=os.environ.get("TMPDIR", "/tmp"))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import bench
    from tinyknn_amd import _lib
    from tinyknn_amd.ivf import DeviceIndex
    assert _lib.device_count() >= 1, "bench_store.py needs a GPU"
    device = torch.device("cuda", 0)
    bargs = argparse.Namespace(n=1183514, d=100, n_clusters=1087, seed=10, build_probes=1, metric="angular",
                               data="glove-like", fit_sample=100000, cache_dir=args.cache_dir)
    ivf, cent = bench.build_index(bargs, device)
    qs = bench.synth_queries(cent, args.nq, bargs.seed + 1, kind="glove-like")
    qn, qp = ivf._prepare(qs.copy())
    devs = {"float32": DeviceIndex(ivf), "float16": DeviceIndex(ivf, store="float16")}
    is64 = int(qp.dtype != np.float32)
    stream = torch.cuda.current_stream().cuda_stream
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    sink = open(args.out, "a") if args.out else None

    def emit(line):
        print(json.dumps(line), flush=True)
        if sink:
            sink.write(json.dumps(line) + "\n")
            sink.flush()

    emit(dict(bench="store", leg="bytes", n=bargs.n, d=bargs.d,
              **{f"vector_bytes_{s}": int(d.vector_bytes) for s, d in devs.items()},
              code_bytes=int(devs["float32"].code_bytes)))

    batches = []
    for _ in range(4):
        batches.append(dict(q=torch.from_numpy(np.ascontiguousarray(qn)).to(device),
                            qp=torch.from_numpy(np.ascontiguousarray(qp)).to(device),
                            out=torch.full((args.nq, args.k), -1, dtype=torch.int64, device=device)))

    # ---- the float32 twin's ids of these queries (one call; its vectors leave HBM again)
    tw = copy.copy(ivf)
    tw._dev, tw.store = None, None
    tw.data = np.asarray(ivf.data, dtype=np.float32).astype(np.float16).astype(np.float32)
    tdev = DeviceIndex(tw)
    tdev.query_batch_dev(batches[0]["q"].data_ptr(), batches[0]["qp"].data_ptr(), is64, args.nq, args.k, args.n_probes,
                         batches[0]["out"].data_ptr(), stream=stream)
    tdev.join(stream)
    torch.cuda.synchronize()
    twin_ids = batches[0]["out"].cpu().numpy().copy()
    tdev.close()
    del tw, tdev

    # ---- pipelined calls, as the headline
    def rate(dev):
        dev.set_pipeline(2)
        dev.set_coalesce(2)
        dev.reserve(2 * args.nq, args.k, args.n_probes)
        n = [0]

        def step(ev=None):
            b = batches[n[0] % len(batches)]
            n[0] += 1
            dev.query_batch_dev(b["q"].data_ptr(), b["qp"].data_ptr(), is64, args.nq, args.k, args.n_probes,
                                b["out"].data_ptr(), stream=stream, done_event=ev)

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

    qps = {"float32": [], "float16": []}
    for r in range(args.runs):
        qps["float32"].append(rate(devs["float32"]))
        ids32 = [b["out"].cpu().numpy().copy() for b in batches]
        qps["float16"].append(rate(devs["float16"]))
        ids16 = [b["out"].cpu().numpy().copy() for b in batches]
        emit(dict(bench="store", leg="pipelined", run=r, nq=args.nq, k=args.k, n_probes=args.n_probes,
                  qps_float32=qps["float32"][-1], qps_float16=qps["float16"][-1],
                  same_as_twin=all(np.array_equal(x, twin_ids) for x in ids16),
                  rows_identical_to_float32=float(np.mean([(a == b).all(axis=1).mean() for a, b in zip(ids16, ids32)]))))
    m32, m16 = float(np.median(qps["float32"])), float(np.median(qps["float16"]))
    spread32 = float(max(qps["float32"]) - min(qps["float32"]))
    emit(dict(bench="store", leg="pipelined", summary=True, qps_float32_median=m32, qps_float16_median=m16,
              float32_spread=spread32, gain_pct=100.0 * (m16 - m32) / m32, not_slower=bool(m16 >= m32 - spread32)))

    # ---- the rescoring stage alone: one batch in flight, HIP events around the stages
    def stage_ms(dev):
        dev.set_coalesce(1)
        dev.set_pipeline(1)
        dev.reserve(args.nq, args.k, args.n_probes)
        b = batches[0]

        def step():
            dev.query_batch_dev(b["q"].data_ptr(), b["qp"].data_ptr(), is64, args.nq, args.k, args.n_probes,
                                b["out"].data_ptr(), stream=stream)

        for _ in range(3):
            step()
        torch.cuda.synchronize()
        dev.set_profiling(True)
        for _ in range(10):
            step()
        dev.join(stream)
        torch.cuda.synchronize()
        stages, _, n_prof = dev.last_profile()
        dev.set_profiling(False)
        return stages, n_prof

    st = {"float32": [], "float16": []}
    for r in range(args.runs):
        for s in ("float32", "float16"):
            stages, n_prof = stage_ms(devs[s])
            st[s].append(stages["rescore"])
            emit(dict(bench="store", leg="stage", run=r, store=s, nq=args.nq, batches=n_prof,
                      **{f"{k}_ms": float(v) for k, v in stages.items()}))
    s32, s16 = float(np.median(st["float32"])), float(np.median(st["float16"]))
    emit(dict(bench="store", leg="stage", summary=True, rescore_ms_float32=s32, rescore_ms_float16=s16,
              ratio=s16 / s32 if s32 else None, lower=bool(s16 < s32)))

    # ---- recall against the exact neighbours on the float32 vectors
    rs = min(args.recall_queries, args.nq)
    truth = devs["float32"].knn_brute(qn[:rs], args.k)
    got = {s: d.query_batch(qn[:rs], qp[:rs], args.k, args.n_probes) for s, d in devs.items()}

    def recall(ids):
        return float(np.mean([len(np.intersect1d(ids[i], truth[i])) / args.k for i in range(rs)]))

    emit(dict(bench="store", leg="recall", queries=rs, k=args.k, n_probes=args.n_probes,
              recall_float32=recall(got["float32"]), recall_float16=recall(got["float16"]),
              rows_identical=float((got["float32"] == got["float16"]).all(axis=1).mean()),
              ids_identical=float((got["float32"] == got["float16"]).mean())))


if __name__ == "__main__":
    main()
