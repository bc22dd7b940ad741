#!/usr/bin/env python
"""CPU model of the lane replay's insert rounds per wave (heap.hip, heap_replay_lanes_kernel; numpy + heapq, no GPU).

A wave replays 64 queries, one per lane; a ROUND is one insert step of the wave: every lane with a pending row
inserts one.  The kernel's time is its rounds (a latency chain), so what a staging scheme costs is how
many rounds a wave spends waiting for its slowest lane:

  segments of S blocks, lanes in step     sum over segments of the max over lanes of the inserts in the segment
  lanes not in step at all                max over lanes of the query's inserts
  per-lane ring (RING)                    the kernel's loop: refills every T rounds or when no lane has a pending
                                          row; per refill a lane drops what it requested a refill ago into its ring
                                          of 8 slots, moves its cursor over at most two windows of 16 block minima
                                          and requests up to `loads` blocks whose minimum is below its bound of now

Data: a quarter-size stand-in of the benchmark's workload: 296 000 x 100 rows in 75 Gaussian clusters (sigma 0.7),
normalised, 272 k-means lists, 1 024 queries, n_probes = 10, R = 111.  A row's value: its squared distance to the
query plus noise (the PQ error), mapped to int8 so that the 111th best probed row sits near -90.  The reference's
loop per block: bound captured at block start, strict <, replace-root insert (_fast_pq_256.pyx:65-123).

    python scripts/sim_replay_rounds.py [--quick]
"""
import argparse
import heapq

import numpy as np


def workload(n, n_clusters, n_lists, nq, n_probes, R, rng, noise=0.10):
    d = 100
    cent = rng.standard_normal((n_clusters, d))
    X = cent[rng.integers(n_clusters, size=n)] + 0.7 * rng.standard_normal((n, d))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    Q = cent[rng.integers(n_clusters, size=nq)] + 0.7 * rng.standard_normal((nq, d))
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    C = X[rng.choice(n, n_lists, replace=False)].copy()
    for _ in range(6):                                  # k-means
        a = np.concatenate([(X[i:i + 50000] @ C.T).argmax(axis=1) for i in range(0, n, 50000)])
        for c in range(n_lists):
            m = X[a == c]
            if len(m):
                C[c] = m.mean(axis=0)
        C /= np.linalg.norm(C, axis=1, keepdims=True)
    order = np.argsort(a, kind="stable")
    start = np.searchsorted(a[order], np.arange(n_lists + 1))
    queries = []
    for q in Q:
        probes = np.argsort(-(C @ q))[:n_probes]
        vals = []
        for l in probes:
            rows = X[order[start[l]:start[l + 1]]]
            dist = 2 - 2 * rows @ q + noise * rng.standard_normal(len(rows))
            pad = (-len(dist)) % 16
            vals.append(np.concatenate([dist, np.full(pad, np.inf)]))
        dist = np.concatenate(vals)
        fin = dist[np.isfinite(dist)]
        ref = np.partition(fin, R - 1)[R - 1]
        scale = 110.0 / max(np.median(fin) - ref, 1e-9)                  # the median probed row near +20
        v = np.where(np.isfinite(dist), np.clip(np.rint(-90 + scale * (dist - ref)), -128, 127), 127).astype(np.int64)
        queries.append(v.reshape(-1, 16))
    return queries


def reference_loop(blocks, R):
    """-> inserts per block, bound at every block's start (one more entry: the final bound), block minima."""
    heap = [-127] * R                       # max-heap of values by negation; a fresh heap holds the largest value
    ins = np.zeros(len(blocks), np.int64)
    bound = np.zeros(len(blocks) + 1, np.int64)
    for b, blk in enumerate(blocks):
        bd = -heap[0]
        bound[b] = bd
        for v in blk[blk < bd]:             # stale bound inside the block: every row below it goes in
            heapq.heapreplace(heap, -int(v))
            ins[b] += 1
    bound[-1] = -heap[0]
    return ins, bound, blocks.min(axis=1)


def rounds_in_step(wave, seg):
    n = max(len(q[0]) for q in wave)
    tot = 0
    for g in range(0, n, seg):
        tot += max(int(q[0][g:g + seg].sum()) for q in wave)
    return tot


def rounds_ring(wave, T=4, loads=4, slots=8, windows=2):
    """The kernel's loop.  -> (rounds, refills, blocks fetched per query)."""
    L = len(wave)
    ins, bound, mins = zip(*wave)
    nb = [len(x) for x in ins]
    nxt = [0] * L            # first block the cursor has not looked at
    wend = [0] * L           # end of the window the cursor is in
    ring = [[] for _ in range(L)]
    flight = [[] for _ in range(L)]
    left = [0] * L           # inserts left in the current block
    at = [0] * L             # bound index: the block the lane is in, or the one behind its last
    rounds = refills = fetched = since = 0
    while True:
        for i in range(L):
            while left[i] == 0 and ring[i]:
                b = ring[i].pop(0)
                left[i] = int(ins[i][b])
                at[i] = b if left[i] else b + 1
        pending = any(left)
        if not pending or since >= T:
            since = 0
            if any(flight[i] or nxt[i] < nb[i] for i in range(L)):
                refills += 1
                for i in range(L):
                    ring[i] += flight[i]
                    flight[i] = []
                    live = bound[i][at[i]]
                    room = min(slots - len(ring[i]), loads)
                    moved = 0
                    while room and nxt[i] < nb[i]:
                        if nxt[i] == wend[i]:
                            if moved == windows:
                                break
                            moved += 1
                            wend[i] = min(wend[i] + 16, nb[i])
                        while nxt[i] < wend[i] and room:
                            if mins[i][nxt[i]] < live:
                                flight[i].append(nxt[i])
                                room -= 1
                            nxt[i] += 1
                    fetched += len(flight[i])
                if not pending:
                    continue
            elif not pending:
                break
        rounds += 1
        since += 1
        for i in range(L):
            if left[i]:
                left[i] -= 1
                if left[i] == 0:
                    at[i] += 1
    return rounds, refills, fetched / L


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--quick", action="store_true", help="a sixteenth of the rows and 256 queries")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    n, lists, nq = (74000, 68, 256) if a.quick else (296000, 272, 1024)
    qs = [reference_loop(b, 111) for b in workload(n, 75, lists, nq, 10, 111, rng)]
    per_q = np.array([q[0].sum() for q in qs])
    print(f"inserts per query: mean {per_q.mean():.0f}, sd {per_q.std():.0f}; blocks per query: "
          f"{np.mean([len(q[0]) for q in qs]):.0f}")
    waves = [qs[i:i + 64] for i in range(0, len(qs), 64)]

    def mean(f):
        return np.mean([f(w) for w in waves], axis=0)
    print("| staging | rounds per wave | refills per wave | blocks fetched per query |")
    print("|---|---|---|---|")
    for seg in (8, 16, 32):
        print(f"| segments of {seg}, lanes in step | {mean(lambda w: rounds_in_step(w, seg)):.0f} | - | all |")
    print(f"| lanes not in step at all | {mean(lambda w: max(int(q[0].sum()) for q in w)):.0f} | - | - |")
    for T, loads, slots in ((4, 4, 8), (8, 4, 8), (4, 8, 8), (2, 4, 8), (4, 4, 4)):
        r = mean(lambda w: rounds_ring(w, T, loads, slots))
        print(f"| ring of {slots}, refill every {T} rounds, {loads} loads | {r[0]:.0f} | {r[1]:.0f} | {r[2]:.0f} |")


if __name__ == "__main__":
    main()
