"""Indexes of a chosen PQ width: M = dq / dims_per_block blocks for any dims_per_block the C ABI takes (1 .. 32) and
any M up to its 512 blocks, made by hand so that no k-means runs (FastPQ.fit rotates every input that is not 100-d
down to 64 dims and is slow at hundreds of blocks; use_kmeans=False is defined for dims_per_block 2 only).  The kernels
change form with M (plain_scan.hip: guarded / unguarded register shapes up to M = 52; adc_scan.hip: the LDS forms'
scan_form_gmax; tables.hip: the M <= 256 paths, the float64 LDS region past 64 KiB from M = 474), and the suite's
fitted indexes only ever have M <= 32 or M = 52 with dims_per_block 2.

The codebook is sampled from the data (per block: 16 rows of the padded, rotated data plus a little noise) and
assembled exactly as FastPQ.fit assembles its own, so dims_per_block = 1 leaves the F-ordered view fit leaves.  The
coarse centres are sampled rows.  Everything else — list assignment, encoding, packing — is IVF.build's host code."""
import numpy as np


def handmade_index(metric, d, dpb, n_lists, n, nq, seed, f64=False, rot=None, M=None):
    """-> (ivf, qs): a built IVF (host build) over n clustered rows of d dims and nq float32 queries from the same
    clusters.  rot: rotate to that many dims (an orthogonal float64 matrix cut to `rot` rows, as fit cuts its own).
    f64: float64 rows (float64 rescoring) AND float64 table-build queries: the product makes q_pq float64 only
    through `q @ R.T`, so where no `rot` is asked for R is the identity — every product is x * 1 or x * 0 and every
    sum exact, in any order: q_pq is the float32 query widened.  M: the block count the caller expects (asserted)."""
    from tinyknn_amd import IVF, FastPQ
    from tinyknn_amd.fast_pq import dpad
    from tinyknn_amd.utils import pad2
    rng = np.random.RandomState(seed)
    cent = rng.randn(40, d)
    X = (cent[rng.randint(40, size=n)] + 0.5 * rng.randn(n, d)).astype(np.float64 if f64 else np.float32)
    qs = (cent[rng.randint(40, size=nq)] + 0.5 * rng.randn(nq, d)).astype(np.float32)
    rows = X / np.linalg.norm(X, axis=1, keepdims=True) if metric == "angular" else X
    pq = FastPQ(dpb, rotate_dim=None)
    ivf = IVF(metric, n_lists, pq)                      # (wants its PQ unfitted)
    ivf.all_centers = np.ascontiguousarray(rows[rng.choice(n, n_lists, replace=False)], dtype=np.float32)
    P = pad2(rows, 16, dpad * dpb)
    if rot is not None:
        q, _ = np.linalg.qr(rng.randn(P.shape[1], P.shape[1]))
        pq.R = np.ascontiguousarray(q.T[:rot], dtype=np.float64)
    elif f64:
        pq.R = np.eye(P.shape[1], dtype=np.float64)
    if pq.R is not None:
        P = P @ pq.R.T
    dq = P.shape[1]
    assert dq % dpb == 0
    blocks = dq // dpb
    assert M is None or blocks == M, (d, dpb, rot, blocks, M)
    pick = rng.randint(n, size=(blocks, 16))                   # (not the zero rows that pad P to 16)
    books = P.reshape(len(P), blocks, dpb)[pick, np.arange(blocks)[:, None]] + 0.01 * rng.randn(blocks, 16, dpb)
    pq.centers = np.array(list(books), dtype=np.float32).transpose(1, 0, 2).reshape(16, dq)   # fast_pq.py:99-102
    assert pq.centers.flags.c_contiguous == (dpb != 1)
    pq.sqrt_n_blocks = np.sqrt(blocks)
    ivf.build(X, n_probes=1, device=False)
    assert len(ivf.active_centers) == n_lists
    return ivf, qs


def oracle_index(oracle, ivf):
    """The CPU oracle's copy of a built index, with the index's own dims_per_block."""
    L = len(ivf.active_centers)
    return oracle.OracleIndex(ivf.pq.centers, ivf.pq.dims_per_block, ivf.pq.R, ivf.pq.sqrt_n_blocks,
                              ivf.active_centers, ivf.pq_transformed_centers.packed,
                              [ivf.pq_transformed_points[i].packed for i in range(L)],
                              [ivf.pq_transformed_points[i].size for i in range(L)],
                              [ivf.ids[i] for i in range(L)], ivf.data)


def oracle_answers(ox, qn, k, n_probes, pass_1=None):
    """The oracle's per-query ids (padded with -1 to k), probe lists and heap arrays, stacked over the batch."""
    ids, probes, hidx, hval = [], [], [], []
    for q in qn:
        got, dbg = ox.query(q, k, n_probes=n_probes, pass_1=pass_1, debug=True)
        ids.append(np.concatenate([got, np.full(k - len(got), -1, dtype=np.int64)]))
        probes.append(dbg["probes"])
        hidx.append(dbg["heap_idx"])
        hval.append(dbg["heap_val"])
    return dict(ids=np.stack(ids), probes=np.stack(probes), heap_idx=np.stack(hidx), heap_val=np.stack(hval))
