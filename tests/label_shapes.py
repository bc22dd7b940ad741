"""Indexes whose LABELS are chosen against the replays' duplicate test (`insert`, _fast_pq.pyx:284-287), made on the
host without a GPU.  IVF.build numbers its rows 0 .. n-1; the replay forms branch on what the labels and lists look
like — labels that fill the hash set's buckets, labels around 2**24, many copies per label, more lists than the
TWIN form's bitmap holds — and this module builds those shapes.

Relabelling is exact: give every row a new number (ids -> perm[ids], data[perm[i]] = data[i]) and the reference's
answers are perm of its former answers, bit for bit: `insert` compares labels only for equality, and the rescoring reads
the same vectors through the new numbers (tests/test_label_shapes_cpu.py asserts it for every permutation used)."""
import ctypes as C
import functools

import numpy as np


def relabelled(ivf, perm, n_rows):
    """The index `ivf` with row i renamed perm[i]: ids[i] = perm[ids[i]], `data` of n_rows rows whose row perm[i] is
    the old row i (the rest zero).  Codes, centres, PQ and metric are shared with `ivf`."""
    from tinyknn_amd import IVF
    perm = np.asarray(perm, dtype=np.int64)
    n, d = ivf.data.shape
    assert perm.shape == (n,) and perm.min() >= 0 and perm.max() < n_rows and len(np.unique(perm)) == n
    L = len(ivf.active_centers)
    out = IVF(ivf.metric, L, None)
    out.pq = ivf.pq
    out.active_centers = ivf.active_centers
    out.pq_transformed_centers = ivf.pq_transformed_centers
    out.pq_transformed_points = list(ivf.pq_transformed_points[:L])
    out.ids = [perm[np.asarray(ivf.ids[i], dtype=np.int64)] for i in range(L)]
    data = np.zeros((n_rows, d), dtype=ivf.data.dtype)
    data[perm] = ivf.data
    out.data = data
    return out


def oracle_of(oracle, ivf):
    """The CPU oracle over the arrays of a built (or relabelled) index."""
    L = len(ivf.active_centers)
    return oracle.OracleIndex(ivf.pq.centers, ivf.pq.dims_per_block, ivf.pq.R, ivf.pq.sqrt_n_blocks,
                              ivf.active_centers, ivf.pq_transformed_centers.packed,
                              [ivf.pq_transformed_points[i].packed for i in range(L)],
                              [ivf.pq_transformed_points[i].size for i in range(L)],
                              [ivf.ids[i] for i in range(L)], ivf.data)


@functools.lru_cache(maxsize=None)
def _buckets_below(below):
    """(b1, b2) of every label < below, from the library's own function (tk_label_buckets: no device needed)"""
    from tinyknn_amd import _lib
    fn = _lib.lib().tk_label_buckets
    a, b = C.c_int32(), C.c_int32()
    out = np.zeros((below, 2), dtype=np.int64)
    for label in range(below):
        assert fn(label, C.byref(a), C.byref(b)) == 0
        out[label] = a.value, b.value
    assert ((out >= 0) & (out < 64)).all() and (out[:, 0] != out[:, 1]).all()
    return out


def labels_in_buckets(B, below):
    """-> (labels, capacity): the labels < below whose two buckets of the lane replay's hash set both lie in B,
    ascending, and how many of them the set can hold at once: four per bucket of B and four in the stash."""
    B = sorted(set(int(b) for b in B))
    bk = _buckets_below(int(below))
    return np.flatnonzero(np.isin(bk[:, 0], B) & np.isin(bk[:, 1], B)).astype(np.int64), 4 * len(B) + 4


def perm_onto(rows, labels, n_rows, n=None):
    """A bijection of the rows 0 .. n-1 (n = n_rows unless given) into 0 .. n_rows-1 that sends rows[j] to labels[j]
    and every other row, in order, to the smallest numbers that `labels` leaves unused."""
    rows = np.asarray(rows, dtype=np.int64)
    labels = np.asarray(labels, dtype=np.int64)
    n = int(n_rows if n is None else n)
    assert rows.shape == labels.shape and rows.ndim == 1 and n <= n_rows
    assert len(np.unique(rows)) == len(rows) and len(np.unique(labels)) == len(labels)
    assert (rows >= 0).all() and (rows < n).all() and (labels >= 0).all() and (labels < n_rows).all()
    perm = np.full(n, -1, dtype=np.int64)
    perm[rows] = labels
    rest = np.flatnonzero(perm < 0)
    # the first len(rest) numbers outside `labels`: none of them is beyond len(rest) + len(labels)
    free = np.setdiff1d(np.arange(min(n_rows, len(rest) + len(labels)), dtype=np.int64), labels)[:len(rest)]
    assert len(free) == len(rest)
    perm[rest] = free
    return perm


def clustered(rng, n, d, n_clusters=40, spread=0.5, cent=None):
    """n float32 rows around n_clusters gaussian centres (-> rows, centres: draw the queries with cent=centres)"""
    if cent is None:
        cent = rng.randn(n_clusters, d)
    return (cent[rng.randint(len(cent), size=n)] + spread * rng.randn(n, d)).astype(np.float32), cent


def index_with_centres(metric, X, n_lists, build_probes, seed):
    """A host-built IVF over X whose coarse centres are n_lists distinct rows of X — every centre is then the nearest
    one of its own row, none is inactive, and the index has exactly n_lists lists — with FastPQ(2) fitted on a
    sample and every row in its build_probes nearest lists."""
    from tinyknn_amd import IVF, FastPQ
    rng = np.random.RandomState(seed)
    n = len(X)
    ivf = IVF(metric, n_lists, FastPQ(2))
    rows = X / np.linalg.norm(X, axis=1, keepdims=True) if metric == "angular" else X
    state = np.random.get_state()
    np.random.seed(seed)                    # (the codebook's k-means draws from numpy's global generator)
    try:
        ivf.pq.fit(rows[rng.choice(n, min(n, 4000), replace=False)])
    finally:
        np.random.set_state(state)
    pick = rng.choice(n, n_lists, replace=False)
    assert len(np.unique(rows[pick], axis=0)) == n_lists
    ivf.all_centers = np.ascontiguousarray(rows[pick], dtype=np.float32)
    ivf.build(X, n_probes=build_probes, device=False)
    assert len(ivf.active_centers) == n_lists
    return ivf


def heap_rows(ox, qn, k, n_probes, pass_1=None):
    """the labels in the oracle's final heap of every query of qn: a list of int64 arrays (the -1 of empty slots left out)"""
    out = []
    for q in qn:
        _, dbg = ox.query(q, k, n_probes=n_probes, pass_1=pass_1, debug=True)
        h = dbg["heap_idx"]
        out.append(np.array(h[h >= 0], dtype=np.int64))
    return out


def interleaved(groups, limit):
    """Up to `limit` distinct numbers taken from the arrays of `groups` in turn, one from each per round, so that
    every group gets its share of a short supply."""
    seen, out = set(), []
    for r in range(max(len(g) for g in groups)):
        for g in groups:
            if r < len(g) and int(g[r]) not in seen:
                seen.add(int(g[r]))
                out.append(int(g[r]))
    return np.array(out[:limit], dtype=np.int64)


# ---- the four shapes of tests/test_label_shapes_{cpu,gpu}.py: built once per process, never changed -------------------

_CASES = {}


def _once(key, make):
    if key not in _CASES:
        _CASES[key] = make()
    return _CASES[key]


def _base(metric, n, d, n_lists, build_probes, nq, seed, n_clusters=40):
    rng = np.random.RandomState(seed)
    X, cent = clustered(rng, n, d, n_clusters)
    qs, _ = clustered(rng, nq, d, cent=cent)
    ivf = index_with_centres(metric, X, n_lists, build_probes, seed)
    qn, qp = ivf._prepare(qs.copy())
    return ivf, qn, np.ascontiguousarray(qp)


A_TARGETS, A_K, A_PROBES = 12, 10, 10
# (buckets the colliding labels come from, n_probes, pass_1): heaps of 111; of 149, the hash-set form's largest, over the
# 8 probed lists beside which it still fits the form's LDS rule, and over 10, where it does not (packed kernel); of 21
A_SETTINGS = ((8, 10, None), (8, 8, 149), (8, 10, 149), (4, 10, 21))


def case_a(oracle):
    """A. the hash set over its capacity: 65 536 x 16 rows in 64 lists, every row in two; the labels of the twelve
    target queries' heap rows are renamed into the few labels of 8 (and of 4) buckets.
    -> base index, its oracle, queries, and per bucket count (8, 4): perm, relabelled index, labels, capacity"""
    def make():
        n = 65536
        ivf, qn, qp = _base("euclidean", n, 16, 64, 2, 96, 41)
        ox = oracle_of(oracle, ivf)
        tq = qn[:A_TARGETS]
        out = dict(ivf=ivf, ox=ox, qn=qn, qp=qp)
        # 8 buckets, heaps of 111: rows of the targets' heaps behind the first probed list (many are evicted later)
        # and behind the last (kept to the end), two of the latter for one of the former
        final = heap_rows(ox, tq, A_K, A_PROBES)
        first = heap_rows(ox, tq, A_K, 1, pass_1=(A_PROBES + 1) * A_K + 1)
        groups = []
        for f, e in zip(final, first):
            e = e[~np.isin(e, f)]
            seq = []
            for i in range(len(f)):
                seq.append(f[i])
                if i % 2 == 1 and i // 2 < len(e):
                    seq.append(e[i // 2])
            groups.append(np.array(seq, dtype=np.int64))
        for nb, grp in ((8, groups), (4, heap_rows(ox, tq, A_K, A_PROBES, pass_1=21))):
            labels, cap = labels_in_buckets(range(nb), n)
            rows = interleaved(grp, len(labels))
            perm = perm_onto(rows, labels[:len(rows)], n)
            out[nb] = dict(perm=perm, ivf=relabelled(ivf, perm, n), labels=labels, capacity=cap)
        return out
    return _once("a", make)


B_ROWS = 2 ** 24 + 16
B_TARGETS, B_K, B_PROBES = 12, 10, (10, 20, 40)


def case_b(oracle, which):
    """B. the 24-bit boundary: 40 000 x 8 rows in 40 lists, every row in two, renamed into 2**24 + 16 rows.
    which = 0: the largest label is 0xfffffe (the register heap's label24 entries still apply);
    which = 1: the most wanted row is 0xffffff — the label24 entries' "no row" — and sixteen rows lie above it;
    which = 2: the most wanted row is 0xffffff and no label lies above it: the first index label24 entries cannot serve.
    The top labels go to the rows that most of the twelve targets' final heaps hold.
    -> relabelled index, perm, queries, the top labels in the order they were handed out"""
    def base():
        rng = np.random.RandomState(42)
        X, cent = clustered(rng, 40000, 8)
        qs, _ = clustered(rng, 300, 8, cent=cent)
        # the twelve targets crowd around one row, so that one row is in most of their heaps (300 queries drawn as the
        # rows are share a row of their final heaps seven times at the most)
        qs[:B_TARGETS] = X[rng.randint(len(X))] + (0.05 * rng.randn(B_TARGETS, 8)).astype(np.float32)
        ivf = index_with_centres("euclidean", X, 40, 2, 42)
        qn, qp = ivf._prepare(qs.copy())
        qp = np.ascontiguousarray(qp)
        ox = oracle_of(oracle, ivf)
        final = heap_rows(ox, qn[:B_TARGETS], B_K, B_PROBES[0])
        rows, counts = np.unique(np.concatenate(final), return_counts=True)
        wanted = rows[np.argsort(-counts, kind="stable")][:64]          # most wanted first
        return dict(ivf=ivf, ox=ox, qn=qn, qp=qp, wanted=wanted)
    b = _once("b", base)
    below = np.arange(0xfffffe, 0xfffffe - 64, -1, dtype=np.int64)
    if which == 0:
        top = below
    elif which == 2:
        top = np.concatenate([[0xffffff], below])[:64].astype(np.int64)
    else:
        top = np.concatenate([[0xffffff], np.arange(B_ROWS - 1, 0xffffff, -1), below])[:64].astype(np.int64)
    perm = perm_onto(b["wanted"], top, B_ROWS, n=len(b["ivf"].data))
    return dict(base=b, perm=perm, ivf=relabelled(b["ivf"], perm, B_ROWS), qn=b["qn"], qp=b["qp"], top=top)


C_SETTINGS = ((10, 3), (2, 40), (3, 40))        # (k, n_probes): heaps of 41, 83 and 124 entries


def case_c(oracle, build_probes):
    """C. copies per label: 3 000 x 16 rows in 40 lists, every row in build_probes (9, 17, 18) of them"""
    def make():
        ivf, qn, qp = _base("euclidean", 3000, 16, 40, build_probes, 200, 43 + build_probes)
        return dict(ivf=ivf, ox=oracle_of(oracle, ivf), qn=qn, qp=qp)
    return _once(("c", build_probes), make)


D_K, D_PROBES = 1, (3, 100)


def case_d(oracle, n_lists):
    """D. 70 000 x 16 rows, every row in two of 4 096 / 4 097 lists: the largest list bitmap of the TWIN form, and none"""
    def make():
        ivf, qn, qp = _base("euclidean", 70000, 16, n_lists, 2, 300, 44)
        return dict(ivf=ivf, ox=oracle_of(oracle, ivf), qn=qn, qp=qp)
    return _once(("d", n_lists), make)


def through(perm, idx):
    """perm of an array of row numbers in which -1 means "none" """
    idx = np.asarray(idx)
    return np.where(idx >= 0, np.asarray(perm)[np.maximum(idx, 0)], -1)
