"""The default cases of per_group=, made on the host without a GPU: the golden fixtures under four group
assignments and a small synthetic index that holds some rows twice.  tests/test_per_group_cpu.py asserts, from the CPU
reference alone, that these cases hold what they are here for (capped answers that differ from the uncapped ones, rows
that end in -1, heaps of at most k ids, candidates at equal distances); tests/test_per_group_gpu.py runs the device on
the same cases.  A case's heaps do not depend on its groups or caps, so the guarded reference runs once per (index,
n_probes, restriction) and the cases walk its rankings (per_group_reference.capped_from_heaps)."""
import functools

import numpy as np

from conftest import G6_TAGS, golden
from per_group_reference import capped_from_heaps, heaps_of
from store_reference import fixture_ivf, oracle_index

# heaps of (5 + 1) * 10 + 1 = 61 entries: the staged kernels, one 64-rank chunk.  (The pass_1 = 300 legs of the GPU file
# take the lane-per-row kernel under every form; larger staged heaps are tests/per_group_edge_shapes.py's.)
K, N_PROBES = 10, 5
ASSIGNMENTS = ("mod3", "oct", "one", "own")
CAPS = (1, 2, K, "mix")                 # "mix": a per-query array of 0, 1 and 3

SYN_N, SYN_D, SYN_NQ, SYN_LISTS = 2000, 20, 32, 20
# groups of the synthetic index: id % 8, so that a cap of 1 leaves at most 8 ids and every such row ends in -1.
# Rows [1000, 1020) repeat rows [0, 20): the same group (1000 % 8 == 0); rows [1020, 1040) repeat rows [27, 47):
# another group (1020 % 8 != 27 % 8)
SYN_TWINS = ((1000, 0, 20), (1020, 27, 20))


def assignment(name, N):
    ids = np.arange(N, dtype=np.int64)
    return {"mod3": ids % 3, "oct": ids // 8, "one": np.full(N, 5), "own": ids}[name].astype(np.int32)


def caps(m, nq):
    """the per_group= argument of a case: an int, or the per-query mix"""
    return np.tile(np.array([0, 1, 3], dtype=np.int32), nq // 3 + 1)[:nq] if m == "mix" else int(m)


@functools.lru_cache(maxsize=None)
def fixture(tag):
    """-> (IVF without a device copy, the reference's copy, qn, qp)"""
    from oracle import oracle
    oracle.build()
    g = golden(f"g6_ivf_{tag}.npz")
    ivf = fixture_ivf(g)
    return ivf, oracle_index(oracle, ivf, g["data"]), g["qn"], g["qpq"]


@functools.lru_cache(maxsize=None)
def synthetic():
    """-> (IVF built on the host, the reference's copy, qn, qp, groups): clustered rows, two runs of them stored twice
    under other ids, half of the queries right beside a repeated row"""
    from oracle import oracle
    from tinyknn_amd import IVF, FastPQ
    oracle.build()
    rng = np.random.RandomState(4151)
    cent = rng.randn(SYN_LISTS, SYN_D) * 2.0
    X = (cent[rng.randint(SYN_LISTS, size=SYN_N)] + 0.5 * rng.randn(SYN_N, SYN_D)).astype(np.float32)
    for at, src, n in SYN_TWINS:
        X[at:at + n] = X[src:src + n]
    near = np.concatenate([np.arange(0, 8), np.arange(27, 35)])
    qs = np.concatenate([X[near] + 0.02 * rng.randn(len(near), SYN_D),
                         cent[rng.randint(SYN_LISTS, size=SYN_NQ - len(near))] + 0.5 * rng.randn(SYN_NQ - len(near), SYN_D)])
    qs = qs.astype(np.float32)
    ivf = IVF("euclidean", SYN_LISTS, FastPQ(2, rotate_dim=None))        # unrotated: the reference is fed qn
    state = np.random.get_state()
    np.random.seed(4152)                # (both k-means draw from the global generator)
    try:
        ivf.fit(X).build(X, n_probes=1, device=False)
    finally:
        np.random.set_state(state)
    qn, qp = ivf._prepare(qs.copy())
    groups = (np.arange(SYN_N) % 8).astype(np.int32)
    return ivf, oracle_index(oracle, ivf, ivf.data), np.ascontiguousarray(qn), np.ascontiguousarray(qp), groups


def synthetic_few():
    """the allowed mask of the short-heap cases: a handful of rows, about one per list"""
    return np.arange(SYN_N) % 97 == 0


@functools.lru_cache(maxsize=None)
def heaps(index, n_probes, few=False):
    """heap_idx of the guarded reference for a fixture tag or "syn", computed once, never changed"""
    from oracle import oracle
    ox, qn = (synthetic() if index == "syn" else fixture(index))[1:3]
    h = heaps_of(oracle, ox, qn, K, n_probes, allowed=synthetic_few() if few else None)
    h.setflags(write=False)
    return h


def default_cases():
    """(index, assignment or "syn8", cap, n_probes, few) of every default case"""
    out = [(tag, a, m, N_PROBES, False) for tag in G6_TAGS for a in ASSIGNMENTS for m in CAPS]
    out += [("syn", "syn8", m, N_PROBES, False) for m in CAPS]             # equal distances
    out += [("syn", "syn8", m, 1, True) for m in (1, 2)]                   # short and empty heaps
    return out


def case_inputs(case):
    """-> (ox, qn, groups, per_group argument, heaps) of a default case"""
    index, a, m, n_probes, few = case
    if index == "syn":
        _, ox, qn, _, groups = synthetic()
    else:
        _, ox, qn, _ = fixture(index)
        groups = assignment(a, len(ox.data))
    return ox, qn, groups, caps(m, len(qn)), heaps(index, n_probes, few)


def reference(case, full=False):
    """capped_from_heaps of a default case: (ids, distances, counts[, rankings])"""
    from oracle import oracle
    ox, qn, groups, m, h = case_inputs(case)
    return capped_from_heaps(oracle, ox, qn, h, m, groups, K, full=full)
