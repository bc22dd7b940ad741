"""per_group= where the capped walk leaves its first 64 ranks, made on the host without a GPU: small
indexes, group assignments that push the kept rows to late ranks, and a grid of heap sizes R (pass_1 sets R directly)
and k around the edges of cap_select.h's 64-rank chunks and of the staged kernel's rankings (strict_counts<1|2|4> at
nc <= 64 / <= 128 / else).  tests/test_per_group_edges_cpu.py asserts, from the CPU reference alone, that the grid holds
what it is here for; tests/test_per_group_edges_gpu.py runs the device on it.  Everything follows from fixed seeds.

A case's heaps depend on neither its groups nor its caps: the guarded reference runs once per (index, k, R) and the
legs walk its rankings (per_group_reference.capped_from_heaps), as in tests/per_group_shapes.py."""
import functools

import numpy as np

import per_group_shapes as base
from per_group_reference import capped_from_heaps, heaps_of
from restricted_shapes import first_list
from store_reference import oracle_index, rounded

N, NQ, LISTS, N_PROBES = base.SYN_N, base.SYN_NQ, base.SYN_LISTS, base.N_PROBES

# name -> (d, the dtype of the vectors, store): "twins" is per_group_shapes.synthetic() as it is (rows stored twice:
# equal distances, the positional tie walk); the others are its recipe without the repeated rows (no two candidates of
# a query at one distance: the strict-count ranking of the staged body)
INDEXES = {
    "twins": (base.SYN_D, np.float32, None),
    "distinct": (100, np.float32, None),
    "distinct16": (100, np.float32, "float16"),
    "wide": (256, np.float32, None),
    "odd17": (17, np.float32, None),
    "odd130": (130, np.float32, None),
    "f64": (20, np.float64, None),
}
ODD = ("odd17", "odd130")
NO_TIES = ("distinct", "distinct16", "wide") + ODD
# where each index's random stream starts: chosen so that no ranking of a NO_TIES index holds two equal distances at any
# R of the grid (by chance about one float32 index in ten has such a pair; tests/test_per_group_edges_cpu.py asserts it)
_SEED = {"distinct": 4200, "distinct16": 4210, "wide": 4221, "odd17": 4230, "odd130": 4240, "f64": 4250}

R_GRID = (63, 64, 65, 127, 128, 129, 192, 193, 255, 256, 257)
K_GRID = (1, 10, 63, 64, 65, 100)
THIN_R = (65, 128, 129, 256, 257)       # the grid of every index but "twins"
THIN_K = (1, 10, 64, 65)
# (assignment, m); "mix": the per-query array of 0, 1 and 3 of per_group_shapes.caps
LEGS = (("mod3", 1), ("lists", 2), ("near5", 1), ("near5", 3), ("oct", 1), ("mod3", "mix"), ("near2", 1))
FORMS = (0, 1, 2)
# the largest heap a capped call admits (largest_admitted_heap), on "twins" and "f64": every list probed, group kind
# "lists" with m = 1 — a query's ten nearest lists, one row each, the walk far beyond the first chunks
LARGEST_K, LARGEST_PROBES = 10, 20
LARGEST_LEGS = (("lists", 1), ("mod3", 1))      # (mod3: three kept rows, every chunk of the heap walked)


def grid(index):
    """(R, k) of an index's legs: k < R"""
    rs, ks = (R_GRID, K_GRID) if index == "twins" else (THIN_R, THIN_K)
    return [(R, k) for R in rs for k in ks if k < R]


def ks_of(index, R):
    return [k for r, k in grid(index) if r == R]


@functools.lru_cache(maxsize=None)
def index(name):
    """-> (IVF built on the host, the reference's copy, qn, qp): per_group_shapes.synthetic() for "twins", else its
    recipe at the index's d, dtype and store, no row repeated"""
    if name == "twins":
        return base.synthetic()[:4]
    from oracle import oracle
    from tinyknn_amd import IVF, FastPQ
    oracle.build()
    d, dtype, store = INDEXES[name]
    rng = np.random.RandomState(_SEED[name])
    cent = rng.randn(LISTS, d) * 2.0
    X = (cent[rng.randint(LISTS, size=N)] + 0.5 * rng.randn(N, d)).astype(dtype)
    near = np.arange(16)
    qs = np.concatenate([X[near] + 0.02 * rng.randn(len(near), d),
                         cent[rng.randint(LISTS, size=NQ - len(near))] + 0.5 * rng.randn(NQ - len(near), d)])
    qs = qs.astype(np.float32)
    ivf = IVF("euclidean", LISTS, FastPQ(2, rotate_dim=None))        # unrotated: the reference is fed qn
    state = np.random.get_state()
    np.random.seed(_SEED[name] + 1)     # (both k-means draw from the global generator)
    try:
        ivf.fit(X).build(X, n_probes=1, device=False, store=store)
    finally:
        np.random.set_state(state)
    assert ivf.data.dtype == dtype
    qn, qp = ivf._prepare(qs.copy())
    # the half store's rescoring reads float32(float16(data)): so does its reference
    ox = oracle_index(oracle, ivf, rounded(ivf.data) if store == "float16" else ivf.data)
    return ivf, ox, np.ascontiguousarray(qn), np.ascontiguousarray(qp)


@functools.lru_cache(maxsize=None)
def groups(name, a):
    """the group of every row under assignment `a`: mod3, oct (id // 8), own, lists (the list a row is stored in),
    near5 (its list where id % 5 != 0, else a group of its own), near2 (the same with id % 2).  The last three put
    runs of one group at the front of a ranking: the kept rows come from late ranks.  Under near2 with m = 1 a walk
    that does not fill k ends on the heap's last rank whenever that row's id is even: about half of the queries, also
    where that rank is the only one of its chunk (R = 65, 129, 193, 257: lane 0 alone holds a rank)."""
    ivf = index(name)[0]
    ids = np.arange(N, dtype=np.int64)
    L = len(ivf.active_centers)
    if a in ("lists", "near5", "near2"):
        g = first_list([ivf.ids[l] for l in range(L)], N).astype(np.int64)
        if a != "lists":
            g = np.where(ids % (5 if a == "near5" else 2) != 0, g, L + ids)
    else:
        g = {"mod3": ids % 3, "oct": ids // 8, "own": ids}[a]
    g = g.astype(np.int32)
    g.setflags(write=False)
    return g


def caps(m):
    return base.caps(m, NQ)


@functools.lru_cache(maxsize=None)
def heaps(name, k, R, n_probes=N_PROBES):
    """heap_idx (NQ, R) of the guarded reference, computed once per (index, k, R), never changed"""
    from oracle import oracle
    _, ox, qn, _ = index(name)
    h = heaps_of(oracle, ox, qn, k, n_probes, pass_1=R)
    assert h.shape == (NQ, R), h.shape
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def reference(name, R, k, a, m, n_probes=N_PROBES):
    """capped_from_heaps of a leg: (ids, distances, counts, rankings); computed once, never changed"""
    from oracle import oracle
    _, ox, qn, _ = index(name)
    out = capped_from_heaps(oracle, ox, qn, heaps(name, k, R, n_probes), caps(m), groups(name, a), k, full=True)
    for x in out[:3]:
        x.setflags(write=False)
    return out


def last_kept_ranks(ref):
    """per query, the rank of its last returned id within its full ranking (-1 where nothing is returned)"""
    ids, _, counts, ranked = ref
    out = np.full(len(ids), -1, dtype=np.int64)
    for i, (c, _) in enumerate(ranked):
        if counts[i]:
            out[i] = _rank_of_last(c, ids[i], counts[i])
    return out


def _rank_of_last(c, row, n):
    """the kept ids are a subsequence of the ranking c (an id may stand in it once only: one list per row): walk it"""
    at = -1
    for x in row[:n]:
        at = at + 1 + int(np.flatnonzero(c[at + 1:] == x)[0])
    return at


# ---- which kernel a shape takes: a LABEL for the census, not a reference ---------------------------------------------
# rescore.hip, launch_float_sums: float32 sums (float32 and half rows) are staged through an LDS tile of 32 (form 2,
# the default) or 64 (form 1) rows where d % 4 == 0, d <= 256, R <= 256 and the LDS total — ids and row offsets (16 R),
# distances and query (4 bytes each, rounded up to 4 entries), the tile of tile_rows + 1 rows of (d / 4) | 1 pieces (16
# bytes of float32, 8 of half) rounded up to 16 bytes, and the capped ranking (cap_select.h: 16 R) — is at most 64 KiB;
# else, and under form 0 and for float64 vectors (tk_launch_rescore), every lane walks its own row.

def staged(name, R, form):
    d, dtype, store = INDEXES[name]
    if dtype == np.float64 or form not in (1, 2) or d % 4 or d > 256 or R > 256:
        return False
    piece = 8 if store == "float16" else 16
    tile = ((32 if form == 2 else 64) + 1) * ((d // 4) | 1) * piece
    lds = R * 16 + (((R + 3) & ~3) + ((d + 3) & ~3)) * 4 + ((tile + 15) & ~15) + R * 16
    return lds <= 64 * 1024


def largest_admitted_heap(d, dist_size):
    """the largest R of a capped call (api_index.hip, the `per_group:` ARGCHECK):
    R * (8 + dsz) + d * dsz + 32 + cap_lds_bytes(R, dsz) <= 64 KiB, cap_lds_bytes = R * (8 + dsz + 4)"""
    return (64 * 1024 - 32 - d * dist_size) // ((8 + dist_size) + (8 + dist_size + 4))


# ---- the fuzz cases: the awkward indexes of tests/restricted_shapes.py, each with groups and caps drawn on top --------

FUZZ_DEFAULT_SEEDS = 16
# where the caps' own random streams start: chosen so that the 32 default cases of restricted_shapes hold what
# tests/test_per_group_edges_cpu.py asserts
FUZZ_STREAM = 6300
FUZZ_GROUP_KINDS = ("mod3", "pairs", "lists", "oct", "one", "mod7")
FUZZ_CAPS = (0, 1, 1, 2, 3)
_fuzz = {}


def fuzz_seeds():
    """the seeds of a run: FUZZ_DEFAULT_SEEDS, or TINYKNN_FUZZ_SEEDS as in the other fuzz files"""
    import os
    return range(int(os.environ.get("TINYKNN_FUZZ_SEEDS", str(FUZZ_DEFAULT_SEEDS))))


class CapCase:
    """case: the restricted_shapes.Case (unchanged, shared); groups (int32 per row of its index after the layout
    change): the case's own where it has them, else one of FUZZ_GROUP_KINDS cycled by seed; group_kind; caps (int32
    per query, drawn from FUZZ_CAPS on the seed's own stream)"""

    def __init__(self, seed):
        import restricted_shapes as rs
        self.seed = seed
        self.case = case = rs.case(seed)
        self.skipped = case.skipped
        if self.skipped is not None:
            return
        rng = np.random.RandomState(FUZZ_STREAM + seed)
        n_rows, nq, L = len(case.ref_data), len(case.qn), case.shape["n_clusters"]
        ids = np.arange(n_rows, dtype=np.int64)
        if case.groups is not None:
            self.group_kind, g = "case", case.groups
        else:
            self.group_kind = kind = FUZZ_GROUP_KINDS[seed % len(FUZZ_GROUP_KINDS)]
            g = (first_list([case.ivf.ids[l] for l in range(L)], n_rows) if kind == "lists" else
                 {"mod3": ids % 3, "pairs": ids // 2, "oct": ids // 8, "one": np.full(n_rows, 5), "mod7": ids % 7}[kind])
        self.groups = np.ascontiguousarray(g, dtype=np.int32)
        self.caps = np.array(FUZZ_CAPS, dtype=np.int32)[rng.randint(len(FUZZ_CAPS), size=nq)]
        self.R = (case.shape["n_probes"] + 1) * case.shape["k"] + 1

    def __repr__(self):
        return f"per_group seed {self.seed} groups {self.group_kind} on {self.case}"

    def from_heaps(self, qn, heap_idx, caps=None, full=False):
        from oracle import oracle
        return capped_from_heaps(oracle, self.case.ox, qn, heap_idx, self.caps if caps is None else caps, self.groups,
                                 self.case.shape["k"], full=full)

    def want(self):
        """(ids, distances, counts, rankings) under the case's own restriction and the caps: computed once"""
        if "_want" not in self.__dict__:
            self.__dict__["_want"] = self.from_heaps(self.case.qn, self.case.want()[1]["heap_idx"], full=True)
        return self.__dict__["_want"]

    def uncapped(self):
        return self.from_heaps(self.case.qn, self.case.want()[1]["heap_idx"], caps=0)

    def second(self):
        """the partner call of a coalesced pair (Case.second) under caps of its own, this case's rolled by one
        -> qn_b, qp_b, exclude_b, group_b, caps_b, (ids, distances, counts)"""
        if "_second" not in self.__dict__:
            qn, qp, ex, gr, ids = self.case.second()
            got, dbg = self.case.reference(qn=qn, exclude=ex, group=gr)
            assert np.array_equal(got, ids)
            caps_b = np.ascontiguousarray(np.roll(self.caps, 1))
            self.__dict__["_second"] = (qn, qp, ex, gr, caps_b, self.from_heaps(qn, dbg["heap_idx"], caps=caps_b))
        return self.__dict__["_second"]


def fuzz_case(seed):
    if seed not in _fuzz:
        _fuzz[seed] = CapCase(int(seed))
    return _fuzz[seed]
