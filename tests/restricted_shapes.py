"""Restricted queries (allowed=, exclude=, group=) on the awkward indexes of tests/test_fuzz_gpu.py, made on the host
without a GPU: case(seed) draws an index shape, a change of its layout and a restriction, builds the index and the CPU
reference's copy of it, and answers with the guarded reference (tests/groups_reference.py::grouped_batch).  Everything
follows from the seed.  tests/test_restricted_shapes_cpu.py asserts that the default seeds hold what they are here for
(wrapped probe lists with the excluded row in the list named twice, short and empty probed lists, answers shorter than
k, ...); tests/test_restricted_fuzz_gpu.py runs the device on the same cases.

Shapes: the ranges of test_fuzz_gpu._case.  Odd seeds are steered towards probe lists that wrap: spread 6.0 (the coarse
heap keeps -1 sentinels, which name the last list — ivf.py:141 — beside the lists found) and n_probes in
{n_lists, n_lists + 3}; they always carry an exclude array, since the pass that has code for a list named twice is
exclude_pass_kernel.  Even seeds walk through the subsets of {allowed, exclude, group} in turn."""
import functools
import os

import numpy as np

from groups_reference import grouped_batch
from store_reference import oracle_index, rounded

DEFAULT_SEEDS = 32
# Where the seeds' random streams start.  Chosen, with the steering below, so that the default seeds hold every
# condition tests/test_restricted_shapes_cpu.py asserts (about a quarter of the steered shapes wrap a probe list).
STREAM = 7200
ABSENT = 2**31 - 2          # the largest group id: no row carries it

ALLOWED_KINDS = ("all", "half", "few", "one", "none", "lists", "not_top1")
EXCLUDE_KINDS = ("nothing", "top1", "random", "twice", "short")
GROUP_KINDS = ("one", "some", "lists", "own")
# the subsets of {allowed, exclude, group} by seed: steered seeds cycle through the four with an exclude array, the
# others through the three without and, every fourth, one of the former
_STEERED_SETS = ("e", "ae", "eg", "aeg")
_OTHER_SETS = ("a", "g", "ag")


def seeds():
    """the seeds of a run: DEFAULT_SEEDS, or TINYKNN_FUZZ_SEEDS as in tests/test_fuzz_gpu.py"""
    return range(int(os.environ.get("TINYKNN_FUZZ_SEEDS", str(DEFAULT_SEEDS))))


def pair_seeds(seeds):
    """The seeds of the pipelined pairs: every third, so that all seven subsets take part (a stride of four meets the
    cycle of subsets below at the same few); from 2, where most partners' answers depend on their own arrays
    (tests/test_restricted_shapes_cpu.py counts them)."""
    return [s for s in seeds if s % 3 == 2]


def shape(seed):
    rng = np.random.RandomState(STREAM + seed)
    steered = seed % 2 == 1
    d = int(rng.choice([3, 8, 17, 20, 33, 100, 130]))
    n_clusters = int(rng.choice([2, 7, 16, 17, 40] if steered else [1, 2, 7, 16, 17, 40]))
    n = int(rng.choice([n_clusters + 1, 60, 333, 1500, 3000]))
    n = max(n, 17 * max(1, n_clusters // 8))       # FastPQ.fit wants >= 16 distinct points
    c = dict(
        d=d, n=n, n_clusters=n_clusters,
        metric=str(rng.choice(["euclidean", "angular"])),
        build_probes=int(min(n_clusters, rng.choice([1, 2, 3] if steered else [1, 1, 2, 3]))),
        k=int(rng.choice([1, 5, 10, 50])),
        n_probes=int(rng.choice([1, 2, 5, n_clusters, n_clusters + 3])),
        nq=int(rng.choice([1, 3, 65, 200])),
        spread=float(rng.choice([0.3, 1.0, 6.0])),
        rotate=bool(rng.rand() < 0.75),
        change=str(rng.choice(["none", "remove", "add"])),
        store=str(rng.choice(["float32", "float32", "float16"])),
        steered=steered,
    )
    if steered:
        c["spread"] = 6.0
        c["n_probes"] = int(rng.choice([n_clusters, n_clusters + 3]))
        c["nq"] = int(rng.choice([3, 65, 200]))
        c["subset"] = _STEERED_SETS[(seed // 2) % 4]
    else:
        i = seed // 2
        c["subset"] = _STEERED_SETS[(i // 4) % 4] if i % 4 == 3 else _OTHER_SETS[(i - i // 4) % 3]
    return c


def probed_lists(probes, n_lists):
    """the lists a row of the reference's probes names: the -1 of an unfilled coarse heap is the last list"""
    p = np.asarray(probes, dtype=np.int64)
    return np.where(p < 0, p + n_lists, p)


def twice(probes, n_lists):
    """the lists one query's probe list names more than once"""
    l, c = np.unique(probed_lists(probes, n_lists), return_counts=True)
    return l[c > 1]


def first_list(ids_per_list, N):
    """the (lowest) list every row is stored in, 0 for a row stored nowhere"""
    first = np.zeros(N, dtype=np.int32)
    for l in reversed(range(len(ids_per_list))):
        first[np.asarray(ids_per_list[l], dtype=np.int64)] = l
    return first


class Case:
    """One case.  shape: the dict of shape(seed); ivf: the host-built index after the layout change, its groups set,
    no device copy; ref_data: the rows the device rescoring reads (float32(float16(data)) for the half store); ox: the reference's
    copy of the index over ref_data; qs: the raw queries, qn, qp: as IVF._prepare makes them; base, base_dbg: the
    unrestricted reference answer; emptied: the list remove() emptied, or None;
    allowed (bool mask or None), exclude (int64 per query or None), groups (int32 per row or None) and group (int32 per
    query or None): the restriction; rows: the stored rows of the query_rows leg (None without an exclude array);
    sizes: rows per list; skipped: why the case could not be built, or None."""
    skipped = None

    def __init__(self, seed):
        self.seed = seed
        self.shape = shape(seed)
        self._want = {}

    def __repr__(self):
        return f"seed {self.seed} {self.shape}"

    # ---- the restriction in the two forms its users need ----
    def device_kwargs(self, aset=None):
        """the keyword arguments of DeviceIndex.query_batch / IVF.query_batch (aset: a prepared AllowSet of the mask)"""
        kw = {}
        if self.allowed is not None:
            kw["allowed"] = self.allowed if aset is None else aset
        if self.exclude is not None:
            kw["exclude"] = self.exclude
        if self.group is not None:
            kw["group"] = self.group
        return kw

    def reference(self, qn=None, sel=slice(None), allowed="own", exclude="own", group="own"):
        """grouped_batch(debug=True) over the queries `sel` with the case's restriction, or with the parts given"""
        from oracle import oracle
        qn = self.qn[sel] if qn is None else qn
        allowed = self.allowed if isinstance(allowed, str) else allowed
        exclude = self.exclude if isinstance(exclude, str) else exclude
        group = self.group if isinstance(group, str) else group
        N = len(self.ref_data)
        return grouped_batch(oracle, self.ox, qn, -1 if group is None else np.asarray(group)[sel],
                             np.zeros(N, np.int32) if self.groups is None else self.groups,
                             self.shape["k"], self.shape["n_probes"],
                             allowed=allowed, exclude=None if exclude is None else exclude[sel], debug=True)

    def want(self):
        """the restricted reference answer (ids, dict(probes, heap_idx, heap_val)): computed once, never changed"""
        if "own" not in self._want:
            self._want["own"] = self.reference()
        return self._want["own"]

    def second(self):
        """The partner call of a coalesced pair.  Two calls join only under one allowed set, grouped both or neither,
        and with room for the second (api_index.hip: coalesce_call): so it has as many rows as the first — the case's
        queries rolled by one, row i of the two calls differs —, the case's allowed set, and arrays of its own: every
        query's unrestricted top-1 excluded (an exclude array whether the case has one or not) and, where the case
        has groups, its query groups rolled by three.
        -> qn_b, qp_b, exclude_b, group_b, reference ids"""
        if "second" not in self._want:
            qn = np.ascontiguousarray(np.roll(self.qn, 1, axis=0))
            qp = np.ascontiguousarray(np.roll(self.qp, 1, axis=0))
            ex = np.ascontiguousarray(np.roll(self.base[:, 0], 1), dtype=np.int64)
            gr = None if self.group is None else np.ascontiguousarray(np.roll(self.group, 3))
            ids, _ = self.reference(qn=qn, exclude=ex, group=gr)
            self._want["second"] = (qn, qp, ex, gr, ids)
        return self._want["second"]


def _index(c, seed):
    """-> (the built index, rows for add(), raw queries, the stream to go on drawing from), or why not (a string)"""
    from tinyknn_amd import IVF, FastPQ
    rng = np.random.RandomState(STREAM + 100000 + seed)
    cent = rng.randn(max(c["n_clusters"], 3), c["d"]) * c["spread"]
    X = (cent[rng.randint(len(cent), size=c["n"])] + 0.5 * rng.randn(c["n"], c["d"])).astype(np.float32)
    qs = (cent[rng.randint(len(cent), size=c["nq"])] + 0.5 * rng.randn(c["nq"], c["d"])).astype(np.float32)
    ivf = IVF(c["metric"], c["n_clusters"], FastPQ(2) if c["rotate"] else FastPQ(2, rotate_dim=None))
    state = np.random.get_state()
    np.random.seed(STREAM + 200000 + seed)      # (both k-means, centres and codebook, draw from the global generator)
    try:
        ivf.fit(X).build(X, n_probes=c["build_probes"], device=False,
                         store="float16" if c["store"] == "float16" else None)
    except AssertionError:
        return "the host build rejects this shape exactly as the reference does"
    finally:
        np.random.set_state(state)
    if len(ivf.active_centers) != c["n_clusters"]:
        return "inactive centres: the reference's grouping asserts on them"
    n_new = int(rng.choice([1, 5, 40]))
    new = (cent[rng.randint(len(cent), size=n_new)] + 0.5 * rng.randn(n_new, c["d"])).astype(np.float32)
    return ivf, new, qs, rng


def _unrestricted(ox, qn, k, n_probes):
    """OracleIndex.query for every row in the form of grouped_batch(debug=True): what grouped_batch gives with no
    restriction (tests/test_restricted_shapes_cpu.py compares the two)"""
    R = (n_probes + 1) * k + 1
    out = np.full((len(qn), k), -1, dtype=np.int64)
    probes = np.zeros((len(qn), min(n_probes, ox.n_lists)), dtype=np.int64)
    hidx = np.zeros((len(qn), R), dtype=np.int64)
    hval = np.zeros((len(qn), R), dtype=np.int32)
    for i, q in enumerate(qn):
        ids, d = ox.query(q, k, n_probes, debug=True)
        out[i, :len(ids)] = ids
        probes[i, :len(d["probes"])] = d["probes"]
        hidx[i], hval[i] = d["heap_idx"], d["heap_val"]
    return out, dict(probes=probes, heap_idx=hidx, heap_val=hval)


def _build(seed):
    from oracle import oracle
    oracle.build()
    case = Case(seed)
    c = case.shape
    made = _index(c, seed)
    if isinstance(made, str):
        case.skipped = made
        return case
    ivf, new, qs, rng = made
    L = c["n_clusters"]
    qn, qp = ivf._prepare(qs.copy())
    qn, qp = np.ascontiguousarray(qn), np.ascontiguousarray(qp)
    k, n_probes = c["k"], c["n_probes"]

    # ---- the layout change (the coarse stage reads the centres alone: the probes stay what they were) ----
    case.emptied = None
    if c["change"] == "remove":
        ox0 = oracle_index(oracle, ivf, ivf.data)
        probed = np.unique(np.concatenate([probed_lists(ox0.query(q, k, n_probes, debug=True)[1]["probes"], L)
                                           for q in qn]))
        case.emptied = int(rng.choice(probed))
        ivf.remove(np.asarray(ivf.ids[case.emptied], dtype=np.int64))
        assert len(ivf.ids[case.emptied]) == 0
    elif c["change"] == "add":
        ivf.add(new)
    N = len(ivf.data)
    case.ivf = ivf
    case.ref_data = rounded(ivf.data) if c["store"] == "float16" else ivf.data
    case.ox = ox = oracle_index(oracle, ivf, case.ref_data)
    case.qs, case.qn, case.qp = qs, qn, qp
    case.sizes = np.array([len(ivf.ids[l]) for l in range(L)], dtype=np.int64)
    case.allowed = case.exclude = case.groups = case.group = case.rows = None
    case.base, case.base_dbg = _unrestricted(ox, qn, k, n_probes)
    probes = case.base_dbg["probes"]
    nq = len(qn)
    stored = np.unique(np.concatenate([np.asarray(ivf.ids[l], dtype=np.int64) for l in range(L)]))
    short = np.flatnonzero((case.sizes > 0) & (case.sizes < 16))
    short_rows = (np.unique(np.concatenate([np.asarray(ivf.ids[l], dtype=np.int64) for l in short]))
                  if len(short) else np.zeros(0, np.int64))
    top1 = case.base[:, 0]

    # ---- the restriction ----
    sub = c["subset"]
    if "a" in sub:
        kind = case.allowed_kind = ALLOWED_KINDS[rng.randint(len(ALLOWED_KINDS))]
        m = np.zeros(N, dtype=bool)
        if kind == "all":
            m[:] = True
        elif kind == "half":
            m = rng.rand(N) < 0.5
        elif kind == "few":
            m = rng.rand(N) < 0.05
        elif kind == "one":
            m[rng.choice(stored) if len(stored) else 0] = True
        elif kind == "lists":
            for l in rng.choice(L, max(1, L // 3), replace=False):
                m[np.asarray(ivf.ids[l], dtype=np.int64)] = True
        elif kind == "not_top1":
            m[:] = True
            m[top1[top1 >= 0]] = False
        case.allowed = m
    if "e" in sub:
        ex = np.full(nq, -1, dtype=np.int64)
        kinds = []
        for i in range(nq):
            tw = twice(probes[i], L)
            tw = tw[case.sizes[tw] > 0]
            # (a query whose probe list wraps takes a row of the list named twice half of the time)
            kind = "twice" if len(tw) and rng.rand() < 0.5 else EXCLUDE_KINDS[rng.randint(len(EXCLUDE_KINDS))]
            if kind == "top1":
                ex[i] = top1[i]
            elif kind == "random":
                ex[i] = rng.randint(N)
            elif kind == "twice" and len(tw):
                ex[i] = rng.choice(np.asarray(ivf.ids[int(rng.choice(tw))], dtype=np.int64))
            elif kind == "short" and len(short_rows):
                ex[i] = rng.choice(short_rows)
            kinds.append(kind if ex[i] >= 0 else "nothing")      # (a kind counts where it named a row)
        case.exclude, case.exclude_kinds = ex, kinds
        # the stored rows of the query_rows leg: with duplicates, from the short lists, the excluded rows among them
        rows = rng.randint(N, size=nq).astype(np.int64)
        rows[ex >= 0] = ex[ex >= 0]
        if len(short_rows):
            at = rng.choice(nq, max(1, nq // 4), replace=False)
            rows[at] = rng.choice(short_rows, len(at))
        rows[-1] = rows[0]
        case.rows = rows
    if "g" in sub:
        kind = case.group_kind = GROUP_KINDS[rng.randint(len(GROUP_KINDS))]
        if kind == "one":
            groups = np.full(N, 5, dtype=np.int32)
        elif kind == "some":
            groups = rng.randint(0, 7, N).astype(np.int32)
        elif kind == "lists":
            groups = first_list([ivf.ids[l] for l in range(L)], N)
        else:
            groups = np.arange(N, dtype=np.int32)
        group = rng.choice(np.unique(groups), nq).astype(np.int32)
        group[rng.rand(nq) < 0.2] = -1
        group[rng.rand(nq) < 0.1] = ABSENT
        case.groups, case.group = groups, group
        ivf.set_groups(groups)          # (the host copy: a device index made from this IVF is given them)
    return case


@functools.lru_cache(maxsize=None)
def case(seed):
    """The case of a seed: built once per process and shared; its users change nothing in it (a device index is made
    from case.ivf, not kept on it)."""
    return _build(int(seed))


# ---- what a case holds: the coverage conditions of tests/test_restricted_shapes_cpu.py ----

def facts(case, answers=True):
    """dict of booleans and counts over one case (answers: the restricted and unrestricted reference answers compared
    as well, which computes the restricted one)"""
    c, L = case.shape, case.shape["n_clusters"]
    probes = case.base_dbg["probes"]
    lists = [probed_lists(p, L) for p in probes]
    tw = [twice(p, L) for p in probes]
    in_twice = False
    if case.exclude is not None:
        for i, e in enumerate(case.exclude):
            in_twice |= any(e >= 0 and e in np.asarray(case.ivf.ids[l]) for l in tw[i])
    probed = np.unique(np.concatenate(lists)) if len(lists) else np.zeros(0, np.int64)
    out = dict(
        wraps=any(len(t) for t in tw),
        excluded_in_twice=bool(in_twice),
        build_probes=c["build_probes"],
        probes_short=bool(((case.sizes[probed] > 0) & (case.sizes[probed] < 16)).any()),
        probes_empty=bool((case.sizes[probed] == 0).any()),
        more_probes_than_lists=c["n_probes"] > L,
        single=L == 1 or len(case.qn) == 1,
    )
    if answers:
        want, _ = case.want()
        n_got = (want != -1).sum(axis=1)
        n_base = (case.base != -1).sum(axis=1)
        out.update(fewer_than_k=bool((n_got < c["k"]).any()), none=bool((n_got == 0).any()),
                   differs_same_length=bool(((n_got == n_base) & (want != case.base).any(axis=1)).any()))
    return out
