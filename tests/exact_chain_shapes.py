"""The chains of tests/list_chain_shapes.py with what the exact and restricted calls read beside the lists: a group id,
a tag mask and a value per row, carried through every IVF.add / remove / update; one chain steered at an index that
IVF.remove leaves too sparse for a twin table (thinned); and four chains on integer coordinates, where numpy gives the
`part` of knn_brute and radius_brute bit for bit.  No GPU: tests/test_exact_chain_cpu.py holds the attribute arrays
against the library's host copies and asserts what the default seeds cover; tests/test_exact_chain_gpu.py runs the
device.  list_chain_shapes.py is imported, never changed: ListsModel knows nothing of tags and values, the arrays live
beside it (Attrs).

Attributes: groups for EVERY seed (the chain's own where shape["groups"], else drawn here, ids 0 .. 4), uint64 tag
masks of 8 bits with about one row in eight carrying no tag at all (mask 0), int64 values in [0, 100).  The rows of an
add or update step get new ones drawn from (seed, step)."""
import functools

import numpy as np

import list_chain_shapes as lc

# Where the attribute streams start.  With ATTRS = 700000, the first start tried, the default seeds hold every condition
# that tests/test_exact_chain_cpu.py::test_default_seeds_cover_what_the_exact_calls_need asserts (it prints its counts).
ATTRS = 700000
N_GROUPS = 5
INT_SEEDS = (0, 1, 2, 3)
THINNED = (2, 3)


def _rng(seed, step):
    """the stream of (seed, step); step -1: the rows the index was built over"""
    return np.random.RandomState(lc.STREAM + ATTRS + 1000 * int(seed) + step + 1)


def draw_attrs(rng, n, groups=None):
    """n rows' attributes: dict(groups int32 — the ones given, else drawn —, tags uint64, values int64)"""
    g = rng.randint(0, N_GROUPS, size=n).astype(np.int32)
    tags = rng.randint(1, 256, size=n).astype(np.uint64)
    tags[rng.rand(n) < 0.125] = 0
    values = rng.randint(0, 100, size=n).astype(np.int64)
    return dict(groups=g if groups is None else np.asarray(groups, np.int32), tags=tags, values=values)


class Attrs:
    """The attribute arrays by row id that the references read: groups (N,) int32, tags (N,) uint64, values (N,)
    int64.  add appends, update overwrites, remove changes nothing (the library keeps a removed row's attributes)."""

    def __init__(self, groups, tags, values):
        self.groups, self.tags, self.values = groups.copy(), tags.copy(), values.copy()

    def apply(self, op, new):
        if op["kind"] == "add":
            for name in ("groups", "tags", "values"):
                setattr(self, name, np.concatenate([getattr(self, name), new[name]]))
        elif op["kind"] == "update":
            for name in ("groups", "tags", "values"):
                a = getattr(self, name).copy()
                a[op["ids"]] = new[name]
                setattr(self, name, a)
        return self


def initial_attrs(case):
    """the attributes of the rows the case's index was built over"""
    return Attrs(**draw_attrs(_rng(case.seed, -1), case.N0, case.ivf.groups))


def step_attrs(case, step):
    """the new attributes of the rows of step `step` (None for a removal)"""
    op = case.ops[step]
    if op["kind"] == "remove":
        return None
    return draw_attrs(_rng(case.seed, step), len(op["X"]), op["groups"])


def fresh(case):
    """(a copy of the case's index with the three attributes set, their arrays)"""
    ivf, attrs = case.fresh_ivf(), initial_attrs(case)
    ivf.set_groups(attrs.groups)
    ivf.set_tags(attrs.tags)
    ivf.set_values(attrs.values)
    return ivf, attrs


def apply(ivf, op, new, attrs):
    """the change `op` through the library with its rows' attributes `new`, and the same on the arrays"""
    if op["kind"] == "add":
        out = ivf.add(op["X"], groups=new["groups"], tags=new["tags"], values=new["values"])
    elif op["kind"] == "remove":
        out = ivf.remove(op["ids"])
    else:
        out = ivf.update(op["ids"], op["X"], groups=new["groups"], tags=new["tags"], values=new["values"])
    attrs.apply(op, new)
    return out


def replay(case):
    """(step, op, the model after it, the attribute arrays after it, the groups before it) from the model alone"""
    m, attrs = case.model(), initial_attrs(case)
    for i, op in enumerate(case.ops):
        before = attrs.groups
        m.apply(op)
        attrs.apply(op, step_attrs(case, i))
        yield i, op, m, attrs, before


def stored_mask(m):
    out = np.zeros(m.N, dtype=bool)
    out[m.stored_ids()] = True
    return out


def ref_ivf(case, m):
    """the IVF a fresh upload and the oracle take for the model's state (test_list_chain_gpu._host_chain's ref_of)"""
    from test_update_gpu import _ref_ivf
    built_L = len(case.ivf.active_centers)
    return _ref_ivf(case.ivf, (m.ids, m.labels), m.data, m.zero, L1=m.L if m.L > built_L else None)


def deep_steps(n):
    """the two steps with the full set of checks (test_list_chain_gpu._deep_steps)"""
    return {n // 2 - 1 if n >= 2 else 0, n - 1}


# ---- the restrictions of a state, drawn from (seed, step) --------------------------------------------------------------

def restrictions(case, step, m, attrs, nq):
    """The restriction arguments asked at one state: dict name -> (keywords of the device call, keywords of
    brute_restricted_reference.passes).  Drawn from (seed, step) over the state's N rows: an allowed mask of about
    half the rows; an excluded stored row for three queries in four; a group for most queries (query 0 always has
    one); tag masks of 1-3 bits, 0 for some queries; ranges of width 45 over the values."""
    rng = np.random.RandomState(lc.STREAM + ATTRS + 500000 + 1000 * int(case.seed) + step)
    N = m.N
    stored = m.stored_ids()
    mask = rng.rand(N) < 0.5
    exclude = (rng.choice(stored, nq) if len(stored) else np.full(nq, -1)).astype(np.int64)
    exclude[3::4] = -1
    group = rng.randint(-1, N_GROUPS, size=nq).astype(np.int32)
    group[0] = rng.randint(0, N_GROUPS)
    tags = (1 << rng.randint(0, 8, size=nq)).astype(np.uint64) | (1 << rng.randint(0, 8, size=nq)).astype(np.uint64)
    tags[2::5] = 0
    lo = rng.randint(0, 60, size=nq).astype(np.int64)
    between = (lo, lo + 45)
    g = dict(group=group, groups=attrs.groups)
    t_any = dict(tags=tags, tags_mode="any", row_tags=attrs.tags)
    t_all = dict(tags=tags, tags_mode="all", row_tags=attrs.tags)
    b = dict(between=between, values=attrs.values)
    wide = np.full(nq, 0b11111111, dtype=np.uint64)
    wide[::3] = tags[::3]
    loose = rng.rand(N) < 0.8
    return {
        "allowed": (dict(allowed=mask), dict(allowed=mask)),
        "exclude": (dict(exclude=exclude), dict(exclude=exclude)),
        "group": (dict(group=group), g),
        "tags any": (dict(tags=tags, tags_mode="any"), t_any),
        "tags all": (dict(tags=tags, tags_mode="all"), t_all),
        "between": (dict(between=between), b),
        "all five": (dict(allowed=loose, exclude=exclude, group=group, tags=wide, tags_mode="any",
                          between=(np.zeros(nq, np.int64), np.full(nq, 80, np.int64))),
                     dict(allowed=loose, exclude=exclude, group=group, groups=attrs.groups, tags=wide, tags_mode="any",
                          row_tags=attrs.tags, between=(np.zeros(nq, np.int64), np.full(nq, 80, np.int64)),
                          values=attrs.values)),
    }


def knn_groups(rs):
    """the group ids knn_group is asked with at a state: restrictions()' group, a drawn id in place of every -1 (the
    call refuses "any group")"""
    g = rs["group"][0]["group"].copy()
    free = np.flatnonzero(g < 0)
    g[free] = free % N_GROUPS
    return g


# ---- b. the steered case: an index IVF.remove leaves too sparse for the index's own twin table -------------------------

class _Made(lc.Case):
    """a Case whose shape is given, not drawn"""

    def __init__(self, seed, shape):
        self.seed, self.shape = seed, shape


def _finish(case, ivf, cent, qs):
    case.ivf, case.cent, case.left_out, case.N0, case.qs = ivf, cent, None, len(ivf.data), qs
    qn, qp = ivf._prepare(qs.copy())
    case.qn, case.qp = np.ascontiguousarray(qn), np.ascontiguousarray(qp)
    case.ops = []
    return case


def _op(case, m, kind, sel, ids=None, X=None):
    op = dict(kind=kind, sel=sel, ids=ids, X=X, new=None, near=None, labels=None, groups=None)
    if X is not None:
        op["new"], op["near"], op["labels"] = lc.prepared(case.ivf, X, m.kp)
    case.ops.append(op)
    m.apply(op)


THIN_N, THIN_KEPT = 3000, 100


@functools.lru_cache(maxsize=None)
def thinned(kp):
    """Euclidean, d = 8, 16 lists, 3000 rows each stored in its kp nearest lists; the chain: (0) remove every row but
    100, row N - 1 among the survivors; (1) add 5 rows; (2) update 10 of the survivors.  After step 0 the lists hold
    T = 100 kp entries under the largest label 2999: for kp = 2 that is beyond the 8 T + 1024 labels up to which
    install_lists makes the index's own twin table (api_index.hip: build_twins), so radius_search(n_probes=) has to
    make its own; for kp = 3 (8 * 300 + 1024 = 3424) the index still makes one, of width 2, from nearly empty lists.
    tests/test_exact_chain_cpu.py::test_thinned asserts both."""
    from tinyknn_amd import IVF, FastPQ
    seed = 900 + kp
    rng = np.random.RandomState(lc.STREAM + ATTRS + 600000 + kp)
    d, L, nq = 8, 16, 33
    shape = dict(d=d, n=THIN_N, n_clusters=L, metric="euclidean", build_probes=kp, k=10, n_probes=5, nq=nq, store="float32",
                 groups=False, steered=True)
    cent = rng.randn(L, d) * 3.0
    X = (cent[rng.randint(L, size=THIN_N)] + 0.5 * rng.randn(THIN_N, d)).astype(np.float32)
    qs = (cent[rng.randint(L, size=nq)] + 0.5 * rng.randn(nq, d)).astype(np.float32)
    ivf = IVF("euclidean", L, FastPQ(2, rotate_dim=None))
    state = np.random.get_state()
    np.random.seed(lc.STREAM + ATTRS + 610000 + kp)
    try:
        ivf.fit(X).build(X, n_probes=kp, device=False)
    finally:
        np.random.set_state(state)
    assert len(ivf.active_centers) == L
    case = _finish(_Made(seed, shape), ivf, cent, qs)
    m = case.model()
    kept = np.concatenate([rng.choice(THIN_N - 1, THIN_KEPT - 1, replace=False), [THIN_N - 1]])
    _op(case, m, "remove", "all but 100", ids=np.setdiff1d(np.arange(THIN_N), kept).astype(np.int64))
    _op(case, m, "add", "n=5", X=case.rows_near(rng, 5))
    ids = np.sort(rng.choice(kept, 10, replace=False)).astype(np.int64)
    _op(case, m, "update", "survivors", ids=ids, X=case.rows_near(rng, 10))
    return case


def twin_table_of(m):
    """(T, largest label + 1, copies of the most stored label, does install_lists make the index's own twin table)
    for the model's lists, by the rule of api_index.hip: build_twins"""
    ids = np.concatenate(m.ids) if m.L else np.zeros(0, np.int64)
    T = len(ids)
    if T == 0:
        return 0, 0, 0, False
    copies = int(np.bincount(ids).max())
    bound = int(ids.max()) + 1
    return T, bound, copies, 2 <= copies <= 17 and bound <= 8 * T + 1024


# ---- c. integer coordinates: the `part` of knn_brute / radius_brute is reproduced bit for bit -------------------------

INT_SHAPES = {      # seed: (d, build_probes, lists, rows, queries)
    0: (3, 1, 7, 333, 24),
    1: (33, 2, 16, 1500, 33),
    2: (128, 2, 2, 60, 3),
    3: (33, 1, 1, 333, 24),
}


class IntCase(_Made):
    """a chain case whose rows, queries and new rows are integers in [-50, 50], float32"""

    def rows_near(self, rng, n, centre=None):
        cent = self.cent
        rows = cent[rng.randint(len(cent), size=n)] + rng.randint(-9, 10, size=(n, cent.shape[1]))
        return np.clip(rows, -50, 50).astype(np.float32)


@functools.lru_cache(maxsize=None)
def int_case(seed):
    """The integer case of a seed: a euclidean float32 index built over integer rows round integer centres, its chain
    drawn by lc.draw_op as it is (odd seeds: step 0 is lc.edge_removal)."""
    from tinyknn_amd import IVF, FastPQ
    d, kp, L, n, nq = INT_SHAPES[seed]
    rng = np.random.RandomState(lc.STREAM + ATTRS + 800000 + seed)
    shape = dict(d=d, n=n, n_clusters=L, metric="euclidean", build_probes=kp, k=10, n_probes=L + 3, nq=nq, store="float32",
                 groups=False, steered=seed % 2 == 1, n_ops=6)
    case = IntCase(1000 + seed, shape)
    case.cent = cent = rng.randint(-40, 41, size=(max(L, 3), d))
    X = case.rows_near(rng, n)
    qs = case.rows_near(rng, nq)
    ivf = IVF("euclidean", L, FastPQ(2, rotate_dim=None))
    state = np.random.get_state()
    np.random.seed(lc.STREAM + ATTRS + 810000 + seed)
    try:
        ivf.fit(X).build(X, n_probes=kp, device=False)
    finally:
        np.random.set_state(state)
    assert len(ivf.active_centers) == L, "inactive centres"
    _finish(case, ivf, cent, qs)
    np.testing.assert_array_equal(case.qn, qs)                  # (euclidean: the preparation leaves the rows alone)
    m = case.model()
    if shape["steered"]:
        _op(case, m, "remove", "edges", ids=lc.edge_removal(m, rng))
    for _ in range(shape["n_ops"]):
        op = lc.draw_op(case, m, rng, {})
        case.ops.append(op)
        m.apply(op)
    return case
