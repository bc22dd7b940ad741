"""What tests/test_between_gpu.py and tests/test_between_fuzz_gpu.py run the device on, made without a GPU so that
tests/test_between_cpu.py can assert on the reference alone that these inputs can tell a right range pass from a wrong
one: the value assignments over an index's rows, the query ranges of a batch (the kinds in turn), the synthetic index
of the replay-form legs (tests/tag_shapes.py's, imported), and the fuzz cases — the awkward indexes of
tests/restricted_shapes.py (imported, not copied) with values, ranges and, for half of them, tags drawn on top."""
import numpy as np

import tag_shapes as ts

INT64_MIN, INT64_MAX = -2**63, 2**63 - 1
ASSIGNMENTS = ("uniform", "ties", "lists", "extremes", "extremes_int", "two")
RANGE_KINDS = ("two_sided", "low", "high", "point", "empty", "unbounded", "one_column", "stored")
TINY = 5e-324                       # the smallest denormal
FLOAT_POOL = np.array([-np.inf, -np.finfo(np.float64).max, -1.0, -TINY, -0.0, 0.0, TINY, np.finfo(np.float64).tiny,
                       np.nextafter(1.0, 0.0), 1.0, np.nextafter(1.0, 2.0), np.finfo(np.float64).max, np.inf])
INT_POOL = np.array([INT64_MIN, INT64_MIN + 1, -2**53 - 1, -1, 0, 1, 2**53, 2**53 + 1, INT64_MAX - 1, INT64_MAX],
                    dtype=np.int64)


def assignments(ids_per_list, N, seed):
    """name -> values of the N rows:
    uniform       (N,) float32, uniform in [0, 1);
    ties          (N,) int32 in 0 .. 5: a point range hits many rows;
    lists         (N,) int64, the lowest list the row is stored in: whole lists pass or fail;
    extremes      (N,) float64 from FLOAT_POOL: +-inf, +-max, -0.0 and +0.0, denormals, 1.0 and its two neighbours;
    extremes_int  (N,) int64 from INT_POOL: the int64 extremes and their neighbours, integers no float64 holds;
    two           (N, 2) float32: a uniform column and a column of ties."""
    rng = np.random.default_rng(seed)
    uniform = rng.random(N).astype(np.float32)
    ties = rng.integers(0, 6, N).astype(np.int32)
    return dict(uniform=uniform, ties=ties, lists=ts.first_list(ids_per_list, N),
                extremes=FLOAT_POOL[rng.integers(0, len(FLOAT_POOL), N)],
                extremes_int=INT_POOL[rng.integers(0, len(INT_POOL), N)],
                two=np.stack([rng.random(N).astype(np.float32), rng.integers(0, 6, N).astype(np.float32)], axis=1))


def float_bounds(values):
    """Whether a batch's bounds over these values are float64 arrays (floating columns, and the int32 ties: fractions
    that must be ceil'ed / floor'ed, -inf / +inf for an unbounded end) or int64 arrays (INT64_MIN / INT64_MAX for an
    unbounded end)."""
    return values.dtype.kind == "f" or values.dtype == np.int32


def ranges(values, nq, seed, kinds=None):
    """-> (lo, hi, kinds): (nq, C) bounds and the kind of every query's range, RANGE_KINDS in turn (or `kinds`):
    two_sided   two stored values (a half above each where the bounds are floats over integers: passes (a, b]);
    low / high  one stored value, the other end unbounded;
    point       lo == hi == a stored value;
    empty       lo > hi;
    unbounded   every end unbounded;
    one_column  column 0 alone bounded (as `stored`), the others unbounded;
    stored      two stored values: rows with exactly lo and exactly hi exist, and pass.
    Columns behind the first take the middle half of their stored values, except where the kind says otherwise.
    An unbounded end is -inf / +inf in float64 bounds, INT64_MIN / INT64_MAX in int64 bounds: the same truth."""
    rng = np.random.default_rng(seed)
    v = np.asarray(values).reshape(len(values), -1)
    C = v.shape[1]
    fb = float_bounds(v)
    neg, pos = (-np.inf, np.inf) if fb else (INT64_MIN, INT64_MAX)
    lo = np.full((nq, C), neg, dtype=np.float64 if fb else np.int64)
    hi = np.full((nq, C), pos, dtype=np.float64 if fb else np.int64)
    stored = [np.unique(v[:, c]) for c in range(C)]
    out_kinds = []
    for i in range(nq):
        kind = RANGE_KINDS[i % len(RANGE_KINDS)] if kinds is None else kinds[i]
        out_kinds.append(kind)
        for c in range(C):
            s = stored[c]
            a, b = sorted(rng.integers(0, len(s), 2))
            if kind == "unbounded" or (kind == "one_column" and c > 0):
                continue
            if c > 0 and kind != "empty":
                lo[i, c], hi[i, c] = s[len(s) // 4], s[min(len(s) - 1, 3 * len(s) // 4)]
            elif kind in ("two_sided", "stored", "one_column"):
                half = 0.5 if kind == "two_sided" and fb and v.dtype.kind != "f" else 0
                lo[i, c], hi[i, c] = s[a] + half, s[b] + half
            elif kind == "low":
                lo[i, c] = s[a]
            elif kind == "high":
                hi[i, c] = s[b]
            elif kind == "point":
                lo[i, c] = hi[i, c] = s[a]
            else:                                   # empty
                lo[i, c], hi[i, c] = (s[-1], s[0]) if len(s) > 1 else (1, 0)
    return lo, hi, out_kinds


# ---- the synthetic index of tests/tag_shapes.py (one list emptied, one cut to one whole chunk), two value columns ----

SYN_N, SYN_NQ = ts.SYN_N, ts.SYN_NQ


def synthetic(kp):
    """-> (the shared index of tag_shapes.synthetic(kp), raw queries, (N, 2) float32 values, (lo, hi) of its queries,
    the emptied list, the list of 16 rows)"""
    ivf, qs, _, emptied, cut = ts.synthetic(kp)
    L = len(ivf.active_centers)
    values = assignments([ivf.ids[l] for l in range(L)], SYN_N, 8)["two"]
    lo, hi, _ = ranges(values, SYN_NQ, 9)
    return ivf, qs, values, (lo, hi), emptied, cut


# ---- the fuzz cases ----

FUZZ_DEFAULT_SEEDS = 16
# Where the fuzz seeds start among the cases of tests/restricted_shapes.py (seed i here is its case FUZZ_FIRST + i),
# and where the values' own random streams start.  Chosen so that the default seeds hold what the census of
# tests/test_between_cpu.py asserts.
FUZZ_FIRST = 0
FUZZ_STREAM = 6300
VALUE_KINDS = ("uniform", "ties", "lists", "extremes", "two")
_fuzz = {}


def fuzz_seeds():
    """the seeds of a run: FUZZ_DEFAULT_SEEDS, or TINYKNN_FUZZ_SEEDS as in the other fuzz files"""
    import os
    return range(int(os.environ.get("TINYKNN_FUZZ_SEEDS", str(FUZZ_DEFAULT_SEEDS))))


class BetweenCase:
    """case: the restricted_shapes.Case (unchanged, shared); values (of its index's rows after the layout change),
    value_kind, between = (lo, hi) per query, range_kinds; tags / masks / mode where the seed drew tags too (else
    None): all from the seed's own stream"""

    def __init__(self, seed):
        import restricted_shapes as rs
        self.seed = seed
        self.case = case = rs.case(FUZZ_FIRST + seed)
        self.skipped = case.skipped
        if self.skipped is not None:
            return
        rng = np.random.RandomState(FUZZ_STREAM + seed)
        N, nq, L = len(case.ref_data), len(case.qn), case.shape["n_clusters"]
        self.value_kind = kind = VALUE_KINDS[rng.randint(len(VALUE_KINDS))]
        self.values = assignments([case.ivf.ids[l] for l in range(L)], N, FUZZ_STREAM + seed)[kind]
        self.range_kinds = [RANGE_KINDS[rng.randint(len(RANGE_KINDS))] for _ in range(nq)]
        lo, hi, _ = ranges(self.values, nq, FUZZ_STREAM + 1000 + seed, self.range_kinds)
        self.between = (lo, hi)
        self.tags = self.masks = self.mode = None
        if rng.rand() < 0.5:
            self.mode = ts.MODES[rng.randint(2)]
            self.tags = ts.bit(0) << rng.randint(0, 3, N).astype(np.uint64)
            self.masks = np.where(rng.rand(nq) < 0.5, ts.bit(0) << rng.randint(0, 3, nq).astype(np.uint64), ts.U64(0))

    def __repr__(self):
        return f"between seed {self.seed} {self.value_kind} tags={self.mode} on {self.case}"

    def device_kwargs(self, aset=None):
        kw = self.case.device_kwargs(aset)
        kw.update(between=self.between)
        if self.tags is not None:
            kw.update(tags=self.masks, tags_mode=self.mode)
        return kw

    def want(self):
        """the reference answer under the case's own restriction, the ranges and the tags (ids, debug): computed once"""
        if "_want" not in self.__dict__:
            from oracle import oracle
            from between_reference import ranged_batch
            c = self.case
            self.__dict__["_want"] = ranged_batch(oracle, c.ox, c.qn, self.between, self.values, c.shape["k"],
                                                  c.shape["n_probes"], allowed=c.allowed, exclude=c.exclude,
                                                  group=c.group, groups=c.groups, mask=self.masks,
                                                  mode=self.mode or "any", tags=self.tags, debug=True)
        return self.__dict__["_want"]


def fuzz_case(seed):
    if seed not in _fuzz:
        _fuzz[seed] = BetweenCase(int(seed))
    return _fuzz[seed]


def chunk_facts(t):
    """What the ranges of a built BetweenCase do to the chunks its queries probe, on the reference alone (the census of
    tests/test_between_cpu.py): point_pair — a point range passes two rows or more of one chunk; all_beside_none — one
    query probes a chunk of 16 stored rows that all pass and a chunk with stored rows of which none does;
    conjunction — with two bounded columns, a probed row that column 0 alone passes and a probed row that column 1
    alone passes are both rejected."""
    import restricted_shapes as rs
    from between_reference import bounds_of, passing
    c = t.case
    L = c.shape["n_clusters"]
    v = np.asarray(t.values).reshape(len(t.values), -1)
    out = dict(point_pair=False, all_beside_none=False, conjunction=False)
    for i, probes in enumerate(c.base_dbg["probes"]):
        lo, hi = bounds_of(t.between, i)
        ok = passing(t.values, lo, hi)
        cols = [passing(v[:, j], lo[j], hi[j]) for j in range(v.shape[1])]
        full = none = False
        only = [False, False]
        for l in np.unique(rs.probed_lists(probes, L)):
            lab = np.asarray(c.ivf.ids[l], dtype=np.int64)
            for o in range(0, len(lab), 16):
                p = ok[lab[o:o + 16]]
                full |= len(p) == 16 and p.all()
                none |= not p.any()
                if t.range_kinds[i] == "point" and p.sum() >= 2:
                    out["point_pair"] = True
            if len(cols) == 2 and len(lab):
                only[0] |= bool((cols[0][lab] & ~cols[1][lab]).any())
                only[1] |= bool((cols[1][lab] & ~cols[0][lab]).any())
        out["all_beside_none"] |= full and none
        out["conjunction"] |= all(only)
    return out
