"""Indexes whose rows lie beyond the offsets at which an address `rows + id * d` wraps when the product is formed in 32
bits, and the references of every row-addressed call on them.  With float32 rows of d = 128 the byte offset
passes 2^32 at row 2^30 / d, the element offset 2^31 at row 2^31 / d and 2^32 at row 2^32 / d: the three BOUNDARIES.  The
default shape, N = 2^25 + 2^16 rows, has rows behind all three; tests/test_offsets_gpu.py builds it in HBM.
tests/test_offsets_cpu.py runs this module at N = 6000, d = 20 with the boundaries moved to rows 1500, 3000 and 5999 on
a host-built index and holds every helper below against the reference it shortens.  No GPU is needed to import it.

The marked set S (about 600 rows): the four rows b - 2 .. b + 1 round every boundary b, row 0, row N - 1 and 140 random
rows in each of the four bands the boundaries cut.  S is group GROUP, carries tag bit TAG_BIT and the values VALUE0 +
rank; every other row has another group, no such tag and a negative value.  So a call restricted to S by any of the three
reads S's rows and nothing else, and its reference needs S's rows alone: `rows_S`, which the caller makes WITHOUT reading
the index under test (the seeded generator, one row at a time).  The helpers rank over rows_S with the suite's existing
references and map positions in S back to row ids; S ascends, so ties by row id keep their order.

Calls that read other rows (query_batch, radius_search(n_probes=)) go to the CPU oracle on a sparse file of vectors, as
tests/test_c5_full_size_gpu.py feeds it: `fill` writes the rows a reference will read — heaps taken from the oracle's own
first pass, never from the device's answer."""
import numpy as np

from allowed_reference import guarded_batch
from between_exact_reference import knn_between_reference
from brute_reference import numpy_part, pad_chunk
from brute_restricted_reference import restricted_dist, restricted_k_best
from group_exact_reference import knn_group_reference
from per_group_reference import capped_from_heaps
from radius_probe_reference import candidates, oracle_probes, radius_probe_csr
from radius_reference import radius_csr
from rows_reference import excluded_batch

D, N, N_LISTS, SEED, SIGMA = 128, 2**25 + 2**16, 4096, 27, 0.7
GROUP, OTHER_GROUPS, TAG_BIT, VALUE0 = 7, 1000, 5, 10**6
PER_BAND, N_QS, N_ANY = 140, 32, 300


def boundaries(d=D):
    """the rows at which byte offsets pass 2^32 (float32), element offsets 2^31 and element offsets 2^32"""
    return (2**30 // d, 2**31 // d, 2**32 // d)


def bands(n, B):
    """the four row ranges [lo, hi) the boundaries cut [0, n) into"""
    edges = [0, *B, n]
    return list(zip(edges[:-1], edges[1:]))


def band_of(rows, B):
    """the band (0 .. 3) of each row id"""
    return np.searchsorted(np.asarray(B), np.asarray(rows), side="right")


def around(B, lo=-2, hi=1):
    """the rows b + lo .. b + hi of every boundary"""
    return np.array([b + o for b in B for o in range(lo, hi + 1)], dtype=np.int64)


class Case:
    """One shape (n, d, B): the marked set, the row attributes, and — once `rows_S` and `any_rows` are given — the
    queries.  Nothing here touches an index."""

    def __init__(self, n=N, d=D, B=None, seed=SEED, n_lists=N_LISTS, attributes=True):
        self.n, self.d, self.B, self.seed, self.n_lists = n, d, tuple(boundaries(d) if B is None else B), seed, n_lists
        assert 2 < self.B[0] and self.B[0] + 1 < self.B[1] - 2 and self.B[1] + 1 < self.B[2] - 2 and self.B[2] + 1 < n
        rng = np.random.RandomState(seed)
        self.centres = rng.randn(1000, d).astype(np.float32)
        picks = [rng.randint(lo, hi, size=PER_BAND) for lo, hi in bands(n, self.B)]
        self.S = np.unique(np.concatenate([around(self.B), [0, n - 1], *picks])).astype(np.int64)
        s = len(self.S)
        # the sources of Q_S: the rows round every boundary and five more of S in every band
        near = around(self.B)
        free = np.setdiff1d(self.S, near)
        pick = np.random.RandomState(seed + 3)
        more = [pick.choice(free[band_of(free, self.B) == b], 5, replace=False) for b in range(4)]
        self.src = np.concatenate([near, *more]).astype(np.int64)
        assert len(self.src) == N_QS == len(np.unique(self.src))
        self.q0_rows = near
        self._noise = (1e-3 * pick.randn(N_QS, d)).astype(np.float32)
        if not attributes:          # (the marked set alone: what test_offsets_cpu.py asserts of the default shape)
            return
        # every other row: one of OTHER_GROUPS groups that is not GROUP, a negative value, tags without TAG_BIT
        g = rng.randint(0, OTHER_GROUPS, size=n).astype(np.int32)
        g[g >= GROUP] += 1
        g[self.S] = GROUP
        self.groups = g
        v = -1 - rng.randint(0, 10**6, size=n).astype(np.int64)
        v[self.S] = VALUE0 + np.arange(s)
        self.values = v
        t = rng.randint(0, 256, size=n).astype(np.uint64) & ~np.uint64(1 << TAG_BIT)
        t[self.S] |= np.uint64(1 << TAG_BIT)
        self.tags = t
        self.value_range = (VALUE0, VALUE0 + s - 1)

    def at(self, rows):
        """positions in S of row ids that are in S"""
        pos = np.searchsorted(self.S, rows)
        assert np.array_equal(self.S[pos], rows)
        return pos

    def set_rows(self, rows_S, any_rows):
        """rows_S: (len(S), d) float32, S's vectors from the generator; any_rows: (N_ANY, d) rows of another seed"""
        assert rows_S.shape == (len(self.S), self.d) and rows_S.dtype == np.float32
        self.rows_S = rows_S
        self.Q_S = (rows_S[self.at(self.src)] + self._noise).astype(np.float32)
        self.Q0 = rows_S[self.at(self.q0_rows)].copy()
        self.Q_any = np.ascontiguousarray(any_rows, dtype=np.float32)
        return self

    def restrictions(self, nq):
        """the three restrictions that each select exactly S, as the device calls take them, and all three together"""
        lo, hi = self.value_range
        g = dict(group=np.full(nq, GROUP, np.int32))
        t = dict(tags=np.full(nq, 1 << TAG_BIT, np.uint64))
        b = dict(between=(np.full(nq, lo, np.int64), np.full(nq, hi, np.int64)))
        return {"group": g, "tags": t, "between": b, "all three": {**g, **t, **b}}

    def to_ids(self, local):
        """positions in S (-1 kept) -> row ids"""
        local = np.asarray(local)
        return np.where(local >= 0, self.S[np.maximum(local, 0)], -1).astype(np.int64)


def handmade_pq(ivf, sample, rng):
    """tests/pq_shapes.py's codebook (dims_per_block 2, no rotation, no k-means) from sampled rows"""
    from tinyknn_amd.fast_pq import dpad
    from tinyknn_amd.utils import pad2
    pq, dpb = ivf.pq, ivf.pq.dims_per_block
    P = pad2(sample, 16, dpad * dpb)
    dq = P.shape[1]
    blocks = dq // dpb
    pick = rng.randint(len(sample), size=(blocks, 16))
    books = P.reshape(len(P), blocks, dpb)[pick, np.arange(blocks)[:, None]] + 0.01 * rng.randn(blocks, 16, dpb)
    pq.centers = np.array(list(books), dtype=np.float32).transpose(1, 0, 2).reshape(16, dq)
    pq.sqrt_n_blocks = np.sqrt(blocks)


def unbuilt_ivf(case, sample):
    """a euclidean IVF with coarse centres sampled from `sample` (the first rows of the data set: every centre is some
    row's nearest) and the hand-made codebook, ready for build / build_resident"""
    from tinyknn_amd import IVF, FastPQ
    rng = np.random.RandomState(case.seed + 1)
    ivf = IVF("euclidean", case.n_lists, FastPQ(2, rotate_dim=None))
    ivf.all_centers = sample[rng.choice(len(sample), case.n_lists, replace=False)].copy()
    handmade_pq(ivf, sample, rng)
    return ivf


def set_attributes(ivf, case):
    ivf.set_groups(case.groups)
    ivf.set_tags(case.tags)
    ivf.set_values(case.values)


# ---- references over S's rows alone ------------------------------------------------------------------------------------

def group_reference(oracle, case, qn, k, rows_S=None, keep=None):
    """knn_group(qn, k, GROUP): group_exact_reference over S's rows; keep: the bool mask over S of rows still stored"""
    rows_S = case.rows_S if rows_S is None else rows_S
    zeros = np.zeros(len(qn), np.int32)
    ids, dist = knn_group_reference(oracle, qn, rows_S, k, zeros, np.zeros(len(rows_S), np.int32), stored=keep)
    return case.to_ids(ids), dist


def between_reference(oracle, case, qn, k, rows_S=None, keep=None):
    """knn_between(qn, k, case.value_range): between_exact_reference over S's rows and values"""
    rows_S = case.rows_S if rows_S is None else rows_S
    lo, hi = case.value_range
    between = (np.full(len(qn), lo, np.int64), np.full(len(qn), hi, np.int64))
    ids, dist = knn_between_reference(oracle, qn, rows_S, k, between, case.values[case.S], stored=keep)
    return case.to_ids(ids), dist


def part_S(case, qn):
    """numpy's `part` of the queries against S's rows (brute_reference.numpy_part on a whole chunk of 100 queries)"""
    return numpy_part(pad_chunk(qn, np.random.RandomState(case.seed + 2)), case.rows_S)[:len(qn)]


def brute_reference(case, qn, k, part=None):
    """knn_brute_dist(qn, k) under a restriction that selects S: (ids, part)"""
    part = part_S(case, qn) if part is None else part
    ok = np.ones(len(case.S), dtype=bool)
    local = np.stack([restricted_k_best(part[i], ok, k) for i in range(len(qn))])
    return case.to_ids(local), np.stack([restricted_dist(part[i], local[i]) for i in range(len(qn))])


def radius_reference(case, part, radius):
    """radius_search(qn, radius) under a restriction that selects S, or where no other row lies within: CSR"""
    lims, local, dist = radius_csr(part, None, radius)
    return lims, case.to_ids(local), dist


def kth_part(part, k):
    """every query's k-th smallest part as its float32 radius"""
    return np.sort(part, axis=1)[:, k - 1].astype(np.float32)


def own_radius(case, part):
    """Q0's part against S: the float32 radius that just admits every query's own row.  An exact copy's part is
    (|x|^2 + |x|^2) - 2 x.x with the norms and the product summed in different orders: a few ulp of |x|^2 from zero,
    on either side, so a radius of 1e-6 admits only some of them."""
    return np.float32(part[np.arange(len(part)), case.at(case.q0_rows)].max())


def kth_dist(csr, k):
    """every query's k-th distance of a sorted float32 CSR result as its radius, +inf where it lists fewer"""
    lims, _, dist = csr
    return np.array([dist[a + k - 1] if b - a >= k else np.inf for a, b in zip(lims[:-1], lims[1:])], dtype=np.float32)


def nearest_groups(case, csr):
    """the group of every query's nearest listed row (every list holds one)"""
    lims, ids, _ = csr
    assert (np.diff(lims) > 0).all()
    return case.groups[ids[lims[:-1]]].astype(np.int32)


# ---- references on the oracle and a sparse file of vectors ------------------------------------------------------------

def oracle_of(oracle, ivf_like, lists, data):
    """The oracle's copy of an index from its exported lists (sizes, packed codes, ids) and `data`, which it must not
    copy: a sparse (N, d) file."""
    sizes, codes, ids = lists
    L = len(sizes)
    coff = np.concatenate([[0], np.cumsum((sizes + 15) // 16)])
    ioff = np.concatenate([[0], np.cumsum(sizes)])
    ox = oracle.OracleIndex(ivf_like.pq.centers, 2, ivf_like.pq.R, ivf_like.pq.sqrt_n_blocks, ivf_like.active_centers,
                            ivf_like.pq_transformed_centers.packed,
                            [codes[coff[i]:coff[i + 1]] for i in range(L)], list(sizes),
                            [ids[ioff[i]:ioff[i + 1]] for i in range(L)], data)
    assert ox.data is data or np.may_share_memory(ox.data, data), "the oracle copied the sparse vector file"
    return ox


def fill(data, rows, fetch):
    """data[rows] = fetch(rows) for the distinct rows >= 0"""
    rows = np.unique(np.asarray(rows).ravel())
    rows = rows[rows >= 0]
    if len(rows):
        data[rows] = fetch(rows)
    return rows


def heaps(ox, qn, k, n_probes):
    """heap_idx (nq, R) of the oracle's unrestricted query: it does not depend on the vectors"""
    return np.stack([ox.query(q, k, n_probes, debug=True)[1]["heap_idx"] for q in qn])


def distances(oracle, qn, data, ids):
    """the rescoring's float32 distances of the ids, +inf beside -1"""
    out = np.full(ids.shape, np.inf, dtype=np.float32)
    for i in range(len(ids)):
        live = ids[i] >= 0
        out[i][live] = oracle.sqdist_gather(qn[i], data, ids[i][live]).astype(np.float32)
    return out


def batch_reference(oracle, ox, qn, k, n_probes, data, fetch):
    """query_batch(return_distances=True): (ids, distances, heap_idx) from the oracle, the heaps' rows fetched first"""
    h = heaps(ox, qn, k, n_probes)
    fill(data, h, fetch)
    ids = ox.query_batch(qn, k, n_probes)
    return ids, distances(oracle, qn, data, ids), h


def capped_reference(oracle, ox, qn, h, per_group, groups, k):
    """query_batch(per_group=, return_distances=True) from batch_reference's heaps (their rows are in the file):
    per_group_reference.capped_batch from the heap on -> (ids, distances)"""
    return capped_from_heaps(oracle, ox, qn, h, per_group, groups, k)[:2]


def tagged_reference(oracle, case, ox, qn, k, n_probes, data, rows_S=None):
    """query_batch(tags=1 << TAG_BIT, return_distances=True): the guarded reference with S as the allowed set; only
    S's rows can reach a heap, and they are written from rows_S (the half store: its rounding)"""
    data[case.S] = case.rows_S if rows_S is None else rows_S
    mask = np.zeros(case.n, dtype=bool)
    mask[case.S] = True
    ids = guarded_batch(oracle, ox, qn, k, n_probes, allowed=mask)
    return ids, distances(oracle, qn, data, ids)


def rows_reference(oracle, ox, rows, qn, qp, k, n_probes, data, fetch):
    """query_rows(rows, k, n_probes, return_distances=True): rows_reference.excluded_batch, a first pass for the heaps'
    rows; qn / qp: the gathered queries (qp the device-made table-build query)"""
    _, dbg = excluded_batch(oracle, ox, qn, rows, k, n_probes, q_pq=qp, debug=True)
    fill(data, dbg["heap_idx"], fetch)
    ids = excluded_batch(oracle, ox, qn, rows, k, n_probes, q_pq=qp)
    return ids, distances(oracle, qn, data, ids)


def probe_reference(oracle, ox, qn, radius, n_probes, data, fetch, oks=None, n=None):
    """radius_search(n_probes=): radius_probe_reference.radius_probe_csr with only the probed lists' rows fetched
    (fetch None: they are in the file already) -> (CSR, probes)"""
    probes = oracle_probes(ox, qn, n_probes)
    n = len(data) if n is None else n
    if fetch is not None:
        fill(data, np.concatenate([candidates(ox, p, n) for p in probes]), fetch)
    return radius_probe_csr(oracle, ox, qn, data, radius, n_probes, oks=oks, probes=probes), probes


def group_masks(case, group, n=None):
    """brute_restricted_reference.passes(i, n, group=group, groups=case.groups) for every query, one comparison each;
    n > case.n: the rows added behind carry no group of the case"""
    masks = [case.groups == g for g in group]
    if n is not None and n > case.n:
        masks = [np.concatenate([m, np.zeros(n - case.n, dtype=bool)]) for m in masks]
    return masks
