"""tests/offset_shapes.py on the CPU: the builder and every reference helper that tests/test_offsets_gpu.py compares the
device with, at N = 6000, d = 20 on a host-built index, each held against the suite's existing reference run over ALL
rows — so the GPU file compares against code that is itself pinned.  The boundaries are moved to rows 1500, 3000 and
4500 (a third boundary at row 5999 of 6000 would have no row b + 1 and a band of one row, and the conditions below could
not hold).  Also what the marked set must satisfy, on this shape and on the default one."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import offset_shapes as osh  # noqa: E402
from between_exact_reference import knn_between_reference  # noqa: E402
from brute_reference import numpy_part, pad_chunk  # noqa: E402
from brute_restricted_reference import passes, restricted_dist, restricted_k_best  # noqa: E402
from group_exact_reference import knn_group_reference, same_bits  # noqa: E402
from per_group_reference import capped_batch  # noqa: E402
from radius_probe_reference import radius_probe_csr, same_csr  # noqa: E402
from radius_reference import radius_csr  # noqa: E402
from rows_reference import excluded_batch  # noqa: E402
from store_reference import exact_distances, oracle_index, rounded  # noqa: E402
from tags_reference import tagged_batch  # noqa: E402

N, D, B, LISTS = 6000, 20, (1500, 3000, 4500), 16
K, P = 10, 5


class Small:
    pass


@pytest.fixture(scope="module")
def small(oracle):
    """the scaled case, its host-built index, the oracle on all rows and the oracle on a sparse array"""
    case = osh.Case(N, D, B, n_lists=LISTS)
    rng = np.random.RandomState(case.seed + 10)
    X = (case.centres[rng.randint(len(case.centres), size=N)] + osh.SIGMA * rng.randn(N, D)).astype(np.float32)
    any_rows = (case.centres[rng.randint(len(case.centres), size=osh.N_ANY)] +
                osh.SIGMA * rng.randn(osh.N_ANY, D)).astype(np.float32)
    case.set_rows(X[case.S].copy(), any_rows)
    ivf = osh.unbuilt_ivf(case, X[:2000])
    ivf.build(X, n_probes=1, device=False)
    assert len(ivf.active_centers) == LISTS
    s = Small()
    s.case, s.X, s.ivf = case, X, ivf
    s.full = oracle_index(oracle, ivf, X)
    pts = ivf.pq_transformed_points
    lists = (np.array([p.size for p in pts], dtype=np.int64), np.concatenate([p.packed for p in pts]),
             np.concatenate([np.asarray(i, dtype=np.int64) for i in ivf.ids]))
    s.data = np.zeros((N, D), dtype=np.float32)             # the sparse file: only what `fill` writes
    s.sparse = osh.oracle_of(oracle, ivf, lists, s.data)
    s.fetch = lambda rows: X[rows]
    qn, qp = ivf._prepare(case.Q_any.copy())
    s.qn, s.qp = np.ascontiguousarray(qn), np.ascontiguousarray(qp)
    return s


def _conditions(case):
    S, Bs = case.S, case.B
    counts = np.bincount(osh.band_of(S, Bs), minlength=4)
    assert (counts >= 100).all(), counts
    for b in Bs:
        assert np.isin([b - 2, b - 1, b, b + 1], S).all(), b
    assert S[0] == 0 and S[-1] == case.n - 1 and (np.diff(S) > 0).all()
    src_bands = np.bincount(osh.band_of(case.src, Bs), minlength=4)
    assert (src_bands >= 4).all() and np.isin(osh.around(Bs), case.src).all(), src_bands
    assert np.isin(case.src, S).all() and len(case.src) == osh.N_QS
    return counts


def test_the_marked_set_of_both_shapes(small):
    _conditions(small.case)
    big = osh.Case(attributes=False)
    assert (big.n, big.d, big.B) == (2**25 + 2**16, 128, (8388608, 16777216, 33554432))
    counts = _conditions(big)
    assert 550 <= len(big.S) <= 600 and counts.sum() == len(big.S)
    # the offsets the boundaries stand for: the first row whose float32 byte offset needs 33 bits, whose element
    # offset needs 32 bits, and whose element offset needs 33
    for b, limit, size in zip(big.B, (2**32, 2**31, 2**32), (4, 1, 1)):
        assert (b - 1) * big.d * size < limit <= b * big.d * size


def test_the_attributes_select_exactly_the_marked_set(small):
    c = small.case
    mask = np.zeros(N, dtype=bool)
    mask[c.S] = True
    np.testing.assert_array_equal(c.groups == osh.GROUP, mask)
    np.testing.assert_array_equal((c.tags & np.uint64(1 << osh.TAG_BIT)) != 0, mask)
    np.testing.assert_array_equal((c.values >= c.value_range[0]) & (c.values <= c.value_range[1]), mask)
    np.testing.assert_array_equal(c.values[c.S], osh.VALUE0 + np.arange(len(c.S)))
    assert (c.values[~mask] < 0).all() and len(np.unique(c.groups)) > 900
    rs = c.restrictions(3)
    ref = dict(groups=c.groups, row_tags=c.tags, values=c.values)
    for name, kw in rs.items():
        np.testing.assert_array_equal(passes(1, N, **kw, **ref), mask, err_msg=name)
    np.testing.assert_array_equal(c.to_ids(np.array([[0, -1, len(c.S) - 1]])), [[0, -1, N - 1]])


@pytest.mark.parametrize("store", [None, "float16"])
@pytest.mark.parametrize("k", [1, 10, 100])
def test_group_and_between_helpers(oracle, small, k, store):
    c = small.case
    X = rounded(small.X) if store else small.X
    rows_S = rounded(c.rows_S) if store else c.rows_S
    nq = len(c.Q_S)
    want = knn_group_reference(oracle, c.Q_S, X, k, np.full(nq, osh.GROUP), c.groups)
    got = osh.group_reference(oracle, c, c.Q_S, k, rows_S)
    np.testing.assert_array_equal(got[0], want[0])
    assert same_bits(got[1], want[1])
    assert (osh.band_of(want[0][want[0] >= 0], c.B) == 3).any()
    between = c.restrictions(nq)["between"]["between"]
    want = knn_between_reference(oracle, c.Q_S, X, k, between, c.values)
    got = osh.between_reference(oracle, c, c.Q_S, k, rows_S)
    np.testing.assert_array_equal(got[0], want[0])
    assert same_bits(got[1], want[1])
    # rows taken out: the mask over S against the mask over all rows
    gone = c.S[::6]
    stored = np.ones(N, dtype=bool)
    stored[gone] = False
    want = knn_group_reference(oracle, c.Q_S, X, k, np.full(nq, osh.GROUP), c.groups, stored=stored)
    got = osh.group_reference(oracle, c, c.Q_S, k, rows_S, keep=stored[c.S])
    np.testing.assert_array_equal(got[0], want[0])
    assert same_bits(got[1], want[1]) and not np.isin(got[0], gone).any()


def test_brute_and_radius_helpers(small):
    c = small.case
    nq = len(c.Q_S)
    rng = np.random.RandomState(5)
    full = numpy_part(pad_chunk(c.Q_S, rng), small.X)[:nq]
    part = osh.part_S(c, c.Q_S)
    assert part.tobytes() == np.ascontiguousarray(full[:, c.S]).tobytes()
    ref = dict(groups=c.groups, row_tags=c.tags, values=c.values)
    for name, kw in c.restrictions(nq).items():
        oks = [passes(i, N, **kw, **ref) for i in range(nq)]
        for k in (1, 10):
            ids = np.stack([restricted_k_best(full[i], oks[i], k) for i in range(nq)])
            dist = np.stack([restricted_dist(full[i], ids[i]) for i in range(nq)])
            got = osh.brute_reference(c, c.Q_S, k, part)
            np.testing.assert_array_equal(got[0], ids, err_msg=name)
            assert got[1].tobytes() == dist.tobytes(), name
        r = osh.kth_part(part, 20)
        want = radius_csr(full, oks, r)
        got = osh.radius_reference(c, part, r)
        same_csr(got, want, name)
        assert (np.diff(want[0]) >= 20).all()


def test_an_exact_copy_has_no_second_row_within_the_small_radius(small):
    """Q0 = the rows round the boundaries themselves: over ALL rows numpy's part lists within 1e-6 nothing but the row
    itself, and within the radius that admits every row's own part — rounding leaves it a few ulp of |x|^2 from zero,
    on either side — still nothing else.  So S's rows are reference enough for the unrestricted radius call."""
    c = small.case
    nq = len(c.Q0)
    full = numpy_part(pad_chunk(c.Q0, np.random.RandomState(5)), small.X)[:nq]
    part = osh.part_S(c, c.Q0)
    assert part.tobytes() == np.ascontiguousarray(full[:, c.S]).tobytes()
    own = full[np.arange(nq), c.q0_rows]
    for r in (np.float32(1e-6), osh.own_radius(c, part)):
        want = radius_csr(full, None, r)
        same_csr(osh.radius_reference(c, part, r), want)
        for i in range(nq):
            assert set(want[1][want[0][i]:want[0][i + 1]]) <= {c.q0_rows[i]}
    want = radius_csr(full, None, osh.own_radius(c, part))
    np.testing.assert_array_equal(want[1], c.q0_rows)
    assert np.abs(own).max() < 1e-3
    # knn_brute with k = 1 returns the row itself
    ids = np.array([restricted_k_best(full[i], np.ones(N, bool), 1) for i in range(nq)])
    np.testing.assert_array_equal(ids[:, 0], c.q0_rows)
    np.testing.assert_array_equal(osh.brute_reference(c, c.Q0, 1, part)[0], ids)


def test_batch_helpers_on_the_sparse_file(oracle, small):
    c, qn = small.case, small.qn
    small.data[:] = 0
    ids, dist, h = osh.batch_reference(oracle, small.sparse, qn, K, P, small.data, small.fetch)
    want = small.full.query_batch(qn, K, P)
    np.testing.assert_array_equal(ids, want)
    assert same_bits(dist, exact_distances(oracle, qn, small.X, want))
    assert len(np.unique(osh.band_of(ids[ids >= 0], c.B))) == 4
    got = osh.capped_reference(oracle, small.sparse, qn, h, 1, c.groups, K)
    want = capped_batch(oracle, small.full, qn, 1, c.groups, K, P)
    np.testing.assert_array_equal(got[0], want[0])
    assert same_bits(got[1], want[1])
    # tags: on Q_any, and on Q_S, whose sources are marked rows
    for q in (qn[:32], c.Q_S):
        small.data[:] = 0
        got = osh.tagged_reference(oracle, c, small.sparse, q, K, P, small.data)
        want = tagged_batch(oracle, small.full, q, 1 << osh.TAG_BIT, "any", c.tags, K, P)
        np.testing.assert_array_equal(got[0], want)
        assert same_bits(got[1], exact_distances(oracle, q, small.X, want))
    assert (want >= 0).any()


def test_rows_helper_on_the_sparse_file(oracle, small):
    c = small.case
    qn, qp = small.ivf._prepare(small.X[c.src].copy())
    qn, qp = np.ascontiguousarray(qn), np.ascontiguousarray(qp)
    small.data[:] = 0
    got = osh.rows_reference(oracle, small.sparse, c.src, qn, qp, K, P, small.data, small.fetch)
    want = excluded_batch(oracle, small.full, qn, c.src, K, P, q_pq=qp)
    np.testing.assert_array_equal(got[0], want)
    assert same_bits(got[1], exact_distances(oracle, qn, small.X, want))
    assert not (want == c.src[:, None]).any()


def test_probe_helper_on_the_sparse_file(oracle, small):
    c, qn = small.case, small.qn[:16]
    small.data[:] = 0
    everything, probes = osh.probe_reference(oracle, small.sparse, qn, np.inf, P, small.data, small.fetch)
    same_csr(everything, radius_probe_csr(oracle, small.full, qn, small.X, np.inf, P))
    r = osh.kth_dist(everything, 10)
    got, _ = osh.probe_reference(oracle, small.sparse, qn, r, P, small.data, small.fetch)
    same_csr(got, radius_probe_csr(oracle, small.full, qn, small.X, r, P, probes=probes))
    assert (np.diff(got[0]) >= 10).all()
    group = osh.nearest_groups(c, everything)
    oks = osh.group_masks(c, group)
    for i in range(len(qn)):
        np.testing.assert_array_equal(oks[i], passes(i, N, group=group, groups=c.groups))
    got, _ = osh.probe_reference(oracle, small.sparse, qn, np.inf, P, small.data, None, oks=oks)
    same_csr(got, radius_probe_csr(oracle, small.full, qn, small.X, np.inf, P, oks=oks, probes=probes))
    assert (np.diff(got[0]) >= 1).all()
