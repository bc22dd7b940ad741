"""Offline build path on the MI355X: tk_encode_pq / tk_assign_lists against
the oracle, the golden fixtures (codes and list memberships produced by the compiled
reference) and the product's own host (numpy) build."""
import numpy as np
import pytest

import build_shapes as B
from conftest import G6_TAGS, golden, split_lists

pytestmark = pytest.mark.gpu


def _same_up_to_exact_ties(oracle, pq, X, a, b):
    """Packed codes a and b may differ only where numpy's own `part` values of the two
    labels are EXACTLY equal (random data does produce a few such ties, mostly for
    dims_per_block = 1, and numpy's AVX-512 argselect then need not return the first)."""
    la, lb = oracle.unpack(a), oracle.unpack(b)
    bad = np.argwhere(la != lb)
    assert len(bad) <= 1e-5 * la.size + 2
    dpb = pq.dims_per_block
    Xp = np.concatenate([X, np.zeros((len(la) - len(X), X.shape[1]), X.dtype)])
    pad = (-X.shape[1]) % (4 * dpb)
    Xp = np.concatenate([Xp, np.zeros((len(Xp), pad), X.dtype)], axis=1)
    if pq.R is not None:
        Xp = Xp @ pq.R.T
    for i, m in bad:
        lo = i - i % 100                                  # the chunk numpy scored the row in
        xc = Xp[lo:lo + 100, m * dpb:(m + 1) * dpb]
        code = pq.centers[:, m * dpb:(m + 1) * dpb]
        part = (np.einsum("ij,ij->i", xc, xc)[:, None] + np.einsum("ij,ij->i", code, code)[None]
                - 2 * xc @ code.T)[i - lo]
        assert part[la[i, m]] == part[lb[i, m]] == part.min()


def _pq(centers, dpb, R=None):
    from tinyknn_amd import FastPQ
    pq = FastPQ(dpb)
    pq.centers = centers
    pq.R = R
    return pq


@pytest.mark.parametrize("dpb,d,rot,f64", [(2, 100, False, False), (1, 100, False, False),
                                           (4, 100, False, False), (2, 128, True, False),
                                           (2, 20, False, True), (8, 64, False, False)])
def test_encode_vs_oracle(oracle, dpb, d, rot, f64):
    rng = np.random.RandomState(3)
    n = 5000
    pad = (-d) % (4 * dpb)
    R = np.linalg.qr(rng.randn(d + pad, d + pad))[0][:64] if rot else None
    dq = 64 if rot else d + pad
    for ties in (False, True):
        X = rng.randn(n, d).astype(np.float64 if f64 else np.float32)
        X[17] = 0                                         # a zero row (what pads a list)
        centers = (rng.randn(16, dq) * 0.8).astype(np.float32)
        if ties:
            # exact ties between centroids: integer rows, half-integer centroids, a duplicate.
            # First occurrence wins (numpy's generic argpartition path; its AVX-512 network
            # may pick another tied entry, so numpy itself is compared on tie-free data only)
            X[100:400] = np.round(X[100:400])
            centers = np.round(centers * 2) / 2
            centers[5] = centers[3]
        pq = _pq(centers, dpb, R)
        got = pq.transform(X, device=True)
        want_n, want = oracle.fastpq_transform(centers, dpb, R, X)
        assert got.size == want_n
        np.testing.assert_array_equal(got.packed, want)
        if not ties:
            host = pq.transform(X, device=False)          # numpy, as the reference
            _same_up_to_exact_ties(oracle, pq, X, got.packed, host.packed)


@pytest.mark.parametrize("tag", G6_TAGS)
def test_encode_reproduces_reference_codes(tag):
    g = golden(f"g6_ivf_{tag}.npz")
    codes, ids = split_lists(g)
    pq = _pq(g["pq_centers"], 2, g["R"] if "R" in g else None)
    for l, rows in enumerate(ids):
        if len(rows):
            np.testing.assert_array_equal(pq.transform(g["data"][rows], device=True).packed, codes[l])
    np.testing.assert_array_equal(pq.transform(g["active_centers"], device=True).packed,
                                  g["center_codes"])


def _assign(X, Y, k, metric):
    from tinyknn_amd import IVF
    ivf = IVF(metric, len(Y))
    ivf.all_centers = Y
    return ivf._nearest_on_device(X, k)


@pytest.mark.parametrize("metric,y64,k,L", [("euclidean", False, 1, 244), ("angular", False, 2, 1087),
                                            ("angular", False, 1, 1087), ("euclidean", False, 1, 33),
                                            ("angular", True, 1, 40), ("euclidean", True, 2, 300),
                                            ("euclidean", False, 2, 2)])
def test_assign_vs_oracle_and_numpy(oracle, metric, y64, k, L):
    from tinyknn_amd.utils import knn_brute
    rng = np.random.RandomState(7)
    n, d = 2317, 100                                      # 23 whole chunks + 17 rows in numpy
    X = rng.randn(n, d).astype(np.float32)
    Y = rng.randn(L, d).astype(np.float64 if y64 else np.float32)
    got = _assign(X, Y, k, metric)
    if k < L:      # k == L: bottom_k_2d returns arange without looking (utils.py:29-30)
        np.testing.assert_array_equal(got[:2300], oracle.assign(X[:2300], Y, k, metric))
    np.testing.assert_array_equal(got, knn_brute(X, Y, k, metric))
    if L > 10:     # exact ties (duplicated centres, incl. centre 0; points ON centres): the
        Y[7] = Y[0]                                       # oracle's dumb_select order
        Y[9] = Y[3]
        Y[L - 1] = Y[0]
        X[:50] = Y[rng.randint(L, size=50)].astype(np.float32)
        got = _assign(X, Y, k, metric)
        np.testing.assert_array_equal(got[:2300], oracle.assign(X[:2300], Y, k, metric))


@pytest.mark.parametrize("tag", [t for t in G6_TAGS if "f64" not in t])
def test_assign_reproduces_reference_lists(tag):
    g = golden(f"g6_ivf_{tag}.npz")
    k = int(g["build_probes"])
    near = _assign(np.ascontiguousarray(g["data"], dtype=np.float32), g["active_centers"], k,
                   str(g["metric"]))
    sizes = g["list_sizes"]
    ioff = np.concatenate([[0], np.cumsum(sizes)])
    for l in range(len(sizes)):
        want = g["ids"][ioff[l]:ioff[l + 1]]
        o = 0
        for j in range(k):
            run = np.nonzero(near[:, j] == l)[0]
            np.testing.assert_array_equal(run, np.sort(want[o:o + len(run)]))
            o += len(run)
        assert o == len(want)


@pytest.mark.parametrize("metric,d,rot,probes", [("angular", 100, False, 1), ("euclidean", 128, True, 2)])
def test_device_build_equals_host_build(metric, d, rot, probes):
    """IVF.build(device=True) == IVF.build(device=False): same lists, ids, codes."""
    from tinyknn_amd import IVF, FastPQ
    rng = np.random.RandomState(1)
    np.random.seed(7)       # sklearn's KMeans and FastPQ.fit draw from numpy's global generator: the same fit every run
    n = 20037
    cent = rng.randn(60, d)
    X = (cent[rng.randint(60, size=n)] + 0.6 * rng.randn(n, d)).astype(np.float32)
    a = IVF(metric, 141, FastPQ(2))
    a.fit(X[:8000])
    b = IVF(metric, 141, FastPQ(2))
    b.all_centers, b.pq = a.all_centers, a.pq
    a.build(X, n_probes=probes, device=False)
    b.build(X, n_probes=probes, device=True)
    assert (a.pq.R is not None) == rot
    np.testing.assert_array_equal(a.active_centers, b.active_centers)
    np.testing.assert_array_equal(a.pq_transformed_centers.packed, b.pq_transformed_centers.packed)
    for l in range(len(a.active_centers)):
        np.testing.assert_array_equal(a.ids[l], b.ids[l])
        ta, tb = a.pq_transformed_points[l], b.pq_transformed_points[l]
        assert isinstance(ta, np.ndarray) == isinstance(tb, np.ndarray)
        if not isinstance(ta, np.ndarray):
            assert ta.size == tb.size
            np.testing.assert_array_equal(ta.packed, tb.packed)


# ---------------------------------------------------------------------------------------------------------------
# The shape table of build_shapes.py: every kernel form of tk_launch_assign / tk_launch_encode_pq, named in the
# test id, against the oracle — exactly, on random and on tied data alike.  (tests/test_build_path.py holds the
# other leg: oracle == numpy on the same inputs.)

def _assign_lists(X, Y, k, normalise):
    """tk_assign_lists as IVF._nearest_on_device calls it, without its restriction to whole 100-row chunks:
    -> (return code, nearest (n, k)).  Angular: the centres are normalised here in numpy (utils.py:75), the rows
    on the device."""
    from tinyknn_amd import _lib
    if normalise:
        Y = Y / np.linalg.norm(Y, axis=1, keepdims=True)
    Y = np.ascontiguousarray(Y)
    yn = np.ascontiguousarray(np.einsum("ij,ij->i", Y, Y))
    assert X.dtype == np.float32 and Y.dtype in (np.float32, np.float64) and yn.dtype == Y.dtype
    out = np.full((len(X), k), -7, dtype=np.int64)
    rc = _lib.lib().tk_assign_lists(_lib.ptr(X, _lib._f32p), len(X), X.shape[1], int(normalise), Y.ctypes.data,
                                    int(Y.dtype == np.float64), yn.ctypes.data, len(Y), k,
                                    _lib.ptr(out, _lib._i64p))
    return rc, out


@pytest.mark.parametrize("case", B.ASSIGN_CASES, ids=B.ASSIGN_IDS)
def test_assign_table_vs_oracle(oracle, case):
    from tinyknn_amd import _lib
    assert B.form_of(case.y64, case.k, case.d) == case.form
    X, Y = B.assign_inputs(case)
    rc, got = _assign_lists(X, Y, case.k, case.metric == "angular")
    _lib.check(rc)
    np.testing.assert_array_equal(got, oracle.assign(X, Y, case.k, B.oracle_metric(case)))


@pytest.mark.parametrize("y64", [False, True])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_assign_lists_refuses_d_above_384_and_k_above_L(y64, k):
    from tinyknn_amd import _lib
    rng = np.random.RandomState(2)
    Y = rng.randn(12, 385).astype(np.float64 if y64 else np.float32)
    X = rng.randn(37, 385).astype(np.float32)
    rc, out = _assign_lists(X, Y, k, False)
    assert rc == -1 and b"d > 384" in _lib.lib().tk_last_error()
    assert (out == -7).all()
    Y, X = np.ascontiguousarray(Y[:k, :384]), np.ascontiguousarray(X[:, :384])      # k = L is the most: L + 1 is refused
    rc, out = _assign_lists(X, Y, k + 1, False)
    assert rc == -1 and b"k must be 1 .. 9" in _lib.lib().tk_last_error()
    assert (out == -7).all()
    rc, out = _assign_lists(X, Y, k, False)                                          # the library goes on working
    _lib.check(rc)
    np.testing.assert_array_equal(np.sort(out, axis=1), np.tile(np.arange(k), (37, 1)))


@pytest.mark.parametrize("metric,d", [("euclidean", 385), ("angular", 129)])
@pytest.mark.parametrize("k", [1, 2])
def test_nearest_on_device_beyond_the_device_limits_is_numpys(metric, d, k):
    """d > 384, and angular rows of more than 128 elements, are numpy's knn_brute itself (IVF._nearest_on_device)."""
    from tinyknn_amd.utils import knn_brute
    rng = np.random.RandomState(d + k)
    X = rng.randn(233, d).astype(np.float32)
    Y = rng.randn(33, d).astype(np.float32)
    np.testing.assert_array_equal(_assign(X, Y, k, metric), knn_brute(X, Y, k=k, metric=metric))


@pytest.mark.parametrize("case", B.ENCODE_CASES, ids=B.ENCODE_IDS)
def test_encode_table_vs_oracle(oracle, case):
    centers, X = B.encode_inputs(case)
    got = _pq(centers, case.dpb).encode_labels(X, device=True)
    assert got.shape == (case.n, case.dq // case.dpb) and got.dtype == np.uint8
    np.testing.assert_array_equal(got, oracle.encode_pq(centers, case.dpb, X))


@pytest.mark.parametrize("dpb,d,rdim", [(2, 36, 24), (16, 100, 64)])
def test_encode_rotated_float32_rows_through_transform(oracle, dpb, d, rdim):
    """float32 rows, padded and rotated by FastPQ.transform itself (the rotated rows are float64): a strip tail
    at dims_per_block 2, the generic kernel at 16."""
    rng = np.random.RandomState(9)
    pad = (-d) % (4 * dpb)
    R = np.linalg.qr(rng.randn(d + pad, d + pad))[0][:rdim]
    X = rng.randn(333, d).astype(np.float32)
    X[7] = 0
    centers = (rng.randn(16, rdim) * 0.3).astype(np.float32)
    centers[9] = centers[4]
    pq = _pq(centers, dpb, R)
    got = pq.transform(X, device=True)
    want_n, want = oracle.fastpq_transform(centers, dpb, R, X)
    assert got.size == want_n == 333
    np.testing.assert_array_equal(got.packed, want)
    _same_up_to_exact_ties(oracle, pq, X, got.packed, pq.transform(X, device=False).packed)


def test_encode_codebook_past_the_lds_budget_is_refused_before_any_launch(oracle):
    """dims_per_block 1: 384 M + 34 816 bytes of LDS; M = 336 is the last that fits 160 KiB (encoded against the
    oracle in the table above).  The next widths — 337 for tk_encode_pq itself, 340 for FastPQ's padding to 4
    blocks — are an argument error: nothing is launched, no label is written, the next call works."""
    from tinyknn_amd import _lib
    assert 384 * B.ENC_LDS_MAX_DQ + 34816 <= 160 * 1024 < 384 * (B.ENC_LDS_MAX_DQ + 1) + 34816
    rng = np.random.RandomState(4)
    for dq in (B.ENC_LDS_MAX_DQ + 1, B.ENC_LDS_MAX_DQ + 4):
        for f64 in (False, True):
            X = rng.randn(65, dq).astype(np.float64 if f64 else np.float32)
            centers = rng.randn(16, dq).astype(np.float32)
            labels = np.full((65, dq), 0xAB, dtype=np.uint8)
            rc = _lib.lib().tk_encode_pq(_lib.ptr(centers, _lib._f32p), dq, 1, X.ctypes.data, int(f64), 65,
                                         _lib.ptr(labels, _lib._u8p))
            assert rc == -1 and b"codebook larger than the LDS budget" in _lib.lib().tk_last_error()
            assert (labels == 0xAB).all()
    with pytest.raises(AssertionError, match="codebook larger than the LDS budget"):
        _pq(centers, 1).encode_labels(X, device=True)
    case = B.ENCODE_CASES[-1]
    assert case.dq == B.ENC_LDS_MAX_DQ and case.dpb == 1
    centers, X = B.encode_inputs(case)
    np.testing.assert_array_equal(_pq(centers, 1).encode_labels(X, device=True), oracle.encode_pq(centers, 1, X))


def _runs_sorted(ivf, l):
    """(ids, labels) of list l with every column block (the rows whose j-th nearest centre is l) in ascending id
    order: inside a block the order is numpy's unstable argsort's in a host build, ascending after IVF.add."""
    from tinyknn_amd._transform import unpack
    ids = np.asarray(ivf.ids[l], dtype=np.int64)
    lab = unpack(ivf.pq_transformed_points[l].packed)[:len(ids)] if len(ids) else np.zeros((0, 0), np.uint8)
    o, order = 0, []
    for c in ivf.list_columns[l]:
        order.append(o + np.argsort(ids[o:o + c], kind="stable"))
        o += int(c)
    assert o == len(ids)
    order = np.concatenate(order)
    return ids[order], lab[order]


@pytest.mark.parametrize("metric,d,probes,rot,form", [("euclidean", 200, 1, False, B.F1), ("angular", 33, 2, True, B.F2)],
                         ids=["euclidean-d200-" + B.F1, "angular-d33-" + B.F2])
def test_device_build_and_add_equal_host_build_at_other_widths(metric, d, probes, rot, form):
    """IVF.build(device=True) == IVF.build(device=False) in lists, ids and codes at widths off the 20/100/128 the
    other tests use: the float32 VALU form of the assignment (d > 128) and the row normalisation at an odd d
    inside a real build; then IVF.add of 150 rows on the device index gives the lists of a host build of all rows."""
    from tinyknn_amd import IVF, FastPQ
    rng = np.random.RandomState(5)
    np.random.seed(11)                # sklearn's KMeans draws from numpy's global generator: the same fit every run
    n0, n1, lists = 6037, 150, 40
    cent = rng.randn(lists, d)
    X = (cent[rng.randint(lists, size=n0 + n1)] + 0.5 * rng.randn(n0 + n1, d)).astype(np.float32)
    # d = 200: the fixed code, unrotated; d = 33: FastPQ's default, rows padded to 40 and rotated (float64)
    a = IVF(metric, lists, FastPQ(2) if rot else FastPQ(2, use_kmeans=False, rotate_dim=None))
    a.fit(X[:3000])
    assert (a.pq.R is not None) == rot and a.all_centers.dtype == np.float32
    assert B.form_of(False, probes, d) == form

    def index():
        ivf = IVF(metric, lists, FastPQ(2))
        ivf.all_centers, ivf.pq = a.all_centers, a.pq
        return ivf

    b, whole = index(), index()
    a.build(X[:n0], n_probes=probes, device=False)
    b.build(X[:n0], n_probes=probes, device=True)
    assert len(a.active_centers) == lists
    np.testing.assert_array_equal(a.active_centers, b.active_centers)
    np.testing.assert_array_equal(a.pq_transformed_centers.packed, b.pq_transformed_centers.packed)
    np.testing.assert_array_equal(a.list_columns, b.list_columns)
    for l in range(lists):
        np.testing.assert_array_equal(a.ids[l], b.ids[l])
        assert a.pq_transformed_points[l].size == b.pq_transformed_points[l].size
        np.testing.assert_array_equal(a.pq_transformed_points[l].packed, b.pq_transformed_points[l].packed)
    dev = b.device_index()
    b.add(X[n0:])
    assert b.device_index() is dev and dev.N == n0 + n1
    whole.build(X, n_probes=probes, device=False)
    np.testing.assert_array_equal(b.list_columns, whole.list_columns)
    for l in range(lists):
        got_ids, got_lab = _runs_sorted(b, l)
        want_ids, want_lab = _runs_sorted(whole, l)
        np.testing.assert_array_equal(got_ids, want_ids)
        np.testing.assert_array_equal(got_lab, want_lab)
