"""Exact k nearest vectors on the f32 matrix cores (tk_index_knn_brute)
against numpy's knn_brute formula (utils.py:66-86): the same `part` values bit for bit, the k
smallest in ascending (part, row) order."""
import numpy as np
import pytest

from brute_reference import CAP, int_part, k_best, numpy_part, pad_chunk, segment_rows, within_tau_per_segment  # noqa: E402

pytestmark = pytest.mark.gpu


def _index(data):
    """a DeviceIndex that only needs its vectors: one list holding everything"""
    from tinyknn_amd import IVF, FastPQ
    from tinyknn_amd.fast_pq import TransformedData
    from tinyknn_amd._transform import transform_data
    n, d = data.shape
    dq = d + (-d) % 8
    ivf = IVF("euclidean", 1, FastPQ(2))
    ivf.pq.centers = np.zeros((16, dq), np.float32)
    ivf.pq.sqrt_n_blocks = float(np.sqrt(dq // 2))
    ivf.active_centers = np.zeros((1, d), np.float32)
    ivf.pq_transformed_centers = TransformedData(1, transform_data(np.zeros((16, dq // 2), np.uint8)))
    pad = (-n) % 16
    ivf.pq_transformed_points = [TransformedData(n, transform_data(np.zeros((n + pad, dq // 2), np.uint8)))]
    ivf.ids = [np.arange(n, dtype=np.int64)]
    ivf.data = data
    return ivf.device_index()


def _numpy_part(X, Y):
    xn = np.einsum("ij,ij->i", X, X)
    yn = np.einsum("ij,ij->i", Y, Y)
    out = np.empty((len(X), len(Y)), np.float32)
    for i in range(0, len(X), 100):            # 100-row chunks: the GEMM shape of the reference
        out[i:i + 100] = xn[i:i + 100, None] + yn[None] - 2 * X[i:i + 100] @ Y.T
    return out


@pytest.mark.parametrize("n,d,nq,k", [(20000, 100, 300, 10), (9000, 17, 131, 1), (5000, 128, 200, 100),
                                      (40000, 64, 1000, 10), (700, 20, 5, 10)])
def test_knn_brute_matches_numpy(n, d, nq, k):
    rng = np.random.RandomState(n + d)
    cent = rng.randn(40, d)
    Y = (cent[rng.randint(40, size=n)] + 0.5 * rng.randn(n, d)).astype(np.float32)
    Y[123] = Y[77]                                   # exact duplicates: ties, lower row first
    Y[n - 1] = Y[77]
    X = (cent[rng.randint(40, size=nq)] + 0.5 * rng.randn(nq, d)).astype(np.float32)
    X[3] = Y[77]                                     # a query ON the duplicated vector
    got = _index(Y).knn_brute(X, k)
    part = _numpy_part(X[:nq - nq % 100 or nq], Y)   # whole chunks: the FMA-chain shape
    for i in range(len(part)):
        order = np.lexsort((np.arange(n), part[i]))[:k]      # ascending (part, row)
        np.testing.assert_array_equal(got[i], order, err_msg=f"query {i}")


def test_knn_brute_recall_of_the_index_itself():
    """the use it is built for: Recall10@10 of IVF.query_batch against it"""
    from tinyknn_amd import IVF, FastPQ
    rng = np.random.RandomState(2)
    cent = rng.randn(100, 50)
    X = (cent[rng.randint(100, size=30000)] + 0.4 * rng.randn(30000, 50)).astype(np.float32)
    qs = (cent[rng.randint(100, size=500)] + 0.4 * rng.randn(500, 50)).astype(np.float32)
    ivf = IVF("euclidean", 170, FastPQ(2))
    ivf.fit(X[:10000]).build(X, n_probes=1)
    truth = ivf.device_index().knn_brute(qs, 10)
    got = ivf.query_batch(qs, 10, n_probes=170)      # every list probed, pass_1 = 1711 candidates
    recall = np.mean([len(set(a) & set(b)) / 10 for a, b in zip(truth, got)])
    assert recall > 0.9, recall


# ---- the paths beyond one segment, the candidate cap and large k -------------------------------------------------
def _clustered(rng, n, d, n_cent=40, spread=0.5, shift=0.0):
    cent = rng.randn(n_cent, d)
    return (cent[rng.randint(n_cent, size=n)] + spread * rng.randn(n, d) + shift).astype(np.float32), cent


_INT_INDEX = {}


def _int_case(d):
    """N = 2 300 017 rows (three segments of 2^20 at k = 10, the last one partial and not a multiple of 32) with
    integer coordinates in [-50, 50]: every norm, product sum and part is an integer below 2^24, so float32
    gives it exactly in any order of summation and the int64 reference is exact.  The same row is planted in
    all three segments."""
    if d not in _INT_INDEX:
        n = 2300017
        rng = np.random.RandomState(1000 + d)
        Y = rng.randint(-50, 51, size=(n, d)).astype(np.float32)
        r, r2 = 4321, 77777
        Y[(1 << 20) + r] = Y[r]
        Y[(1 << 21) + r2] = Y[r]
        _INT_INDEX.clear()                      # one index of this size at a time
        _INT_INDEX[d] = (Y, (r, (1 << 20) + r, (1 << 21) + r2), _index(Y))
    return _INT_INDEX[d]


@pytest.mark.parametrize("d,nq", [(16, 200), (16, 3), (8, 200), (8, 3)])
def test_several_segments_against_exact_integers(d, nq):
    """B1: ids == lexsort((row, part)) of the exact int64 part values; ties (there are many) go to the lower row
    across segment boundaries; nq = 3 takes the split of Y's rows over gridDim.y."""
    k = 10
    Y, planted, dev = _int_case(d)
    n = len(Y)
    assert segment_rows(k, n) == 1 << 20 and n % 32 != 0 and -(-n // (1 << 20)) == 3
    rng = np.random.RandomState(nq + d)
    X = rng.randint(-50, 51, size=(nq, d)).astype(np.float32)
    X[1] = Y[planted[0]]                        # part = 0 in three segments
    X[2] = Y[n - 1]                             # the last row of the partial segment
    got = dev.knn_brute(X, k)
    most = 0
    for c in range(0, nq, 10):
        part = int_part(X[c:c + 10], Y)
        assert part.max() < 1 << 24 and np.abs(part).max() < 1 << 24
        for i in range(len(part)):
            # the inputs cannot trip the cap legitimately: fewer than CAP rows within tau in every segment
            counts = within_tau_per_segment(part[i], k)
            assert len(counts) == 3 and max(counts) < CAP, (c + i, counts)
            most = max(most, max(counts))
            np.testing.assert_array_equal(got[c + i], k_best(part[i], k), err_msg=f"query {c + i}")
    print(f"d={d} nq={nq}: at most {most} rows within tau in one segment")
    np.testing.assert_array_equal(got[1][:3], planted)


@pytest.mark.parametrize("n,d,k", [(1200000, 16, 100), (300000, 16, 1024), (1024, 16, 1024), (700, 20, 700)])
def test_large_k_matches_numpy(n, d, k):
    """B2: k up to the documented 1024 = min(1024, N), at sizes where a segment of 2^20 rows holds far more than
    8192 rows within the sampled tau (k = 100 at N = 1.2 M: about 15 800), and k = ns = N."""
    rng = np.random.RandomState(n + k)
    Y, cent = _clustered(rng, n, d)
    Y[123] = Y[77]
    Y[n - 1] = Y[77]
    nq = 100
    X = (cent[rng.randint(40, size=nq)] + 0.5 * rng.randn(nq, d)).astype(np.float32)
    X[3] = Y[77]
    got = _index(Y).knn_brute(X, k)
    part = numpy_part(X, Y)
    for i in range(nq):
        np.testing.assert_array_equal(got[i], k_best(part[i], k), err_msg=f"query {i}")


@pytest.mark.parametrize("n", [8191, 8192, 8193])
@pytest.mark.parametrize("d", [1, 2, 127])
def test_sample_boundary_small_and_odd_d_one_query(n, d):
    """B3: N around ns = 8192 (the sampling stride becomes 1: below it the sample IS the matrix), d = 1, 2 and the
    odd 127 (a zero operand in the last MFMA step), one query."""
    rng = np.random.RandomState(n + d)
    Y, cent = _clustered(rng, n, d)
    Y[123] = Y[77]
    Y[n - 1] = Y[77]
    dev = _index(Y)
    for x in (Y[77:78].copy(), (cent[:1] + 0.5 * rng.randn(1, d)).astype(np.float32)):
        part = numpy_part(pad_chunk(x, rng), Y)[0]
        for k in (1, 10):
            np.testing.assert_array_equal(dev.knn_brute(x, k)[0], k_best(part, k))


def test_negative_part_values_keep_their_order():
    """B4: far from the origin `part` is the small difference of two numbers near 3.2e7 whose float32 spacing is 2
    to 4: for a query on or next to rows it comes out as ..., -4, -2, 0, 2, ... and the order-preserving key has
    to rank the negative ones first and by value."""
    n, d, nq, k = 20000, 16, 100, 10
    rng = np.random.RandomState(4)
    Y, _ = _clustered(rng, n, d, shift=1000.0)
    at = rng.choice(n - 40, size=nq, replace=False)
    for a in at:                                    # 12 rows within 1e-3 of each other around every query
        Y[a + 1:a + 12] = Y[a] + (1e-3 * rng.randn(11, d)).astype(np.float32)
    X = Y[at].copy()
    X[nq // 2:] += (1e-3 * rng.randn(nq - nq // 2, d)).astype(np.float32)      # half on a row, half next to one
    part = numpy_part(X, Y)
    want = np.stack([k_best(part[i], k) for i in range(nq)])
    best = np.take_along_axis(part, want, axis=1)
    # not vacuous: negative values among the k best, several distinct ones within one query, beside positive ones
    assert (best < 0).any(axis=1).sum() >= nq // 2
    assert any(len(np.unique(b[b < 0])) >= 2 and (b > 0).any() for b in best)
    np.testing.assert_array_equal(_index(Y).knn_brute(X, k), want)


def test_tau_tightens_between_segments():
    """The k-th distance found in one segment bounds what the next one appends.  Query 0 has 12 rows within
    distance^2 12 in the first segment, none of them sampled, and 9000 rows at distance^2 900 in the second, of
    which the sample holds more than k: the sampled tau is 900 and lets all 9000 in, the tightened one none."""
    k, d = 10, 8
    n = (1 << 20) + 40000
    assert segment_rows(k, n) == 1 << 20
    stride = n // 8192
    rng = np.random.RandomState(6)
    Y = rng.randint(-50, 51, size=(n, d)).astype(np.float32)
    X = rng.randint(-50, 51, size=(4, d)).astype(np.float32)
    X[0] = 200.0                                                     # far from the background rows
    close = 1000 * stride + 1 + np.arange(12)                        # no multiple of the stride among them
    assert (close % stride != 0).all()
    Y[close] = X[0]
    Y[close, np.arange(12) % d] += 1 + np.arange(12) // d            # distance^2 1 (8 rows) and 4 (4 rows)
    Y[(1 << 20) + 100:(1 << 20) + 9100] = X[0]
    Y[(1 << 20) + 100:(1 << 20) + 9100, 0] += 30                     # distance^2 900
    part = int_part(X, Y)
    sample = part[0][np.arange(8192) * stride]
    tau0 = np.partition(sample, k - 1)[k - 1]
    assert tau0 == 900 and (part[0][1 << 20:] <= tau0).sum() >= 9000 > CAP
    counts = within_tau_per_segment(part[0], k)
    assert counts[0] == 12 and counts[1] == 0, counts
    got = _index(Y).knn_brute(X, k)
    for i in range(len(X)):
        np.testing.assert_array_equal(got[i], k_best(part[i], k), err_msg=f"query {i}")


def test_candidate_cap_is_loud():
    """B5: 9000 identical rows in one segment and a query on them: more rows tied within tau than a list holds.
    The call may answer (the ten lowest of those rows) or refuse with an error; it never returns other ids, and
    the index answers the next call."""
    from tinyknn_amd._lib import TinyKnnHipError
    n, d, k = 20000, 16, 10
    rng = np.random.RandomState(8)
    Y, cent = _clustered(rng, n, d)
    Y[5000:14000] = Y[5000] + 20.0                  # far from every other row and query
    dev = _index(Y)
    X = (cent[rng.randint(40, size=100)] + 0.5 * rng.randn(100, d)).astype(np.float32)
    part = numpy_part(X, Y)
    assert max(max(within_tau_per_segment(part[i], k)) for i in range(100)) < CAP
    Xon = X.copy()
    Xon[7] = Y[5000]
    assert within_tau_per_segment(numpy_part(Xon, Y)[7], k)[0] >= 9000
    try:
        got = dev.knn_brute(Xon, k)
    except TinyKnnHipError as e:
        print("refused:", e)
        assert "overflow" in str(e)
    else:
        print("answered")
        np.testing.assert_array_equal(got[7], np.arange(5000, 5010))
        for i in (0, 1, 99):
            np.testing.assert_array_equal(got[i], k_best(part[i], k))
    got = dev.knn_brute(X, k)                       # no query on the tied rows: an ordinary call
    for i in range(100):
        np.testing.assert_array_equal(got[i], k_best(part[i], k), err_msg=f"query {i}")
