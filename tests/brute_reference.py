"""References for tests/test_brute_gpu.py (tk_index_knn_brute), plain NumPy, no GPU.
tests/test_brute_reference_cpu.py checks them against slower, more obvious forms."""
import numpy as np

NS = 8192            # rows in the strided sample that gives the first tau (api_build.hip)
CAP = 8192           # candidates a query's list holds (api_build.hip)


def segment_rows(k, n):
    """Rows per segment of the selection pass, the rule stated in brute.hip's header: the largest power of two
    with k * seg / ns <= CAP / 4, at most 2^20 (ns = min(n, NS))."""
    most = CAP * min(n, NS) // (4 * k)
    seg = 32
    while seg < (1 << 20) and 2 * seg <= most:
        seg *= 2
    return seg


def k_best(part_row, k):
    """lexsort((row, part))[:k] without sorting the whole row: only rows within the k-th smallest value can be
    among the first k, and flatnonzero lists them by ascending row, which a stable sort by value keeps."""
    kth = np.partition(part_row, k - 1)[k - 1]
    rows = np.flatnonzero(part_row <= kth)
    return rows[np.argsort(part_row[rows], kind="stable")][:k]


def numpy_part(X, Y, block=1 << 18):
    """knn_brute's `part` (utils.py:84) in float32 for up to 100 rows of X (one chunk of the reference, the GEMM
    shape whose sums are FMA chains over ascending k), the columns taken in blocks of at least `block` rows of Y
    so that a chunk against a million rows fits in memory.  A block changes which rows of Y a GEMM call sees, not
    how one dot product is summed, as long as it is not tiny: a last block of a few rows goes through another
    BLAS routine (one row is a GEMV) with other bits, so a shorter remainder is joined to the block before it
    (test_brute_reference_cpu.py compares the result with the unblocked product)."""
    assert len(X) <= 100 and X.dtype == Y.dtype == np.float32
    xn = np.einsum("ij,ij->i", X, X)
    out = np.empty((len(X), len(Y)), np.float32)
    edges = list(range(0, len(Y), block))[:max(1, len(Y) // block)] + [len(Y)]
    for j, e in zip(edges[:-1], edges[1:]):
        yn = np.einsum("ij,ij->i", Y[j:e], Y[j:e])
        out[:, j:e] = xn[:, None] + yn[None] - 2 * X @ Y[j:e].T
    return out


def pad_chunk(X, rng):
    """X below 100 rows made a whole chunk of 100 (rows of noise appended): numpy multiplies a short chunk through
    another BLAS routine (a 1-row X is a GEMV), whose order of summation is not the FMA chain."""
    if len(X) >= 100:
        return X
    return np.vstack([X, rng.randn(100 - len(X), X.shape[1]).astype(np.float32)])


def int_part(X, Y):
    """`part` for integer-valued coordinates, exactly, in int64: (|x|^2 + |y|^2) - 2 x.y.  No BLAS (numpy
    multiplies integer matrices with its own loops)."""
    Xi, Yi = X.astype(np.int64), Y.astype(np.int64)
    assert np.array_equal(Xi, X) and np.array_equal(Yi, Y)
    xn, yn = (Xi * Xi).sum(axis=1), (Yi * Yi).sum(axis=1)
    return xn[:, None] + yn[None] - 2 * (Xi @ Yi.T)


def within_tau_per_segment(part_row, k):
    """What the selection pass appends for one query, from the reference's part values alone: per segment the number
    of rows with part <= tau.  tau starts as the k-th smallest over the sampled rows i * (n // ns), i < ns, and
    after each segment becomes the k-th smallest of all rows seen so far once k of them lie within it."""
    n = len(part_row)
    ns = min(n, NS)
    seg = segment_rows(k, n)
    sample = part_row[np.arange(ns) * (n // ns)]
    tau = np.partition(sample, k - 1)[k - 1]
    counts = []
    for s0 in range(0, n, seg):
        end = min(n, s0 + seg)
        counts.append(int((part_row[s0:end] <= tau).sum()))
        if end >= k:
            kth = np.partition(part_row[:end], k - 1)[k - 1]
            if kth <= tau:
                tau = kth
    return counts
