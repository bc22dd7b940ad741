"""The references of tests/test_brute_gpu.py (tests/brute_reference.py) against slower, more obvious forms of
themselves.  No GPU."""
import numpy as np
import pytest

from brute_reference import CAP, NS, int_part, k_best, numpy_part, pad_chunk, segment_rows, within_tau_per_segment  # noqa: E402


def test_k_best_is_the_head_of_the_lexsort():
    rng = np.random.RandomState(0)
    for n, k in ((1, 1), (50, 50), (3000, 10), (3000, 1024), (20000, 100)):
        for vals in (rng.randn(n).astype(np.float32), rng.randint(-3, 4, size=n).astype(np.int64),
                     np.zeros(n, np.float32)):
            np.testing.assert_array_equal(k_best(vals, k), np.lexsort((np.arange(n), vals))[:k])


def test_column_blocks_do_not_change_a_bit():
    """a remainder of one row (a GEMV by itself) or of a few rows is joined to the block before it"""
    rng = np.random.RandomState(1)
    for n, d, blocks in ((2 * (1 << 18) + 1, 16, (1 << 18,)), (70001, 16, (1 << 18, 10000, 7000)),
                         (9995, 127, (4096, 999)), (9000, 1, (4096,))):
        Y = rng.randn(n, d).astype(np.float32)
        X = rng.randn(100, d).astype(np.float32)
        whole = (np.einsum("ij,ij->i", X, X)[:, None] + np.einsum("ij,ij->i", Y, Y)[None] - 2 * X @ Y.T)
        assert whole.dtype == np.float32
        for block in blocks:
            assert np.array_equal(numpy_part(X, Y, block).view(np.uint32), whole.view(np.uint32)), (n, d, block)


def test_a_padded_chunk_keeps_its_first_rows():
    rng = np.random.RandomState(2)
    x = rng.randn(1, 20).astype(np.float32)
    p = pad_chunk(x, rng)
    assert p.shape == (100, 20) and np.array_equal(p[:1], x)
    big = rng.randn(100, 20).astype(np.float32)
    assert pad_chunk(big, rng) is big


def test_integer_parts_are_exact_in_float32_in_any_order():
    """the premise of the several-segment GPU test: for integer coordinates in [-50, 50] the float32 formula gives
    the int64 value whichever way it is summed"""
    rng = np.random.RandomState(3)
    for d in (8, 16):
        Y = rng.randint(-50, 51, size=(5000, d)).astype(np.float32)
        X = rng.randint(-50, 51, size=(100, d)).astype(np.float32)
        exact = int_part(X, Y)
        assert np.abs(exact).max() < 1 << 24
        brute = ((X.astype(np.int64)[:, None, :] - Y.astype(np.int64)[None, :, :]) ** 2).sum(axis=2)
        np.testing.assert_array_equal(exact, brute)
        np.testing.assert_array_equal(numpy_part(X, Y).astype(np.int64), exact)
        perm = rng.permutation(d)
        np.testing.assert_array_equal(numpy_part(X[:, perm].copy(), Y[:, perm].copy()).astype(np.int64), exact)
    with pytest.raises(AssertionError):
        int_part(np.full((1, 2), 0.5, np.float32), np.zeros((1, 2), np.float32))


def test_segment_rule():
    """brute.hip's header: 2^20 rows for k <= 16 (the launch sequence of small k), 2^17 for k = 100, 2^14 for
    k = 1024 with a full sample; the expected k * seg / ns appended rows stay within a quarter of the cap"""
    assert [segment_rows(k, 10 ** 7) for k in (1, 10, 16, 17, 100, 1024)] == [1 << 20, 1 << 20, 1 << 20, 1 << 19,
                                                                             1 << 17, 1 << 14]
    for n in (700, 8191, 8192, 300000, 10 ** 7):
        for k in (1, 10, 60, 100, 700, 1024):
            if k > n:
                continue
            seg = segment_rows(k, n)
            assert seg & (seg - 1) == 0 and 32 <= seg <= 1 << 20
            assert k * seg <= CAP // 4 * min(n, NS)
            assert seg == 1 << 20 or 2 * k * seg > CAP // 4 * min(n, NS)
            assert n > NS or seg >= n               # a matrix that is its own sample is one segment


def test_within_tau_simulation_against_a_row_by_row_walk():
    rng = np.random.RandomState(4)
    n, k = 40000, 700                                # segment_rows = 16384: three segments
    part = rng.randint(0, 5000, size=n).astype(np.int64)
    seg = segment_rows(k, n)
    assert seg < n
    tau = sorted(part[np.arange(NS) * (n // NS)])[k - 1]
    want, kept = [], []
    for s0 in range(0, n, seg):
        rows = [j for j in range(s0, min(n, s0 + seg)) if part[j] <= tau]
        want.append(len(rows))
        kept = sorted(kept + rows, key=lambda j: (part[j], j))[:k]      # the list after the cut
        if len(kept) >= k:
            tau = part[kept[k - 1]]
    assert within_tau_per_segment(part, k) == want
    assert sum(want) >= k
