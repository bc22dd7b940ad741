"""The value columns and ranges the exact search inside a value range is tested on (tests/test_between_exact_gpu.py;
tests/test_between_exact_cpu.py holds the span model against the range formulas on every one of them).  Plain NumPy.
A fixture: dict(name, values (N,) or (N, C) in their own dtype, between = (lo, hi), each None or an array with one row
of bounds per query, nq).  Integer columns say "this end is not bounded" per query by the int64 extreme, floating ones
by -inf / +inf."""
import numpy as np

K = 10
MIN, MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
EDGE_LENGTHS = (0, 1, K - 1, K, K + 1, 255, 256, 257, 2047, 2049)


def _fixture(name, values, lo, hi):
    lo = None if lo is None else np.asarray(lo)
    hi = None if hi is None else np.asarray(hi)
    nq = len(lo) if lo is not None else len(hi)
    assert lo is None or hi is None or len(lo) == len(hi)
    return dict(name=name, values=values, between=(lo, hi), nq=nq)


def edges():
    """N = 8000, one int64 column of distinct values 3 * (a permutation): a window of any length can be cut exactly.
    Three windows of every length in EDGE_LENGTHS (length 0: between two keys), then windows whose ends lie between
    keys (length 5).  -> (fixture, the lengths)"""
    rng = np.random.RandomState(70)
    n = 8000
    values = 3 * rng.permutation(n).astype(np.int64)
    lo, hi, lengths = [], [], []
    for rep in range(3):
        for L in EDGE_LENGTHS:
            a = int(rng.randint(0, n - L)) if rep else (0 if L % 2 else n - max(L, 1))
            if L == 0:
                lo.append(3 * a + 1), hi.append(3 * a + 2)
            else:
                lo.append(3 * a), hi.append(3 * (a + L - 1))
            lengths.append(L)
    for a in (100, 4000):
        lo.append(3 * a - 1), hi.append(3 * (a + 4) + 1), lengths.append(5)
    return _fixture("edges", values, np.array(lo, dtype=np.int64), np.array(hi, dtype=np.int64)), np.array(lengths)


def everything():
    """N = 6000, one int64 column, every query's window holds all the rows"""
    rng = np.random.RandomState(71)
    values = rng.randint(0, 1000, size=6000).astype(np.int64)
    return _fixture("everything", values, np.zeros(6, dtype=np.int64), np.full(6, 999, dtype=np.int64))


DUP_VALUE, DUP_ROWS = 50, 300


def dups():
    """N = 3000, an int32 column in [0, 100) where DUP_ROWS rows spread over the ids carry DUP_VALUE: ends on a key
    many rows carry (lower against upper bound), lo == hi, windows below / above every value and straddling either
    end, lo > hi, an end left open"""
    rng = np.random.RandomState(72)
    n = 3000
    values = rng.randint(0, 99, size=n).astype(np.int32)
    values[values >= DUP_VALUE] += 1
    values[rng.choice(n, size=DUP_ROWS, replace=False)] = DUP_VALUE
    pairs = [(50, 50), (50, 60), (40, 50), (50, MAX), (MIN, 50), (51, 60), (40, 49), (-100, -1), (100, 1000),
             (-100, 3), (97, 1000), (60, 40), (51, 50), (0, 99), (7, 7)]
    lo = np.array([p[0] for p in pairs], dtype=np.int64)
    hi = np.array([p[1] for p in pairs], dtype=np.int64)
    return [_fixture("dups", values, lo, hi),
            _fixture("dups_lo_only", values, lo[[0, 1, 5, 7, 8]], None),
            _fixture("dups_hi_only", values, None, hi[[0, 2, 6, 7, 8]]),
            # a floating bound on an integer column: lo is ceil'ed, hi floor'ed
            _fixture("dups_float_bounds", values, np.array([49.5, 50.0, 49.01, 50.5, -np.inf, 1e30, -0.5]),
                     np.array([50.5, 50.0, 50.99, 50.75, 49.99, np.inf, 0.5]))]


def extremes():
    """N = 2000, an int64 column with rows at -2**63 and 2**63 - 1 (and beside them): bounded and open ends there"""
    rng = np.random.RandomState(73)
    n = 2000
    values = rng.randint(-2**62, 2**62, size=n).astype(np.int64)
    at = rng.permutation(n)
    values[at[:20]], values[at[20:40]] = MIN, MAX
    values[at[40:45]], values[at[45:50]] = MIN + 1, MAX - 1
    pairs = [(MIN, MIN), (MAX, MAX), (MIN, MIN + 1), (MAX - 1, MAX), (MIN + 1, MIN + 1), (MIN, 0), (0, MAX),
             (MIN, MAX), (MIN + 1, MAX - 1), (MAX, MIN)]
    return _fixture("extremes", values, np.array([p[0] for p in pairs], dtype=np.int64),
                    np.array([p[1] for p in pairs], dtype=np.int64))


def floats():
    """N = 2500, two float32 columns; column 0 holds -0.0 / +0.0, negative values and +-inf beside random ones"""
    rng = np.random.RandomState(74)
    n = 2500
    values = rng.randn(n, 2).astype(np.float32)
    special = np.array([-np.inf, -2.5, -1.0, -0.0, 0.0, 1.0, 2.5, np.inf], dtype=np.float32)
    at = rng.permutation(n)[:800]
    values[at, 0] = special[rng.randint(0, len(special), size=len(at))]
    inf = np.inf
    pairs0 = [(-0.0, 0.0), (0.0, -0.0), (-inf, -1.0), (-inf, -inf), (inf, inf), (1.0, inf), (-1.5, 1.5), (-inf, inf),
              (-inf, inf), (2.5, -2.5), (-2.5, -2.5)]
    pairs1 = [(-inf, inf)] * 7 + [(-inf, inf), (-0.5, 0.5), (-inf, inf), (-1.0, inf)]
    lo = np.array([[a[0], b[0]] for a, b in zip(pairs0, pairs1)], dtype=np.float32)
    hi = np.array([[a[1], b[1]] for a, b in zip(pairs0, pairs1)], dtype=np.float32)
    return [_fixture("floats", values, lo, hi),
            # integer bounds on floating columns
            _fixture("floats_int_bounds", values, np.array([[-1, -3], [0, -1], [1, 0]], dtype=np.int64),
                     np.array([[1, 3], [0, 1], [2, 0]], dtype=np.int64))]


def narrow_dtypes():
    """a float16 column and a uint64 column (N = 2000 each)"""
    rng = np.random.RandomState(75)
    n = 2000
    h = rng.randn(n).astype(np.float16)
    h[::97] = np.float16(-0.0)
    lo = np.array([-0.25, 0.0, 1.0, -np.inf, 3.0, h[5]], dtype=np.float16)
    hi = np.array([0.25, 0.0, np.inf, -1.0, 2.0, h[5]], dtype=np.float16)
    u = rng.randint(0, 2**62, size=n).astype(np.uint64) * np.uint64(2)
    u[::50], u[1::50] = 0, 2**63 - 1
    ulo = np.array([0, 2**62, 2**63 - 1, 1, 2**63 - 2], dtype=np.uint64)
    uhi = np.array([0, 2**63 - 1, 2**63 - 1, 2**61, 2**63 - 2], dtype=np.uint64)
    return [_fixture("float16", h, lo, hi), _fixture("uint64", u, ulo, uhi)]


WIDTHS = (10, 100, 1000, 4000)      # distinct values of column c: column 0 is the wide one, column 3 the narrow one


def columns(C):
    """N = 4000, C int64 columns of WIDTHS[c] distinct values: every query bounds a random subset of the columns (the
    others at the extremes), the last one none"""
    rng = np.random.RandomState(76 + C)
    n, nq = 4000, 40
    values = np.stack([rng.randint(0, WIDTHS[c], size=n) for c in range(C)], axis=1).astype(np.int64)
    lo = np.full((nq, C), MIN, dtype=np.int64)
    hi = np.full((nq, C), MAX, dtype=np.int64)
    for i in range(nq - 1):
        chosen = np.flatnonzero(rng.rand(C) < 0.6)
        if i < C:
            chosen = np.array([i])              # every column is some query's only one
        elif not len(chosen):
            chosen = np.array([i % C])
        for c in chosen:
            a = rng.randint(0, WIDTHS[c])
            w = rng.randint(0, max(1, WIDTHS[c] // 4))
            if rng.rand() < 0.3:
                lo[i, c] = a                    # one end only
            elif rng.rand() < 0.3:
                hi[i, c] = a
            else:
                lo[i, c], hi[i, c] = a, a + w
    return _fixture(f"columns{C}", values[:, 0] if C == 1 else values, lo[:, 0] if C == 1 else lo,
                    hi[:, 0] if C == 1 else hi)


def wide_and_narrow(narrow):
    """N = 4000, two int64 columns, one of 8 distinct values and one of 2000; column `narrow` is the narrow one.  Both
    are bounded by every query: the span is the narrow column's.  The two fixtures hold the same rows and ranges with
    the columns swapped."""
    rng = np.random.RandomState(90)
    n, nq = 4000, 24
    wide = rng.randint(0, 8, size=n).astype(np.int64)
    thin = rng.randint(0, 2000, size=n).astype(np.int64)
    wlo = rng.randint(0, 4, size=nq).astype(np.int64)
    whi = wlo + rng.randint(2, 5, size=nq)
    tlo = rng.randint(0, 1900, size=nq).astype(np.int64)
    thi = tlo + rng.randint(0, 120, size=nq)
    cols = [(wide, wlo, whi), (thin, tlo, thi)]
    if narrow == 0:
        cols.reverse()
    return _fixture(f"narrow{narrow}", np.stack([c[0] for c in cols], axis=1), np.stack([c[1] for c in cols], axis=1),
                    np.stack([c[2] for c in cols], axis=1))


def ties():
    """N = 3000, three int64 columns of which 1 and 2 are equal, and every query bounds both alike (column 0 open, or
    bounded and wider): equal lengths, so the span is column 1's"""
    rng = np.random.RandomState(91)
    n, nq = 3000, 12
    v = rng.randint(0, 500, size=n).astype(np.int64)
    values = np.stack([rng.randint(0, 5, size=n).astype(np.int64), v, v], axis=1)
    a = rng.randint(0, 450, size=nq).astype(np.int64)
    b = a + rng.randint(0, 50, size=nq)
    lo = np.stack([np.full(nq, MIN), a, a], axis=1)
    hi = np.stack([np.full(nq, MAX), b, b], axis=1)
    lo[::2, 0], hi[::2, 0] = 0, 4               # (column 0 bounded too, and wider)
    return _fixture("ties", values, lo, hi)


def all_fixtures():
    """every fixture above, the GPU tests' list"""
    return ([edges()[0], everything()] + dups() + [extremes()] + floats() + narrow_dtypes() +
            [columns(C) for C in (1, 2, 3, 4)] + [wide_and_narrow(0), wide_and_narrow(1), ties()])
