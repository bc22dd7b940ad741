"""References for the device front end (tk_index_prepare_dev: normalise_rows_kernel, pad_rows_kernel,
rotate_rows_kernel in build.hip), plain NumPy / Python, no GPU.  tests/test_fast_front_end_gpu.py compares the kernels
with them; tests/test_fast_front_end_cpu.py checks the references themselves."""
import math
from fractions import Fraction

import numpy as np

U32 = 2.0 ** -24          # unit roundoff of float32
U64 = 2.0 ** -53          # unit roundoff of float64


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def front_rows(nq, d, seed):
    """(nq, d) float32 raw queries.  By row index modulo 9: 0-3 ordinary (normal entries, a log-normal scale per
    row), 4 scaled by 1e-22 (the squares are denormal or underflow to 0), 5 scaled by 1e18 (the sum of squares is
    near the largest float32 and overflows for some rows), 8 scaled by 1e20 (every square overflows: the row
    becomes 0), 6 all zero (0/0 = nan), 7 one non-zero element."""
    rng = np.random.RandomState(seed)
    X = (rng.randn(nq, d) * rng.lognormal(size=(nq, 1))).astype(np.float32)
    kind = np.arange(nq) % 9
    X[kind == 4] *= np.float32(1e-22)
    X[kind == 5] *= np.float32(1e18)
    X[kind == 8] *= np.float32(1e20)
    X[kind == 6] = 0
    one = np.flatnonzero(kind == 7)
    keep = X[one, one % d].copy()
    X[one] = 0
    X[one, one % d] = np.where(keep == 0, np.float32(1.5), keep)
    return X


def ordinary(nq):
    """the rows of front_rows that are ordinary"""
    return np.flatnonzero(np.arange(nq) % 9 < 4)


def normalise_rows(X):
    """The order normalise_rows_kernel states, in float32, every operation rounded by itself (NumPy's float32
    array operations are the IEEE ones, element by element, so the rows go side by side): products first; d < 8
    one running sum; otherwise 8 accumulators over t < d - d % 8, combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)),
    then the remainder added serially; sqrtf; one division per element."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    n, d = X.shape
    with np.errstate(all="ignore"):
        P = X * X
        assert P.dtype == np.float32
        if d < 8:
            res = np.zeros(n, np.float32)
            for t in range(d):
                res = res + P[:, t]
        else:
            r = [P[:, j].copy() for j in range(8)]
            t = 8
            while t < d - d % 8:
                for j in range(8):
                    r[j] = r[j] + P[:, t + j]
                t += 8
            res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
            while t < d:
                res = res + P[:, t]
                t += 1
        nr = np.sqrt(res)
        assert nr.dtype == np.float32
        return X / nr[:, None]


def normalise_rows_f64(X):
    X64 = np.asarray(X, dtype=np.float64)
    return X64 / np.sqrt((X64 * X64).sum(axis=1, keepdims=True))


def normalise_bound(d):
    """Relative error of one element of normalise_rows against the exact x / sqrt(sum x^2), from the depth of the
    summation alone (no overflow or underflow: ordinary rows).  All terms of the sum are >= 0, so a term that passes
    through m roundings on its way into the sum carries a factor within (1 +- u)^m and so does the sum:
      1 rounding of the product, ceil(d / 8) - 1 additions in its accumulator, 3 combining additions, up to 7
      additions of the remainder                                  m = 1 + (ceil(d/8) - 1) + 3 + 7
    (for d < 8 the single running sum has at most 1 + 6 <= m).  The square root halves the relative error of its
    argument, 1 / sqrt(1 - gamma_m) - 1 with gamma_m = m u / (1 - m u), and sqrtf and the division round once each:
      (1 + u)^2 / sqrt(1 - gamma_m) - 1,
    to which the float64 reference adds its own (d + 3) roundings of 2^-53."""
    m = 1 + (math.ceil(d / 8) - 1) + 3 + 7
    gamma = m * U32 / (1 - m * U32)
    return (1 + U32) ** 2 / math.sqrt(1 - gamma) - 1 + (d + 3) * U64


def pad_rows(X, dq):
    out = np.zeros((X.shape[0], dq), np.float32)
    out[:, :X.shape[1]] = X
    return out


def fma_exact(a, b, c):
    """one correctly rounded float64 fma(a, b, c): exact rational arithmetic, then one rounding (float() of a
    Fraction rounds to nearest, ties to even)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def rotate_rows_fma(X, R, d_pad):
    """rotate_rows_kernel's sum: acc = fma((double) x[t], R[j][t], acc) for t ascending over d_pad (x padded with
    zeros), starting from 0.  X (n, d) float32 finite, R (dq, d_pad) float64 -> (n, dq) float64."""
    n, d = X.shape
    out = np.empty((n, R.shape[0]), np.float64)
    for i in range(n):
        x = [Fraction(float(v)) for v in X[i]] + [Fraction(0)] * (d_pad - d)
        for j in range(R.shape[0]):
            acc = 0.0
            row = R[j]
            for t in range(d_pad):
                acc = float(x[t] * Fraction(float(row[t])) + Fraction(acc))
            out[i, j] = acc
    return out


def rotation_bound(X, R, d_pad):
    """|fma chain - exact sum| <= gamma_n * sum_t |x_t R_jt| for n = d_pad terms of one rounding each
    (u = 2^-53, gamma_n = n u / (1 - n u)): (n, dq) float64."""
    Xp = np.zeros((X.shape[0], d_pad), np.float64)
    Xp[:, :X.shape[1]] = X
    gamma = d_pad * U64 / (1 - d_pad * U64)
    return gamma * (np.abs(Xp) @ np.abs(R).T)


def rotate_rows_f64(X, R, d_pad):
    Xp = np.zeros((X.shape[0], d_pad), np.float64)
    Xp[:, :X.shape[1]] = X
    return Xp @ R.T


def ulp_distance32(a, b):
    """distance in float32 ulps between finite arrays (ordered-integer view)"""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def ulp_distance64(a, b):
    """|a - b| in units of the float64 spacing at |b| (b: the value measured against)"""
    return np.abs(np.asarray(a, np.float64) - b) / np.spacing(np.abs(b))
