"""The references of tests/test_fast_front_end_gpu.py (tests/front_reference.py) checked without a GPU: the restated
normalisation is NumPy's own, bit for bit; its derived error bound holds against float64; the exact FMA chain is a
correctly rounded one and stays within its bound of the float64 product."""
import math
from fractions import Fraction

import numpy as np

from front_reference import (bits32, bits64, fma_exact, front_rows, normalise_bound, normalise_rows,  # noqa: E402
                             normalise_rows_f64, ordinary, pad_rows, rotate_rows_f64, rotate_rows_fma, rotation_bound,
                             ulp_distance32, ulp_distance64)

NQS = (1, 128, 129, 1000)


def test_rows_hold_every_kind():
    X = front_rows(1000, 40, 1)
    with np.errstate(all="ignore"):
        sq = (X * X).sum(axis=1)
    assert X.dtype == np.float32 and np.isfinite(X).all()
    assert (sq[4::9] < 1e-37).all() and (sq[4::9] == 0).any()           # denormal or flushed squares
    assert np.isinf(sq[8::9]).all() and np.isinf(sq[5::9]).any() and np.isfinite(sq[5::9]).any()
    assert not X[6::9].any() and ((X[7::9] != 0).sum(axis=1) == 1).all()
    assert len(ordinary(1000)) > 400 and np.isfinite(sq[ordinary(1000)]).all() and (sq[ordinary(1000)] > 1e-6).all()


def test_restated_normalisation_is_numpys_bit_for_bit():
    """validates the GPU test's reference: for d <= 128 np.linalg.norm(axis=1) sums a row in one leaf of 8
    accumulators, the order normalise_rows restates"""
    for d in range(1, 129):
        for nq in NQS:
            X = front_rows(nq, d, 1000 * d + nq)
            with np.errstate(all="ignore"):
                want = X / np.linalg.norm(X, axis=1, keepdims=True)
            got = normalise_rows(X)
            assert want.dtype == got.dtype == np.float32
            assert np.array_equal(bits32(want), bits32(got)), (d, nq)
    got = normalise_rows(front_rows(129, 40, 5))
    assert np.isnan(got[6::9]).all() and not got[8::9].any()            # 0/0 and x/inf, as NumPy gives them
    assert (np.abs(got[7::9]).sum(axis=1) == 1).all()


def test_restated_normalisation_within_its_derived_bound_of_float64():
    worst = 0.0
    for d in range(1, 129):
        X = front_rows(1000, d, d)[ordinary(1000)]
        ref = normalise_rows_f64(X)
        err = np.abs(normalise_rows(X).astype(np.float64) - ref)
        assert (err <= normalise_bound(d) * np.abs(ref)).all(), d
        nz = ref != 0
        worst = max(worst, (err[nz] / np.abs(ref[nz])).max() / normalise_bound(d))
    assert 0.05 < worst <= 1          # a bound of the right order, not a loose one
    assert normalise_bound(128) < 16 * 2.0 ** -24


def test_a_wrong_order_is_not_the_reference():
    """the comparisons above can tell summation orders apart: a left-to-right sum, or one without the serial
    remainder, differs from normalise_rows on these inputs"""
    X = front_rows(1000, 100, 3)[ordinary(1000)]
    P = X * X
    serial = np.zeros(len(X), np.float32)
    for t in range(100):
        serial = serial + P[:, t]
    assert not np.array_equal(bits32(X / np.sqrt(serial)[:, None]), bits32(normalise_rows(X)))
    assert not np.array_equal(bits32(normalise_rows(X[:, :96])), bits32(normalise_rows(X)))


def test_padding():
    X = front_rows(10, 5, 0)
    P = pad_rows(X, 8)
    assert P.dtype == np.float32 and np.array_equal(bits32(P[:, :5]), bits32(X)) and not P[:, 5:].any()
    assert np.array_equal(bits32(pad_rows(X, 5)), bits32(X))


def test_fma_exact_rounds_once():
    # a product whose low half decides the rounding of the sum: multiply-then-add gets another value
    a, b = 1.0 + 2.0 ** -30, 1.0 + 2.0 ** -30
    c = -(1.0 + 2.0 ** -29)
    assert fma_exact(a, b, c) == 2.0 ** -60 and a * b + c == 0.0
    rng = np.random.RandomState(0)
    for _ in range(2000):
        a, b, c = rng.randn(3) * 10.0 ** rng.randint(-20, 20, size=3)
        exact = Fraction(a) * Fraction(b) + Fraction(c)
        got = fma_exact(a, b, c)
        # correctly rounded: no float64 is closer to the exact value
        for other in (np.nextafter(got, -np.inf), np.nextafter(got, np.inf)):
            assert abs(Fraction(got) - exact) <= abs(Fraction(float(other)) - exact)


def test_fma_chain_within_its_bound_and_not_the_unfused_sum():
    rng = np.random.RandomState(1)
    d, pad, rd = 20, 4, 16
    R = rng.randn(rd, d + pad)
    X = rng.randn(12, d).astype(np.float32)
    X[0] = 0
    X[1, ::2] = 1e-20
    X[1, 1::2] = 1e20
    got = rotate_rows_fma(X, R, d + pad)
    ref = rotate_rows_f64(X, R, d + pad)
    assert not got[0].any()
    assert (np.abs(got - ref) <= rotation_bound(X, R, d + pad)).all()
    assert ulp_distance64(got[2:], ref[2:]).max() < 64
    # multiply-then-add, and a chain that starts at t = 1, give other bits
    unfused = np.zeros_like(got)
    for t in range(d):
        unfused = unfused + X[:, t:t + 1].astype(np.float64) * R[None, :, t]
    assert not np.array_equal(bits64(unfused), bits64(got))
    assert not np.array_equal(bits64(rotate_rows_fma(X[:, 1:], R[:, 1:], d + pad - 1)), bits64(got))


def test_ulp_distances():
    one = np.float32(1)
    assert ulp_distance32(np.array([one]), np.array([np.nextafter(one, np.float32(2))]))[0] == 1
    assert ulp_distance32(np.array([-one]), np.array([one]))[0] == 2 * int(one.view(np.int32))
    assert ulp_distance32(np.array([np.float32(0)]), np.array([np.float32(-0.0)]))[0] == 0
    assert ulp_distance64(np.array([np.nextafter(1.0, 2.0)]), np.array([1.0]))[0] == 1
    assert math.isclose(ulp_distance64(np.array([1.0 + 2.0 ** -50]), np.array([1.0]))[0], 4)
