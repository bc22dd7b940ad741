"""The oracle's distance tables against the reference's own, beyond the widths FastPQ.fit produces (the g5 fixture
stops at dims_per_block 4 and M = 52): tests/golden/g5w_tables_m<M>_b<dims_per_block>.npz hold what the unmodified
reference's distance_table and udistance_table returned (tests/golden/make_golden.py: make_wide_tables) for a
hand-set codebook and float32 / float64 queries, some scaled by 0.05 — transformed tables, shift and scale, compared
with oracle.distance_table bit for bit.

  dims_per_block 8 / 16 / 32: einsum's four-vector group loop (from 16 floats / 8 doubles on), and in the unsigned
    table numpy's pairwise leaf (from 8 elements on `.sum(axis=-1)` runs 8 accumulators, not a sequential sum)
  M around 256, and 472 / 474 / 512: the mean's pairwise tree at 4096+ entries (the widths where tables.hip changes
    path and where a float64 table leaves 64 KiB of LDS), C- and F-ordered centres (dims_per_block 2 / 1)

The GPU tests compare tables.hip with the oracle at these same shapes (test_hip_parity.py::
test_distance_tables_vs_oracle): this test is what makes the oracle a reference there."""
import numpy as np
import pytest

from conftest import golden

WIDE = [(M, dpb) for dpb in (8, 16, 32) for M in (4, 12, 36)]
MANY = [(M, dpb) for dpb in (1, 2) for M in (256, 258, 260, 472, 474, 512)]


@pytest.mark.parametrize("signed", [True, False], ids=["signed", "unsigned"])
@pytest.mark.parametrize("is64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("M,dpb", WIDE + MANY)
def test_oracle_table_equals_the_references(oracle, M, dpb, is64, signed):
    g = golden("g5w_tables_m%d_b%d.npz" % (M, dpb))
    centers = g["centers"]
    assert centers.shape == (16, M * dpb) and centers.dtype == np.float32 and int(g["f_order"]) == int(dpb == 1)
    if int(g["f_order"]):               # dims_per_block 1: the view FastPQ.fit leaves is F-ordered
        centers = np.asfortranarray(centers)
    tag, sign = "f64" if is64 else "f32", "s" if signed else "u"
    qs = g["qs_" + tag]
    want_t, want_shift, want_scale = g["tables_%s_%s" % (sign, tag)], g["shift_%s_%s" % (sign, tag)], g["scale_%s_%s" % (sign, tag)]
    assert qs.dtype == (np.float64 if is64 else np.float32) and len(qs) == (25 if M < 256 else 8)
    assert want_shift.dtype == qs.dtype and want_scale.dtype == np.float64 and want_t.shape == (len(qs), 2 * M)
    for qi, q in enumerate(qs):
        t, shift, scale = oracle.distance_table(centers, dpb, q, float(g["sqrt_n_blocks"]), signed)
        assert shift.dtype == qs.dtype
        assert shift == want_shift[qi] and scale == want_scale[qi], (qi, shift, want_shift[qi], scale, want_scale[qi])
        np.testing.assert_array_equal(oracle.transform_tables(t), want_t[qi], err_msg=f"query {qi}")
