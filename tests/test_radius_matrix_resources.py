"""radius_search(matrix=True)'s tile kernel as the compiler reports it (no GPU needed): all six instances of
radius_matrix_tiles_kernel<PASS, RESTRICTED> compile for gfx950 with no scratch, no vector register spilled, the static
LDS DESIGN §3.24 states — 55 296 bytes, and 65 536 with the queries' attributes behind the tiles — and two workgroups a
CU."""
import pytest

from kernel_usage import have_hipcc, kernel_usage


def test_no_scratch_the_stated_lds_and_two_workgroups_a_cu():
    if not have_hipcc():
        pytest.skip("hipcc not found")
    hits = {k: v for k, v in kernel_usage("radius_matrix.hip").items() if "radius_matrix_tiles_kernel" in k}
    assert len(hits) == 6, sorted(kernel_usage("radius_matrix.hip"))
    assert sorted(u["LDS Size"] for u in hits.values()) == [55296] * 3 + [65536] * 3, hits
    for name, u in hits.items():
        assert u.get("ScratchSize") == 0 and u.get("VGPRs Spill", 0) == 0 and u["Occupancy"] >= 2, (name, u)
