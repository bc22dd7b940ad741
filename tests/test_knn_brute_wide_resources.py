"""knn_brute(wide=True)'s tile kernel as the compiler reports it (no GPU needed): all four instances of
brute_wide_tiles_kernel<MODE, RESTRICTED> compile for gfx950 with no scratch, no vector register spilled, the static
LDS DESIGN §3.25 states — 34 816 bytes, and 45 056 with the queries' attributes behind the slabs — and two workgroups a
CU."""
import pytest

from kernel_usage import have_hipcc, kernel_usage


def test_no_scratch_the_stated_lds_and_two_workgroups_a_cu():
    if not have_hipcc():
        pytest.skip("hipcc not found")
    hits = {k: v for k, v in kernel_usage("brute_wide.hip").items() if "brute_wide_tiles_kernel" in k}
    assert len(hits) == 4, sorted(kernel_usage("brute_wide.hip"))
    assert sorted(u["LDS Size"] for u in hits.values()) == [34816, 34816, 45056, 45056], hits
    for name, u in hits.items():
        assert u.get("ScratchSize") == 0 and u.get("VGPRs Spill", 0) == 0 and u["Occupancy"] >= 2, (name, u)
