"""radius_search(wide=True)'s tile kernel as the compiler reports it (no GPU needed): all six instances of
radius_wide_tiles_kernel<PASS, RESTRICTED> compile for gfx950 with no scratch, no vector register spilled, the static
LDS DESIGN §3.26 states — 34 816 bytes, and 45 056 with the queries' attributes behind the slabs — and two workgroups a
CU."""
import pytest

from kernel_usage import have_hipcc, kernel_usage


def test_no_scratch_the_stated_lds_and_two_workgroups_a_cu():
    if not have_hipcc():
        pytest.skip("hipcc not found")
    hits = {k: v for k, v in kernel_usage("radius_wide.hip").items() if "radius_wide_tiles_kernel" in k}
    assert len(hits) == 6, sorted(kernel_usage("radius_wide.hip"))
    assert sorted(u["LDS Size"] for u in hits.values()) == [34816] * 3 + [45056] * 3, hits
    for name, u in hits.items():
        assert u.get("ScratchSize") == 0 and u.get("VGPRs Spill", 0) == 0 and u["Occupancy"] >= 2, (name, u)
