"""knn_probe(wide=True)'s distance kernel as the compiler reports it (no GPU needed): the three forms of
probe_dist_f32_kernel<U> — a row staged in loads of 16 bytes, of 8 bytes and of floats — compile for gfx950 with no
scratch, no vector register spilled, the static LDS DESIGN §3.27 states (52 224 bytes) and two workgroups a CU."""
import pytest

from kernel_usage import have_hipcc, kernel_usage


def test_three_forms_no_scratch_the_stated_lds_and_two_workgroups_a_cu():
    if not have_hipcc():
        pytest.skip("hipcc not found")
    hits = {k: v for k, v in kernel_usage("probe_f32.hip").items() if "probe_dist_f32_kernel" in k}
    assert len(hits) == 3, sorted(kernel_usage("probe_f32.hip"))
    for name, u in hits.items():
        assert u.get("ScratchSize") == 0 and u.get("VGPRs Spill", 0) == 0, (name, u)
        assert u["LDS Size"] == 52224 and u["Occupancy"] >= 2, (name, u)
