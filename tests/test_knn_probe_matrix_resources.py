"""knn_probe(matrix=True)'s distance kernel as the compiler reports it (no GPU needed): it compiles for gfx950 with no
scratch, no vector register spilled and the static LDS DESIGN §3.22 states — 64 000 bytes, within the 64 KiB a workgroup
gets without asking, two workgroups a CU."""
import pytest

from kernel_usage import have_hipcc, kernel_usage


def test_no_scratch_and_the_stated_lds():
    if not have_hipcc():
        pytest.skip("hipcc not found")
    hits = {k: v for k, v in kernel_usage("probe_matrix.hip").items() if "probe_dist_matrix_kernel" in k}
    assert len(hits) == 1, sorted(kernel_usage("probe_matrix.hip"))
    (u,) = hits.values()
    assert u.get("ScratchSize") == 0 and u.get("VGPRs Spill", 0) == 0, u
    assert u["LDS Size"] == 64000 and u["Occupancy"] >= 2, u
