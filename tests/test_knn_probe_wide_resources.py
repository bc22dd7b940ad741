"""knn_probe's wide distance kernel as the compiler reports it (no GPU needed): its three instantiations compile for
gfx950 with no scratch and no vector register spilled, and their LDS — static, so it is part of the report, and the same
at every d — is at most the 64 KiB a workgroup gets without asking.  DESIGN §3.21 records the register counts."""
import pytest

from kernel_usage import have_hipcc, kernel_usage


@pytest.mark.parametrize("types", ["ff", "fDF16_", "dd"])
def test_no_scratch_and_lds_within_64_kib(types):
    if not have_hipcc():
        pytest.skip("hipcc not found")
    hits = {k: v for k, v in kernel_usage("probe_exact.hip").items() if f"probe_dist_wide_kernelI{types}E" in k}
    assert len(hits) == 1, sorted(kernel_usage("probe_exact.hip"))
    (u,) = hits.values()
    assert u.get("ScratchSize") == 0 and u.get("VGPRs Spill", 0) == 0, u
    assert 0 < u["LDS Size"] <= 64 * 1024, u
