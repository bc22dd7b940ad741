"""Register / scratch / LDS budget of the kernels of between.hip, read from the compiler as tests/test_kernel_resources.py
reads it (no GPU needed): no scratch, no spills, no static LDS, and the occupancy of the tag pass, whose geometry the
range pass has."""
import pytest

from kernel_usage import have_hipcc, kernel_usage


@pytest.fixture(scope="module")
def usage():
    if not have_hipcc():
        pytest.skip("hipcc not found")
    return kernel_usage("between.hip"), kernel_usage("tags.hip")


def test_the_kernels_of_between_hip(usage):
    between, _ = usage
    names = sorted(between)
    assert len([n for n in names if "value_table_kernel" in n]) == 1, names
    assert len([n for n in names if "between_pass_kernel" in n]) == 2, names       # signed or not: no column count
    assert len(names) == 3, names
    for name, u in between.items():
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
        assert u["LDS Size"] == 0, (name, u)
        assert u.get("AGPRs", 0) == 0, (name, u)
    print({n[:40]: between[n] for n in names})


def test_the_range_pass_has_the_occupancy_of_the_tag_pass(usage):
    between, tags = usage
    tag_occupancy = {u["Occupancy"] for n, u in tags.items() if "tag_pass_kernel" in n}
    assert tag_occupancy == {8}, tags
    for name, u in between.items():
        assert u["Occupancy"] >= min(tag_occupancy), (name, u)
        if "between_pass_kernel" in name:
            assert u["VGPRs"] <= 64, (name, u)                  # (eight waves a SIMD: 512 / 8)
