"""Register / scratch budget of the kernels of brute.hip, read from the compiler as tests/test_kernel_resources.py reads
it (no GPU needed): no scratch and no VGPR spill anywhere, two waves a SIMD for every form of the tile kernel, and the
unrestricted forms no larger than they were before the restricted ones were added as a template parameter."""
import pytest

from kernel_usage import have_hipcc, kernel_usage

# VGPRs + AGPRs of the unrestricted tile kernel before the restriction became a template parameter, by MODE
BEFORE = {0: 163 + 16, 1: 186 + 16}


@pytest.fixture(scope="module")
def usage():
    if not have_hipcc():
        pytest.skip("hipcc not found")
    return kernel_usage("brute.hip")


def _tiles(usage):
    """{(mode, restricted): usage} of brute_tiles_kernel<MODE, RESTRICTED>"""
    out = {}
    for name, u in usage.items():
        if "brute_tiles_kernel" in name:
            for mode in (0, 1):
                for r in (0, 1):
                    if f"ILi{mode}ELb{r}EE" in name:
                        out[mode, bool(r)] = u
    return out


def test_no_kernel_of_brute_hip_uses_scratch_or_spills_vector_registers(usage):
    assert len(usage) == 2 + 4 + 2, sorted(usage)      # norms and sample rows, four tile forms, two selections
    for name, u in usage.items():
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0, (name, u)
    print({n[:48]: (u["VGPRs"], u.get("AGPRs", 0), u["Occupancy"]) for n, u in usage.items()})


def test_every_form_of_the_tile_kernel_keeps_two_waves_a_simd(usage):
    tiles = _tiles(usage)
    assert sorted(tiles) == [(0, False), (0, True), (1, False), (1, True)], sorted(usage)
    for form, u in tiles.items():
        assert u["Occupancy"] >= 2, (form, u)
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 256, (form, u)         # (512 registers a lane and SIMD / 2 waves)


def test_the_unrestricted_forms_are_no_larger_than_before(usage):
    tiles = _tiles(usage)
    for mode, before in BEFORE.items():
        u = tiles[mode, False]
        assert u["VGPRs"] + u.get("AGPRs", 0) <= before, (mode, u)
