"""Register / scratch budget of the kernels of radius.hip, read from the compiler as tests/test_brute_resources.py
reads brute.hip's (no GPU needed): no scratch and no VGPR spill in any kernel of the file — the tile forms, the decode
and the kernels the segmented sort instantiates — and two waves a SIMD for every form of the tile kernel."""
import pytest

from kernel_usage import have_hipcc, kernel_usage


@pytest.fixture(scope="module")
def usage():
    if not have_hipcc():
        pytest.skip("hipcc not found")
    return kernel_usage("radius.hip")


def _tiles(usage):
    """{(fill, restricted): usage} of radius_tiles_kernel<FILL, RESTRICTED>"""
    out = {}
    for name, u in usage.items():
        if "radius_tiles_kernel" in name:
            for fill in (0, 1):
                for r in (0, 1):
                    if f"ILb{fill}ELb{r}EE" in name:
                        out[bool(fill), bool(r)] = u
    return out


def test_no_kernel_of_radius_hip_uses_scratch_or_spills_vector_registers(usage):
    assert any("radius_decode_kernel" in n for n in usage) and any("segmented" in n for n in usage), sorted(usage)[:8]
    for name, u in usage.items():
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0, (name, u)


def test_every_form_of_the_tile_kernel_keeps_two_waves_a_simd(usage):
    tiles = _tiles(usage)
    assert sorted(tiles) == [(False, False), (False, True), (True, False), (True, True)], sorted(usage)[:8]
    for form, u in tiles.items():
        assert u["Occupancy"] >= 2, (form, u)
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 256, (form, u)         # (512 registers a lane and SIMD / 2 waves)
    print({form: (u["VGPRs"], u.get("AGPRs", 0), u["Occupancy"]) for form, u in tiles.items()})
