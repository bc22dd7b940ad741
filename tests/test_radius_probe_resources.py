"""Register / scratch budget of the kernels of radius_probe.hip, read from the compiler as
tests/test_radius_resources.py reads radius.hip's (no GPU needed): no scratch and no VGPR spill in any kernel of the
file, and at least four waves a SIMD (128 vector registers a lane or fewer) for the six forms of the count kernel and
the three of the fill kernel.  What the compiler reports (profiles/r25/radius_probe_kernel_resources.txt):
    count <T, TY, RESTRICTED>     VGPRs   occupancy          fill <T, TY>       VGPRs   occupancy
    float,  float,  false           46       8               float,  float        55       8
    float,  float,  true            47       7               float,  half         58       8
    float,  half,   false           48       8               double, double       88       5
    float,  half,   true            49       7
    double, double, false           58       8
    double, double, true            79       6
The restricted forms keep 26 - 35 scalar registers in lanes of a vector register (SGPR spill, no memory)."""
import pytest

from kernel_usage import have_hipcc, kernel_usage

TYPES = {("f", "f"): "Iff", ("f", "h"): "IfDF16_", ("d", "d"): "Idd"}


@pytest.fixture(scope="module")
def usage():
    if not have_hipcc():
        pytest.skip("hipcc not found")
    return kernel_usage("radius_probe.hip")


def _forms(usage):
    """{("count", T, TY, restricted) | ("fill", T, TY): usage}"""
    out = {}
    for name, u in usage.items():
        for (t, ty), tag in TYPES.items():
            if "radius_probe_count_kernel" + tag in name:
                for r in (0, 1):
                    if f"{tag}Lb{r}EE" in name:
                        out["count", t, ty, bool(r)] = u
            if "radius_probe_fill_kernel" + tag + "E" in name:
                out["fill", t, ty] = u
    return out


def test_no_kernel_of_radius_probe_hip_uses_scratch_or_spills_vector_registers(usage):
    for kernel in ("rp_words_kernel", "rp_rank_kernel", "rp_decode64_kernel", "radius_probe_count_kernel",
                   "radius_probe_fill_kernel"):
        assert any(kernel in n for n in usage), (kernel, sorted(usage))
    for name, u in usage.items():
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0, (name, u)


def test_the_six_count_forms_and_three_fill_forms_keep_four_waves_a_simd(usage):
    forms = _forms(usage)
    want = [("count", t, ty, r) for (t, ty) in TYPES for r in (False, True)] + [("fill", t, ty) for (t, ty) in TYPES]
    assert sorted(forms, key=str) == sorted(want, key=str), sorted(usage)
    for form, u in forms.items():
        assert u["Occupancy"] >= 4, (form, u)
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 128, (form, u)         # (512 registers a lane and SIMD / 4 waves)
    print({form: (u["VGPRs"], u["Occupancy"]) for form, u in forms.items()})
