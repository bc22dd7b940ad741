"""What the compiler reports for the kernels of one file of tinyknn_amd/csrc (no GPU needed): the file is compiled
for gfx950 with the library's flags and -Rpass-analysis=kernel-resource-usage, once per file and process; the tests
that pin registers, scratch and occupancy share the result and leave it unchanged."""
import functools
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tinyknn_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
         "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", "-o", os.devnull]


def have_hipcc():
    return bool(shutil.which(HIPCC)) or os.path.exists(HIPCC)


@functools.lru_cache(maxsize=None)
def kernel_usage(fname):
    """{mangled kernel name: {remark: value}} of csrc/<fname>, e.g. "VGPRs", "ScratchSize", "Occupancy" """
    r = subprocess.run([HIPCC] + FLAGS + [fname], cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {}
    cur = None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out
