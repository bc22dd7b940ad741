"""The handout arithmetic of tickets.h on the CPU: `make ticket_ranges` builds hoststub/ticket_ranges_test.cc with the
host compiler (under UBSan) around the header's constexpr functions — tk_range_lo, the bounds of the eight ranges the
work counters of the persistent scan kernels stand for, and tk_range_at, the cyclic order in which a wave walks them
from wherever it starts (the XCC id of its XCD in the plain scan) — and prints what they give.  Whatever range a wave
starts at, and however many blocks there are, every block must lie in exactly one range and every range must be
visited once: that, and the atomic counters, is all the correctness of the handout rests on."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tinyknn_amd", "csrc")

NBS = [0, 1, 7, 8, 9, 1023, 1024, 1025]


@pytest.fixture(scope="module")
def printed():
    if not shutil.which("g++") or not shutil.which("make"):
        pytest.skip("no host toolchain")
    r = subprocess.run(["make", "-C", CSRC, "ticket_ranges"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    r = subprocess.run([os.path.join(CSRC, "hoststub", "ticket_ranges")] + [str(n) for n in NBS],
                       capture_output=True, text=True, timeout=60,
                       env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    rows = [line.split() for line in r.stdout.splitlines()]
    tickets = [int(x[1]) for x in rows if x[0] == "tickets"]
    assert tickets == [8]
    bounds = {int(x[1]): [int(v) for v in x[2:]] for x in rows if x[0] == "N"}
    order = {int(x[1]): [int(v) for v in x[2:]] for x in rows if x[0] == "start"}
    return bounds, order


@pytest.mark.parametrize("nb", NBS)
def test_ranges_partition_the_blocks(printed, nb):
    bounds, _ = printed
    lo = bounds[nb]
    assert len(lo) == 9 and lo[0] == 0 and lo[8] == nb, lo
    assert all(a <= b for a, b in zip(lo, lo[1:])), lo
    # every block in exactly one range, spelled out
    owner = [0] * nb
    for r in range(8):
        for b in range(lo[r], lo[r + 1]):
            owner[b] += 1
    assert owner == [1] * nb
    # equal shares: no range more than one block longer than another
    lens = [b - a for a, b in zip(lo, lo[1:])]
    assert max(lens) - min(lens) <= 1, lens


@pytest.mark.parametrize("nb", NBS)
@pytest.mark.parametrize("start", range(8))
def test_every_start_visits_every_range_once(printed, nb, start):
    bounds, order = printed
    walk = order[start]
    assert walk[0] == start and sorted(walk) == list(range(8)), walk
    assert all(b == (a + 1) % 8 for a, b in zip(walk, walk[1:])), walk
    # a wave alone on the device, starting here, is handed every block exactly once
    lo = bounds[nb]
    handed = [b for r in walk for b in range(lo[r], lo[r + 1])]
    assert sorted(handed) == list(range(nb))
