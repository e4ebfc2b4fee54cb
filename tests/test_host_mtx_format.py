"""The line renderer the writer's kernels run (csrc/mtx_format.h), on a CPU through tools/mtx_format_check.cpp: every digit boundary
of the two indices and of every mode's third token must give the twin's bytes (cellector_amd/mtx_write.py).  This is where the 9- and
10-digit index widths are held: no GPU test can afford a ctx that large."""
import os
import re
import subprocess

import numpy as np
import pytest

from cellector_amd import mtx_write

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "cellector_amd", "csrc", "mtx_format.h")

# 0-based indices next to every power of ten of the 1-based number, and the two largest
INDICES = sorted({0, 1} | {10 ** k - 2 for k in range(1, 10)} | {10 ** k - 1 for k in range(1, 10)} | {10 ** k for k in range(1, 10)}
                 | {1999999998, 1999999999, 2999999999, 3999999999, 4294967294, 4294967295})
COUNTS = [0, 1, 9, 10, 99, 100, 999, 1000, 9999, 10000, 65535]
# (alt, ref) whose sums are the DEPTH token's boundaries: 99999 / 100000 and the largest, 131070
PAIRS = [(a, r) for a in COUNTS for r in COUNTS] + [(65535, 34464), (65535, 34465), (34464, 65535), (34465, 65535), (65535, 65535), (50000, 49999),
                                                     (50000, 50000)]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mtx_format_check") / "mtx_format_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tools", "mtx_format_check.cpp"),
                           "-o", exe])
    return exe


def _entries():
    rows = []
    for k, i in enumerate(INDICES):  # every index as a locus and as a cell, beside every other width
        a, r = PAIRS[k % len(PAIRS)]
        rows.append((i, INDICES[-1 - k], a, r))
        rows.append((INDICES[(k * 7) % len(INDICES)], i, r, a))
    for k, (a, r) in enumerate(PAIRS):
        rows.append((INDICES[k % len(INDICES)], INDICES[(k * 3) % len(INDICES)], a, r))
    return [np.array(x, np.uint64) for x in zip(*rows)]


@pytest.mark.parametrize("sep", ["\t", " "])
@pytest.mark.parametrize("mode", ["aligned", "sparse", "depth"])
@pytest.mark.parametrize("which", [0, 1])
def test_every_digit_boundary_gives_the_twins_bytes(driver, which, mode, sep):
    lo, ce, al, re_ = _entries()
    assert {8, 9, 98, 99, 999999998, 999999999, 4294967294, 4294967295} <= set(lo.tolist()) & set(ce.tolist())
    sums = set((al + re_).tolist())
    assert {99999, 100000, 131070} <= sums and {0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 65535} <= set(al.tolist()) & set(re_.tolist())
    text = "".join("%d %d %d %d\n" % t for t in zip(lo.tolist(), ce.tolist(), al.tolist(), re_.tolist()))
    r = subprocess.run([driver, str(which), str(mtx_write.MODES[mode]), "t" if sep == "\t" else "s"], input=text.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    want = mtx_write.format_lines(lo, ce, al, re_, which, mode, sep)
    assert r.stdout == want
    assert b"4294967296" in want and (mode != "depth" or which == 0 or b"131070\n" in want)


def test_one_line_at_a_time(driver):
    """a wrong byte is named by its entry, not lost in a long stream"""
    for lo, ce, a, r in ((0, 0, 0, 0), (9, 9, 10, 9), (4294967295, 4294967295, 65535, 65535), (999999999, 99999, 0, 100000 - 65535)):
        for which in (0, 1):
            for mode in (0, 1, 2):
                got = subprocess.run([driver, str(which), str(mode), "t"], input=b"%d %d %d %d\n" % (lo, ce, a, r), capture_output=True)
                assert got.returncode == 0
                assert got.stdout == mtx_write.format_lines([lo], [ce], [a], [r], which, mode), (lo, ce, a, r, which, mode)


def test_the_header_divides_by_constants_only():
    src = re.sub(r"//.*", "", open(HEADER).read())
    assert "printf" not in src and "%" not in src
    assert re.findall(r"/\s*\w+", src) == []  # no division at all: digits come from compares and one multiply-high
    assert "0xCCCCCCCDull) >> 35" in src
    # the multiply-high is floor(v / 10) at the edges of every decade and of the 32-bit range
    for v in [0, 9, 10, 11, 99, 100, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 4294967289, 4294967290] + [10 ** k - 1 for k in range(1, 10)] + [10 ** k for k in range(1, 10)]:
        assert (v * 0xCCCCCCCD) >> 35 == v // 10, v
    assert mtx_write.MAX_LINE == int(re.search(r"#define\s+MTXF_MAX_LINE\s+(\d+)", src).group(1))
