"""The writer's numpy twin (cellector_amd/mtx_write.py) against the text contract the project already has: tests/mtx_text_reference.py
reads its bytes back to exactly the arrays written, in all three modes and with both separators, and its ALIGNED + tab + HEADER_ZERO
rendering is the combiner's two files byte for byte.  No GPU."""
import os

import numpy as np
import pytest

import mtx_text_reference as mt
from cellector_amd import join, mtx_write
from test_host_combiner import _run, _two_datasets, combiner_bin  # noqa: F401


def _random_coo(seed, n, total_loci, total_cells, zero_share=0.3, max_count=70000):
    """n entries ascending strictly by (locus, cell); counts of every digit width, a share of zeros in either and in both"""
    rng = np.random.default_rng(seed)
    keys = np.sort(rng.choice(total_loci * total_cells, size=n, replace=False))
    lo, ce = (keys // total_cells).astype(np.uint32), (keys % total_cells).astype(np.uint32)
    width = rng.integers(1, 6, size=(2, n))
    cnt = np.minimum(rng.integers(0, 10 ** width), min(max_count, 65535)).astype(np.uint32)
    cnt[rng.random((2, n)) < zero_share] = 0
    return lo, ce, cnt[0], cnt[1]


HAND = (np.array([0, 0, 8, 9, 98, 99, 999], np.uint32), np.array([0, 9, 9, 10, 0, 99, 100], np.uint32),
        np.array([0, 1, 0, 65535, 10, 0, 9], np.uint32), np.array([0, 0, 7, 65535, 0, 0, 100], np.uint32))
CASES = {"hand": (HAND, 1000, 101), "random": (_random_coo(1, 700, 1200, 90), 1200, 90), "empty": (_random_coo(2, 0, 5, 5), 5, 5),
         "all zero": ((np.arange(40, dtype=np.uint32), np.zeros(40, np.uint32), np.zeros(40, np.uint32), np.zeros(40, np.uint32)), 40, 1)}


def _tokens(data):
    """(locus1, cell1, value) of every body line of one file, by the reference reader's rules"""
    _, sec = mt.split_header(data)
    rows = [mt.alt_line(ln) for ln in mt.data_lines(sec)]
    assert None not in rows
    return tuple(np.array([r[k] for r in rows], np.uint64) for k in range(3))


@pytest.mark.parametrize("sep", ["\t", " "])
@pytest.mark.parametrize("header_zero", [False, True])
@pytest.mark.parametrize("case", sorted(CASES))
def test_aligned_reads_back_to_the_arrays(case, sep, header_zero):
    (lo, ce, al, re), L, N = CASES[case]
    files = [mtx_write.file_bytes(L, N, lo, ce, al, re, k, "aligned", sep, header_zero) for k in (0, 1)]
    m = mt.read_pair(*files)
    assert isinstance(m, mt.Matrix), m
    assert (m.total_loci, m.total_cells) == (L, N)
    assert m.entries == list(zip(lo.tolist(), ce.tolist(), al.tolist(), re.tolist()))
    for k, data in enumerate(files):
        head = data.split(b"\n", 3)
        assert head[0] == b"%%MatrixMarket matrix coordinate real general" and head[1] == b"% written by sprs"
        assert head[2] == (sep.encode()).join(b"%d" % x for x in (L, N, 0 if header_zero else len(lo)))
        assert data.endswith(b"\n") and data == mtx_write.header(L, N, 0 if header_zero else len(lo), sep) + mtx_write.format_lines(lo, ce, al, re, k, "aligned", sep)


@pytest.mark.parametrize("sep", ["\t", " "])
@pytest.mark.parametrize("mode", ["sparse", "depth"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_dropping_modes_read_back_through_the_join(case, mode, sep):
    (lo, ce, al, re), L, N = CASES[case]
    if mode == "depth":  # (the depth join refuses a depth above 65535: the wider sums are the format tests' business)
        re = np.minimum(re, 65535 - al.astype(np.int64)).astype(np.uint32)
    files = [mtx_write.file_bytes(L, N, lo, ce, al, re, k, mode, sep) for k in (0, 1)]
    first, second = _tokens(files[0]), _tokens(files[1])
    assert int(mt.split_header(files[0])[0].split()[2]) == len(first[0]) and int(mt.split_header(files[1])[0].split()[2]) == len(second[0])
    got = join.join_coo(first, second, join.MODE_REF if mode == "sparse" else join.MODE_DEPTH, L, N, one_based=True)
    want = mtx_write.expected_read_back(lo, ce, al, re, mode)
    for g, w in zip(got[:4], want):
        assert np.array_equal(g, w)
    s = mtx_write.summary(L, N, lo, ce, al, re, mode, sep)
    assert s["n_dropped_keys"] == len(lo) - len(want[0]) and s["lines_first"] == len(first[0]) and s["lines_second"] == len(second[0])
    assert (s["bytes_first"], s["bytes_second"]) == (len(files[0]), len(files[1]))


def test_depth_sum_reaches_131070():
    assert mtx_write.format_lines([4], [6], [65535], [65535], 1, "depth") == b"5\t7\t131070\n"
    assert mtx_write.format_lines([4294967295], [4294967294], [0], [3], 1, "sparse", " ") == b"4294967296 4294967295 3\n"
    assert len(b"4294967296\t4294967296\t131070\n") == mtx_write.MAX_LINE


def test_write_pair_and_windows(tmp_path):
    (lo, ce, al, re), L, N = CASES["random"]
    s = mtx_write.write_pair(tmp_path / "a", tmp_path / "b", L, N, lo, ce, al, re, "sparse", " ", True)
    assert (tmp_path / "a").read_bytes() == mtx_write.file_bytes(L, N, lo, ce, al, re, 0, "sparse", " ", True)
    assert (tmp_path / "b").read_bytes() == mtx_write.file_bytes(L, N, lo, ce, al, re, 1, "sparse", " ", True)
    assert s["n_entries"] == 700 and s["n_windows"] == 1
    assert [mtx_write.n_windows(n, w) for n, w in ((0, 0), (0, 5), (1, 0), (4097, 1), (4097, 64), (4097, 1000), (4097, 5000), (1 << 23, 0), ((1 << 23) + 1, 0))] == \
        [0, 0, 1, 4097, 65, 5, 1, 1, 2]
    with pytest.raises(ValueError):
        mtx_write.format_lines(lo, ce, al, re, 0, "aligned", ",")
    with pytest.raises(KeyError):
        mtx_write.format_lines(lo, ce, al, re, 0, "bogus")


@pytest.mark.parametrize("extra", [("--num_cells_1", "80", "--num_cells_2", "25", "--seed", "7"),
                                   ("--num_cells_1", "120", "--num_cells_2", "40", "--downsample_rate", "0.6", "--seed", "3")])
def test_the_combiners_files_byte_for_byte(combiner_bin, tmp_path, extra):  # noqa: F811
    d1, d2, _, _ = _two_datasets(str(tmp_path))
    out = str(tmp_path / "mix")
    r = _run(combiner_bin, d1, d2, out, *extra)
    assert r.returncode == 0, r.stderr
    alt, ref = (open(os.path.join(out, f), "rb").read() for f in ("alt.mtx", "ref.mtx"))
    m = mt.read_pair(alt, ref)
    assert isinstance(m, mt.Matrix) and len(m.entries) > 1000
    lo, ce, al, re = (np.array(x, np.uint32) for x in zip(*m.entries))
    assert ((al == 0) & (re == 0)).any() or "--downsample_rate" not in extra  # (the thinned run keeps its 0 / 0 entries)
    assert mtx_write.file_bytes(m.total_loci, m.total_cells, lo, ce, al, re, 0, "aligned", "\t", header_zero=True) == alt
    assert mtx_write.file_bytes(m.total_loci, m.total_cells, lo, ce, al, re, 1, "aligned", "\t", header_zero=True) == ref
