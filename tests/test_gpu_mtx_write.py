"""GPU: cellector_write_mtx / cellector_format_mtx (csrc/kernels_mtx_write.hip).  Every comparison is exact bytes against the numpy
twin (cellector_amd/mtx_write.py) on staged_coo(): entry counts around every block and wave size, ranges off any power of two, canaries
around the destination, the shortest, the longest and random line lengths (with the ragged heads and tails of any block size
exercised, asserted from the twin alone), every digit width a real ctx reaches, dropped lines, windows, round trips through the
library's three readers, and the refusals.

The 9- and 10-digit indices are held on the host (tests/test_host_mtx_format.py): no GPU test can afford a ctx that large."""
import ctypes as C
import os

import numpy as np
import pytest

from cellector_amd import Cellector, CellectorError, ffi, mtx_write, synth

pytestmark = pytest.mark.gpu

BIG_L, BIG_N = 10_000_001, 100_001  # the one large ctx: 8-digit loci, 6-digit cells
MODES = ("aligned", "sparse", "depth")
EINVAL, EIO = 1, 2


@pytest.fixture(scope="module")
def g():
    with Cellector(0) as c:
        yield c


def _fmt(c, which, mode, first=0, n=None, sep="\t", pad=48):
    """format_mtx into the middle of a canary-filled buffer: (bytes, n_lines); the canaries must survive"""
    lib, m, fl = c._lib, mtx_write.MODES[mode], mtx_write.flags(sep)
    if n is None:
        n = len(c.staged_coo()[0]) - first
    nb, nl = C.c_uint64(12345), C.c_uint64(12345)
    c._ck(lib.cellector_format_mtx(c.h, which, m, fl, first, n, None, 0, C.byref(nb), C.byref(nl)))  # out = NULL: the counts only
    buf = np.full(pad + nb.value + pad, 0xA5, np.uint8)
    nb2, nl2 = C.c_uint64(0), C.c_uint64(0)
    c._ck(lib.cellector_format_mtx(c.h, which, m, fl, first, n, buf[pad:].ctypes.data_as(C.c_void_p), nb.value, C.byref(nb2), C.byref(nl2)))
    assert (nb2.value, nl2.value) == (nb.value, nl.value)
    assert (buf[:pad] == 0xA5).all() and (buf[pad + nb.value:] == 0xA5).all(), "a byte outside [0, n_bytes) was written"
    return buf[pad:pad + nb.value].tobytes(), nl.value


def _check_format(c, coo, which, mode, first=0, n=None, sep="\t"):
    n = len(coo[0]) - first if n is None else n
    part = [a[first:first + n] for a in coo]
    got, lines = _fmt(c, which, mode, first, n, sep)
    assert got == mtx_write.format_lines(*part, which, mode, sep), (which, mode, first, n)
    assert lines == mtx_write.n_lines(part[2], part[3], which, mode)


def _random_lengths(n, seed, L=BIG_L, N=BIG_N, zero_share=0.0):
    """n entries in any order whose index and count widths are drawn per entry: lines of 6 to 22 bytes"""
    rng = np.random.default_rng(seed)
    wl, wc, wv = rng.integers(1, 9, n), rng.integers(1, 7, n), rng.integers(1, 6, (2, n))
    lo = np.minimum(rng.integers(0, 10 ** wl), L - 1).astype(np.uint32)
    ce = np.minimum(rng.integers(0, 10 ** wc), N - 1).astype(np.uint32)
    cnt = np.minimum(rng.integers(0, 10 ** wv), 65535).astype(np.uint32)
    cnt[rng.random((2, n)) < zero_share] = 0
    return lo, ce, cnt[0], cnt[1]


def _small_matrix(n, seed, zero_share=0.3):
    """n entries ascending strictly by (locus, cell) on 300 x 41, counts of one to four digits, zeros in either and in both"""
    rng = np.random.default_rng(seed)
    keys = np.sort(rng.choice(300 * 41, size=n, replace=False))
    cnt = rng.integers(0, 10 ** rng.integers(1, 5, (2, n))).astype(np.uint32)
    cnt[rng.random((2, n)) < zero_share] = 0
    return (keys // 41).astype(np.uint32), (keys % 41).astype(np.uint32), cnt[0], cnt[1]


def _stage(c, total_loci, total_cells, coo):
    c.ingest_coo(total_loci, total_cells, *coo)
    got = c.staged_coo()
    for a, b in zip(got, coo):
        assert np.array_equal(a, b)
    return got


def _files(c, tmp_path, name, mode, sep="\t", header_zero=False):
    a, b = tmp_path / (name + "_first.mtx"), tmp_path / (name + "_second.mtx")
    s = c.write_mtx(a, b, mode, sep, header_zero)
    return a.read_bytes(), b.read_bytes(), s.as_dict()


def _check_files(c, tmp_path, name, dims, coo, mode, sep="\t", header_zero=False, write_window=0):
    first, second, s = _files(c, tmp_path, name, mode, sep, header_zero)
    assert first == mtx_write.file_bytes(*dims, *coo, 0, mode, sep, header_zero)
    assert second == mtx_write.file_bytes(*dims, *coo, 1, mode, sep, header_zero)
    assert s == mtx_write.summary(*dims, *coo, mode, sep, header_zero, write_window)
    return s


# ---- sizes and ranges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4097])
def test_entry_counts_and_ranges(g, tmp_path, n):
    coo = _stage(g, 300, 41, _small_matrix(n, 100 + n))
    for mode in MODES:
        for which in (0, 1):
            _check_format(g, coo, which, mode)
    _check_format(g, coo, 0, "aligned", sep=" ")
    for first in sorted({f for f in (1, 7, 65, n - 1) if 0 <= f <= n}):
        for length in sorted({0, min(1, n - first), n - first}):
            _check_format(g, coo, first % 2, MODES[first % 3], first, length)
    _check_format(g, coo, 1, "sparse", n, 0)  # the empty range at the end
    _check_files(g, tmp_path, "n%d" % n, (300, 41), coo, MODES[n % 3], " " if n % 2 else "\t", header_zero=n % 4 == 1)


# ---- line-length mixes --------------------------------------------------------------------------------------------------------
def test_all_lines_the_shortest(g, tmp_path):
    n = 4097
    coo = _stage(g, 3, 3, tuple(np.zeros(n, np.uint32) for _ in range(4)))
    assert mtx_write.format_lines(*coo, 0, "aligned") == b"1\t1\t0\n" * n  # six bytes: several lines per 16-byte unit
    for first, length in ((0, n), (1, n - 1), (5, 3000)):
        _check_format(g, coo, 0, "aligned", first, length)
    _check_files(g, tmp_path, "short", (3, 3), coo, "aligned")


def test_all_lines_long_and_random_lengths(g, tmp_path):
    n = 4097
    rng = np.random.default_rng(9)
    coo = (rng.integers(9_999_999, BIG_L, n).astype(np.uint32), rng.integers(99_999, BIG_N, n).astype(np.uint32),
           rng.integers(10000, 65536, n).astype(np.uint32), rng.integers(40000, 65536, n).astype(np.uint32))
    coo = _stage(g, BIG_L, BIG_N, coo)
    assert set(map(len, mtx_write.format_lines(*coo, 0, "aligned").split(b"\n")[:-1])) == {8 + 6 + 5 + 2}  # the longest a real ctx reaches here
    for mode in MODES:
        _check_format(g, coo, 1, mode)  # (depth: six-digit sums)
    _check_files(g, tmp_path, "long", (BIG_L, BIG_N), coo, "depth")

    # random lengths.  From the twin alone: over the ranges formatted below, at the entry boundaries of every power-of-two block
    # size from 64 to 4096, the byte offset inside the range takes all 16 residues mod 16 — whatever block size the kernel uses,
    # its ragged heads and tails are all exercised
    n, n_ranges = 6000, 100
    coo = _stage(g, BIG_L, BIG_N, _random_lengths(n, 5))
    lens = np.array([len(x) + 1 for x in mtx_write.format_lines(*coo, 0, "aligned").split(b"\n")[:-1]])
    assert len(lens) == n and lens.min() <= 8 and lens.max() >= 20
    cum = np.concatenate([[0], np.cumsum(lens)])
    for block in (64, 128, 256, 512, 1024, 2048, 4096):
        seen = {int((cum[f + k * block] - cum[f]) % 16) for f in range(n_ranges) for k in range(1, (n - f) // block + 1)}
        assert seen == set(range(16)), block
    for f in range(n_ranges):
        _check_format(g, coo, 0, "aligned", f, n - f)
    for mode in MODES:
        _check_files(g, tmp_path, "random_" + mode, (BIG_L, BIG_N), coo, mode)


# ---- digit widths through a real ctx ----------------------------------------------------------------------------------------------
def test_digit_widths(g, tmp_path):
    loci = [0, 8, 9, 98, 99, 998, 999, 9998, 9999, 99_998, 99_999, 999_998, 999_999, 9_999_998, 9_999_999, 10_000_000]
    cells = [0, 8, 9, 98, 99, 998, 999, 9998, 9999, 99_998, 99_999, 100_000]
    counts = [0, 1, 9, 10, 99, 100, 999, 1000, 9999, 10000, 65535]
    pairs = [(a, r) for a in counts for r in counts] + [(65535, 34464), (65535, 34465), (34464, 65535), (34465, 65535), (65535, 65535)]
    rows = [(loci[k % len(loci)], cells[(k // 3) % len(cells)], a, r) for k, (a, r) in enumerate(pairs)]
    rows += [(l, cells[k % len(cells)], 7, 0) for k, l in enumerate(loci)] + [(loci[k % len(loci)], c, 0, 12) for k, c in enumerate(cells)]
    coo = _stage(g, BIG_L, BIG_N, tuple(np.array(x, np.uint32) for x in zip(*rows)))
    assert {99999, 100000, 131070} <= set((coo[2].astype(np.int64) + coo[3]).tolist())
    for mode in MODES:
        for which in (0, 1):
            for sep in ("\t", " "):
                _check_format(g, coo, which, mode, sep=sep)
        _check_files(g, tmp_path, "digits_" + mode, (BIG_L, BIG_N), coo, mode, header_zero=True)
    text = _fmt(g, 0, "aligned")[0]
    assert b"\n10000001\t" in text and b"\t100001\t" in text
    text = _fmt(g, 1, "depth")[0]
    assert b"\t131070\n" in text and b"\t99999\n" in text and b"\t100000\n" in text


# ---- dropped lines ------------------------------------------------------------------------------------------------------------------
def test_dropped_lines(g, tmp_path):
    n = 9001
    lo, ce, al, re = _small_matrix(n, 77, zero_share=0.2)
    for a in (al, re):
        a[0] = a[-1] = 0          # the first and the last entry dropped
        a[700:700 + 4300] = 0     # a run longer than 4096: whatever the block size, a block emits no byte
    coo = _stage(g, 300, 41, (lo, ce, al, re))
    dropped = int(((al == 0) & (re == 0)).sum())
    assert dropped > 4300
    for mode in MODES:
        for which in (0, 1):
            _check_format(g, coo, which, mode)
        _check_format(g, coo, 0, mode, 700, 4300)   # a range without a line
        if mode != "aligned":
            assert _fmt(g, 1, mode, 700, 4300) == (b"", 0)
        s = _check_files(g, tmp_path, "dropped_" + mode, (300, 41), coo, mode)
        assert s["n_dropped_keys"] == dropped and (mode != "aligned" or s["lines_first"] == n)
    # every entry dropped: the body is empty
    zeros = _stage(g, 300, 41, (lo[:300], ce[:300], np.zeros(300, np.uint32), np.zeros(300, np.uint32)))
    for mode in ("sparse", "depth"):
        first, second, s = _files(g, tmp_path, "none_" + mode, mode)
        assert first == second == mtx_write.header(300, 41, 0) and s["n_dropped_keys"] == 300 and s["lines_first"] == s["lines_second"] == 0
        assert _fmt(g, 0, mode) == (b"", 0)
    _check_files(g, tmp_path, "none_aligned", (300, 41), zeros, "aligned")


# ---- windows ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [1, 64, 1000, 5000])
def test_windows(g, tmp_path, window):
    n = 4097
    coo = _stage(g, 300, 41, _small_matrix(n, 31))
    try:
        g.set_option("write_window", window)
        assert mtx_write.n_windows(n, window) == {1: 4097, 64: 65, 1000: 5, 5000: 1}[window]
        s = _check_files(g, tmp_path, "w", (300, 41), coo, "sparse", header_zero=True, write_window=window)
        assert s["n_windows"] == -(-n // window)
        _check_format(g, coo, 0, "depth")
        if window > 1:  # (each window is a round trip: the one-entry window is held to one file pair and one range)
            _check_files(g, tmp_path, "w", (300, 41), coo, "aligned", " ", write_window=window)
            _check_files(g, tmp_path, "w", (300, 41), coo, "depth", write_window=window)
            _check_format(g, coo, 1, "aligned", 7, n - 8)
    finally:
        g.set_option("write_window", 0)
    _check_files(g, tmp_path, "w0", (300, 41), coo, "sparse", header_zero=True)  # ... and the default window again


# ---- round trips on the device ------------------------------------------------------------------------------------------------------
def _round_trips(c, tmp_path, name):
    """the ctx's staged matrix through the three readers on a second ctx"""
    coo = c.staged_coo()
    d = c.dims()
    key = coo[0].astype(np.uint64) << np.uint64(32) | coo[1]
    assert np.all(key[1:] > key[:-1]) and int(coo[2].max()) + int(coo[3].max()) <= 65535  # what the joins read back
    with Cellector(0) as h:
        for mode, read in (("aligned", lambda a, b: h.load_mtx(a, b)), ("sparse", lambda a, b: h.load_mtx_joined(a, b, "ref")),
                           ("depth", lambda a, b: h.load_mtx_joined(a, b, "depth"))):
            a, b = tmp_path / (name + mode + "_a.mtx"), tmp_path / (name + mode + "_b.mtx")
            s = c.write_mtx(a, b, mode).as_dict()
            assert s == mtx_write.summary(d.total_loci, d.total_cells, *coo, mode)
            read(a, b)
            assert (h.dims().total_loci, h.dims().total_cells) == (d.total_loci, d.total_cells)
            for got, want in zip(h.staged_coo(), mtx_write.expected_read_back(*coo, mode)):
                assert np.array_equal(got, want), (name, mode)
    for x, y in zip(c.staged_coo(), coo):
        assert np.array_equal(x, y)
    return coo


def test_round_trips(g, tmp_path):
    L, N1, N2 = 400, 150, 50
    a = synth.generate_coo(L, N1, 0.2, seed=3, minority_fraction=0.1)
    b = synth.generate_coo(L, N2, 0.2, seed=4, minority_fraction=0.0)
    with Cellector(0) as src:
        src.ingest_coo(L, N2, *b)
        g.ingest_coo(L, N1, *a)
        g.combine(src, downsample_rate=0.3, seed=5)   # ascending, unique keys, some 0 / 0 entries
    coo = _round_trips(g, tmp_path, "combined")
    assert ((coo[2] == 0) & (coo[3] == 0)).any()
    g.restage(keep=np.arange(N1 + N2) % 3 != 1, downsample_rate=0.2, seed=6)
    _round_trips(g, tmp_path, "restaged")
    g.add_doublets([0, 5, 9], [3, 4, 20], downsample_rate=0.1)
    _round_trips(g, tmp_path, "doublets")
    # LOADED with its COO: the write leaves the built matrix and the EM state alone
    with Cellector(0) as ref:
        ref.load_coo(g.dims().total_loci, g.dims().total_cells, *g.staged_coo())
        ref.run()
        want = ref.posteriors()
    g.ingest_finish()
    _round_trips(g, tmp_path, "loaded")
    g.run()
    got = g.posteriors()
    for k in want:
        assert np.array_equal(np.asarray(want[k]), np.asarray(got[k])), k
    _round_trips(g, tmp_path, "loaded_after_run")


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def _refused(fn, status, *words):
    with pytest.raises(CellectorError) as e:
        fn()
    assert e.value.status == status, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_refusals(g, tmp_path):
    a, b = str(tmp_path / "a.mtx"), str(tmp_path / "b.mtx")
    coo = _stage(g, 300, 41, _small_matrix(500, 8))
    lib = g._lib

    def same():
        for x, y in zip(g.staged_coo(), coo):
            assert np.array_equal(x, y)

    def raw_write(first, second, mode=0, flags=0):
        g._ck(lib.cellector_write_mtx(g.h, first, second, mode, flags, None))

    def raw_format(which=0, mode=0, flags=0, first=0, n=500, out=None, cap=0, nb=None):
        g._ck(lib.cellector_format_mtx(g.h, which, mode, flags, first, n, out, cap, nb, None))

    _refused(lambda: raw_write(a.encode(), b.encode(), 3), EINVAL, "mode")
    _refused(lambda: raw_write(a.encode(), b.encode(), -1), EINVAL, "mode")
    _refused(lambda: raw_write(a.encode(), b.encode(), 0, 4), EINVAL, "flags")
    _refused(lambda: raw_write(a.encode(), a.encode()), EINVAL, "both files")
    _refused(lambda: raw_write(None, b.encode()), EINVAL, "first_path is NULL")
    _refused(lambda: raw_write(a.encode(), None), EINVAL, "second_path is NULL")
    assert not os.path.exists(a) and not os.path.exists(b)  # a refusal creates nothing
    _refused(lambda: raw_format(mode=7), EINVAL, "mode")
    _refused(lambda: raw_format(flags=8), EINVAL, "flags")
    _refused(lambda: raw_format(which=2), EINVAL, "which")
    _refused(lambda: raw_format(which=-1), EINVAL, "which")
    _refused(lambda: raw_format(first=1, n=500), EINVAL, "beyond")
    _refused(lambda: raw_format(first=501, n=0), EINVAL, "beyond")
    _refused(lambda: raw_format(first=2 ** 64 - 1, n=2), EINVAL, "beyond")
    same()
    # a capacity below n_bytes: refused, n_bytes still returned, not a byte written
    want = mtx_write.format_lines(*coo, 0, "aligned")
    buf = np.full(len(want) + 32, 0xA5, np.uint8)
    nb = C.c_uint64(0)
    _refused(lambda: raw_format(out=buf.ctypes.data_as(C.c_void_p), cap=len(want) - 1, nb=C.byref(nb)), EINVAL, "capacity")
    assert nb.value == len(want) and (buf == 0xA5).all()
    same()
    # a file that cannot be written: EIO, nothing removed
    _refused(lambda: g.write_mtx("/dev/full", b), EIO, "/dev/full")
    assert os.path.exists("/dev/full") and not os.path.exists(b)  # (the first file failed: the second was never created)
    _refused(lambda: g.write_mtx(a, "/dev/full", "sparse"), EIO, "/dev/full")
    assert os.path.exists("/dev/full") and open(a, "rb").read() == mtx_write.file_bytes(300, 41, *coo, 0, "sparse")  # what was written stays
    _refused(lambda: g.write_mtx(str(tmp_path / "no_such_dir" / "a.mtx"), b), EIO, "cannot create")
    same()
    # the scope: cellector_restage's
    with Cellector(0) as e:
        _refused(lambda: e.write_mtx(a, b), EINVAL, "no staged matrix")
        _refused(lambda: e.format_mtx(0), EINVAL)
        e.set_option("keep_coo", 0)
        e.load_coo(300, 41, *coo)
        _refused(lambda: e.write_mtx(a, b), EINVAL, "keep_coo")
        _refused(lambda: _fmt(e, 0, "aligned", 0, 1), EINVAL, "keep_coo")
    with Cellector(0) as e:
        e.set_shard(3, 30)
        e.ingest_coo(300, 41, *coo)
        _refused(lambda: e.write_mtx(a, b), EINVAL, "cellector_set_shard")
        _refused(lambda: _fmt(e, 0, "aligned", 0, 1), EINVAL, "cellector_set_shard")
    with Cellector(devices=[0, 0]) as m:
        m.ingest_coo(300, 41, *coo)
        _refused(lambda: m.write_mtx(a, b), EINVAL, "single-device")
        _refused(lambda: _fmt(m, 0, "aligned", 0, 1), EINVAL, "single-device")
    # a ctx with a communicator is one whose ranks stage their own cells (the one-rank RCCL self-test of tests/test_gpu_combine.py)
    os.environ["CELLECTOR_COMM_SELFTEST"] = "1"
    try:
        with Cellector(0) as e:
            e.comm_init_rank(ffi.comm_unique_id(), 1, 0)
            e.ingest_coo(300, 41, *coo)
            _refused(lambda: e.write_mtx(a, b), EINVAL, "communicator")
            _refused(lambda: _fmt(e, 0, "aligned", 0, 1), EINVAL, "communicator")
    finally:
        os.environ.pop("CELLECTOR_COMM_SELFTEST", None)
    with Cellector(0) as e:
        e.load_coo(400, 150, *synth.generate_coo(400, 150, 0.2, seed=3, minority_fraction=0.1))
        e.em_begin()
        _refused(lambda: e.write_mtx(a, b), EINVAL, "cellector_em_begin")
        _refused(lambda: _fmt(e, 0, "aligned", 0, 1), EINVAL, "cellector_em_begin")
        e.em_threshold()
        _refused(lambda: e.write_mtx(a, b), EINVAL, "cellector_em_begin")
        e.em_finish()
        e.write_mtx(a, b)  # between iterations it is allowed
        assert open(a, "rb").read() == mtx_write.file_bytes(400, 150, *e.staged_coo(), 0, "aligned")
    same()
