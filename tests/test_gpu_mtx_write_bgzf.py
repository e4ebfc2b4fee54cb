"""GPU: cellector_write_mtx_bgzf (csrc/kernels_mtx_write.hip + csrc/kernels_bgzf.hip).  Each file must be bgzf.compress of the file the
numpy twin of cellector_write_mtx makes (cellector_amd/mtx_write.py), byte for byte: three modes x both separators x header_zero,
windows that end 0, 1 and PAYLOAD - 1 bytes past a block cut of the file's text (lines of 7 bytes: 7 is coprime to PAYLOAD, so every
residue is reached), a window smaller than a block, no entry at all, the round trip through the library's block-parallel reader, and
the refusals of cellector_write_mtx plus a file that cannot be written."""
import gzip
import os

import numpy as np
import pytest

from cellector_amd import Cellector, CellectorError, bgzf, ffi, mtx_write, synth

pytestmark = pytest.mark.gpu

P = bgzf.PAYLOAD
MODES = ("aligned", "sparse", "depth")
EINVAL, EIO = 1, 2


@pytest.fixture(scope="module")
def g():
    with Cellector(0) as c:
        yield c


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


def _expected(dims, coo, mode, sep="\t", header_zero=False, write_window=0):
    """(the two files, the summary) from the twins alone"""
    text = [mtx_write.file_bytes(*dims, *coo, k, mode, sep, header_zero) for k in (0, 1)]
    stats = [{}, {}]
    files = [bgzf.compress(t, s) for t, s in zip(text, stats)]
    summary = dict(text=mtx_write.summary(*dims, *coo, mode, sep, header_zero, write_window), file_bytes_first=len(files[0]),
                   file_bytes_second=len(files[1]), blocks_first=stats[0]["blocks"], blocks_second=stats[1]["blocks"],
                   stored_blocks=stats[0]["stored_blocks"] + stats[1]["stored_blocks"])
    return files, summary


def _check(c, tmp_path, name, want, mode, sep="\t", header_zero=False):
    files, summary = want
    a, b = tmp_path / (name + "_first.mtx.gz"), tmp_path / (name + "_second.mtx.gz")
    s = c.write_mtx_bgzf(a, b, mode, sep, header_zero).as_dict()
    for k, (path, wanted) in enumerate(zip((a, b), files)):
        got = path.read_bytes()
        assert got == wanted, "%s file %d: %d bytes against %d, first difference at %d" % (
            name, k, len(got), len(wanted), next((i for i, (x, y) in enumerate(zip(got, wanted)) if x != y), -1))
    assert s == summary
    return a, b


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sep", ["\t", " "], ids=["tab", "space"])
@pytest.mark.parametrize("header_zero", [False, True])
def test_files_are_the_compressed_text(g, tmp_path, mode, sep, header_zero):
    coo = _stage(g, 300, 41, _small_matrix(4097, 100))
    want = _expected((300, 41), coo, mode, sep, header_zero)
    assert want[1]["blocks_first"] >= 2 or mode != "aligned"
    a, _ = _check(g, tmp_path, "f", want, mode, sep, header_zero)
    assert gzip.decompress(a.read_bytes()) == mtx_write.file_bytes(300, 41, *coo, 0, mode, sep, header_zero)


def _seven_byte_lines(n, seed):
    """entries whose lines are 7 bytes in both files of the aligned pair: `1 1 vv`"""
    rng = np.random.default_rng(seed)
    z = np.zeros(n, np.uint32)
    return z, z.copy(), rng.integers(10, 100, n).astype(np.uint32), rng.integers(10, 100, n).astype(np.uint32)


def test_windows_around_the_block_cuts(g, tmp_path):
    n = 2 * P + 4000
    coo = _stage(g, 3, 3, _seven_byte_lines(n, 5))
    head = len(mtx_write.header(3, 3, n))
    assert set(map(len, mtx_write.format_lines(*coo, 0, "aligned").split(b"\n")[:-1])) == {6}
    windows = {}
    for past in (0, 1, P - 1):  # the first window's text ends `past` bytes behind a block cut: head + 7 w = past (mod P)
        w = (past - head) * pow(7, -1, P) % P
        assert w > 0 and (head + 7 * w) % P == past
        windows[past] = w
    windows["below a block"] = 1000
    assert 7 * 1000 < P
    windows["default"] = 0
    want = _expected((3, 3), coo, "aligned")
    assert want[1]["blocks_first"] >= 14 and want[1]["stored_blocks"] == 0
    try:
        for label, w in windows.items():
            g.set_option("write_window", w)
            expected = (want[0], dict(want[1], text=mtx_write.summary(3, 3, *coo, "aligned", write_window=w)))
            _check(g, tmp_path, "w", expected, "aligned")
    finally:
        g.set_option("write_window", 0)


def test_windows_with_dropped_lines(g, tmp_path):
    coo = _stage(g, 300, 41, _small_matrix(6000, 31))
    try:
        for w in (64, 1000, 4097):
            g.set_option("write_window", w)
            for mode in ("sparse", "depth"):
                _check(g, tmp_path, "d", _expected((300, 41), coo, mode, write_window=w), mode)
    finally:
        g.set_option("write_window", 0)


def test_no_entries_is_a_header_only_file(g, tmp_path):
    z = np.zeros(0, np.uint32)
    coo = _stage(g, 300, 41, (z, z.copy(), z.copy(), z.copy()))
    for mode in MODES:
        want = _expected((300, 41), coo, mode)
        assert want[1]["blocks_first"] == want[1]["blocks_second"] == 1
        a, b = _check(g, tmp_path, "none", want, mode)
        assert gzip.decompress(a.read_bytes()) == gzip.decompress(b.read_bytes()) == mtx_write.header(300, 41, 0)


def test_round_trips_through_the_block_parallel_reader(g, tmp_path):
    coo = _stage(g, 300, 41, _small_matrix(9000, 77, zero_share=0.2))
    with Cellector(0) as h:
        for mode, read in (("aligned", lambda a, b: h.load_mtx(a, b)), ("sparse", lambda a, b: h.load_mtx_joined(a, b, "ref")),
                           ("depth", lambda a, b: h.load_mtx_joined(a, b, "depth"))):
            plain = tmp_path / (mode + "_a.mtx"), tmp_path / (mode + "_b.mtx")
            g.write_mtx(*plain, mode)
            read(*plain)
            from_plain = h.staged_coo()
            packed = tmp_path / (mode + "_a.mtx.gz"), tmp_path / (mode + "_b.mtx.gz")
            s = g.write_mtx_bgzf(*packed, mode).as_dict()
            assert s["file_bytes_first"] == os.path.getsize(packed[0]) < os.path.getsize(plain[0])
            read(*packed)
            for got, same, want in zip(h.staged_coo(), from_plain, mtx_write.expected_read_back(*coo, mode)):
                assert np.array_equal(got, same) and np.array_equal(got, want), mode
    for x, y in zip(g.staged_coo(), coo):
        assert np.array_equal(x, y)


def _refused(fn, status, *words):
    with pytest.raises(CellectorError) as e:
        fn()
    assert e.value.status == status, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_refusals(g, tmp_path):
    a, b = str(tmp_path / "a.mtx.gz"), str(tmp_path / "b.mtx.gz")
    coo = _stage(g, 300, 41, _small_matrix(500, 8))
    lib = g._lib

    def same():
        for x, y in zip(g.staged_coo(), coo):
            assert np.array_equal(x, y)

    def raw(first, second, mode=0, flags=0):
        g._ck(lib.cellector_write_mtx_bgzf(g.h, first, second, mode, flags, None))

    assert lib.cellector_write_mtx_bgzf(None, b"a", b"b", 0, 0, None) == EINVAL
    _refused(lambda: raw(a.encode(), b.encode(), 3), EINVAL, "mode")
    _refused(lambda: raw(a.encode(), b.encode(), -1), EINVAL, "mode")
    _refused(lambda: raw(a.encode(), b.encode(), 0, 4), EINVAL, "flags")
    _refused(lambda: raw(a.encode(), a.encode()), EINVAL, "both files")
    _refused(lambda: raw(None, b.encode()), EINVAL, "first_path is NULL")
    _refused(lambda: raw(a.encode(), None), EINVAL, "second_path is NULL")
    assert not os.path.exists(a) and not os.path.exists(b)  # a refusal creates nothing
    # a file that cannot be written: EIO, nothing removed, the ctx as it was
    _refused(lambda: g.write_mtx_bgzf("/dev/full", b), EIO, "/dev/full")
    assert os.path.exists("/dev/full") and not os.path.exists(b)  # (the first file failed: the second was never created)
    _refused(lambda: g.write_mtx_bgzf(a, "/dev/full", "sparse"), EIO, "/dev/full")
    assert os.path.exists("/dev/full") and open(a, "rb").read() == bgzf.compress(mtx_write.file_bytes(300, 41, *coo, 0, "sparse"))
    _refused(lambda: g.write_mtx_bgzf(str(tmp_path / "no_such_dir" / "a.mtx.gz"), b), EIO, "cannot create")
    same()
    _check(g, tmp_path, "after", _expected((300, 41), coo, "aligned"), "aligned")  # ... and it goes on working
    # the scope: cellector_write_mtx's
    with Cellector(0) as e:
        _refused(lambda: e.write_mtx_bgzf(a, b), EINVAL, "no staged matrix")
        e.set_option("keep_coo", 0)
        e.load_coo(300, 41, *coo)
        _refused(lambda: e.write_mtx_bgzf(a, b), EINVAL, "keep_coo")
    with Cellector(0) as e:
        e.set_shard(3, 30)
        e.ingest_coo(300, 41, *coo)
        _refused(lambda: e.write_mtx_bgzf(a, b), EINVAL, "cellector_set_shard")
    with Cellector(devices=[0, 0]) as m:
        m.ingest_coo(300, 41, *coo)
        _refused(lambda: m.write_mtx_bgzf(a, b), EINVAL, "single-device")
    with Cellector(0) as e:
        e.load_coo(400, 150, *synth.generate_coo(400, 150, 0.2, seed=3, minority_fraction=0.1))
        e.em_begin()
        _refused(lambda: e.write_mtx_bgzf(a, b), EINVAL, "cellector_em_begin")
        e.em_threshold()
        e.em_finish()
        e.write_mtx_bgzf(a, b)  # between iterations it is allowed
        assert open(a, "rb").read() == bgzf.compress(mtx_write.file_bytes(400, 150, *e.staged_coo(), 0, "aligned"))
    same()
    assert ffi.SIGNATURES["cellector_write_mtx_bgzf"][1] == ffi.SIGNATURES["cellector_write_mtx"][1]
