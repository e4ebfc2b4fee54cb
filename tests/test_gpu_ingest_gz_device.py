"""GPU: option gz_device (csrc/kernels_parse.hip + csrc/kernels_inflate.hip): a BGZF .gz pair left compressed on the host and inflated
on the device must stage exactly what the host-inflated pair stages.  Two pairs (the 40 x 30, 260-entry one of
tests/test_host_mtx_bytes.py and the project's 2500 x 1500 synthetic one) as BGZF at block sizes 700 and 65280, with and without
the EOF member, and as cellector_write_mtx_bgzf writes them; loaded whole and with parse_window 512, 4096 and 65536 (windows start
inside members, members span windows, the file is shorter than the look-ahead); the staged COO, the loci used and the exclusion
set after three iterations are compared to the bit between gz_device 0 and 1.  The joined ingests, pairs of one BGZF file with a
plain or a plain-gzip one, a last line without its newline; damaged pairs fail under 1 with the status they have under 0, whole
and windowed — a damaged member among the first (the host sees it at the open) and one behind the first MiB of text (the device
refuses it) — and the ctx loads a good pair afterwards."""
import gzip
import os
import re
import struct

import numpy as np
import pytest

import bgzf_cases
import mtx_text_reference as mt
from cellector_amd import Cellector, CellectorError, mtx_write, synth

pytestmark = pytest.mark.gpu

EINVAL, EIO = 1, 2
WINDOWS = (0, 512, 4096, 65536)


def _small(terminated=True, n=260, seed=5):
    L, N = 40, 30
    entries = mt.locus_major_entries(L, N, n, seed)
    la, lr = mt.build_sections(entries, [None] * n, seed, terminated=terminated)
    return mt.mtx_file(L, N, b"".join(la), nnz=n), mt.mtx_file(L, N, b"".join(lr), nnz=n)


def _synthetic(mode="aligned"):
    dims, coo = bgzf_cases.synthetic()
    return tuple(mtx_write.file_bytes(*dims, *coo, k, mode) for k in (0, 1))


PAIRS = {"small": _small(), "synthetic": _synthetic()}


@pytest.fixture(scope="module")
def g():
    with Cellector(0) as c:
        yield c


def _write(tmp_path, name, a, r, ext=(".gz", ".gz")):
    pa, pr = tmp_path / (name + "_alt.mtx" + ext[0]), tmp_path / (name + "_ref.mtx" + ext[1])
    pa.write_bytes(a)
    pr.write_bytes(r)
    return str(pa), str(pr)


def _load(c, pa, pr, gz_device, window, joined=None, iterate=True):
    """(staged COO, loci used, excluded after three iterations) of one load"""
    c.set_option("gz_device", gz_device)
    c.set_option("parse_window", window)
    try:
        if joined:
            c.ingest_mtx_joined(pa, pr, joined)
        else:
            c.ingest_mtx(pa, pr)
        coo = c.staged_coo()
        c.ingest_finish(4, 4)
        used = c.dims().loci_used
        if iterate:
            for _ in range(3):
                c.em_iteration(5.0)
        return coo, used, c.excluded().copy()
    finally:
        c.set_option("gz_device", 0)
        c.set_option("parse_window", 0)


def _same(c, pa, pr, windows=WINDOWS, joined=None, iterate=True):
    want = _load(c, pa, pr, 0, 0, joined, iterate)
    assert len(want[0][0]) > 0
    for window in windows:
        got = _load(c, pa, pr, 1, window, joined, iterate)
        for x, y in zip(got[0], want[0]):
            assert np.array_equal(x, y), window
        assert got[1] == want[1] and np.array_equal(got[2], want[2]), window
    return want


@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("block", [700, 65280])
@pytest.mark.parametrize("eof", [True, False], ids=["eof", "no_eof"])
def test_bgzf_pairs(g, tmp_path, pair, block, eof):
    a, r = (synth.bgzf_compress(x, block=block, eof_block=eof) for x in PAIRS[pair])
    _same(g, *_write(tmp_path, pair, a, r))


def test_pair_written_by_the_library(g, tmp_path):
    dims, coo = bgzf_cases.synthetic()
    with Cellector(0) as w:
        w.ingest_coo(*dims, *coo)
        pa, pr = str(tmp_path / "alt.mtx.gz"), str(tmp_path / "ref.mtx.gz")
        w.write_mtx_bgzf(pa, pr, "aligned")
    got = _same(g, pa, pr)
    for x, y in zip(got[0], coo):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("mode,written", [("ref", "sparse"), ("depth", "depth")])
def test_joined(g, tmp_path, mode, written):
    a, r = (synth.bgzf_compress(x, block=700) for x in _synthetic(written))
    _same(g, *_write(tmp_path, mode, a, r), joined=mode)


def test_mixed_pairs_and_a_last_line_without_newline(g, tmp_path):
    a, r = PAIRS["synthetic"]
    _same(g, *_write(tmp_path, "bgzf_plain", synth.bgzf_compress(a, block=700), r, (".gz", "")))
    _same(g, *_write(tmp_path, "plain_bgzf", a, synth.bgzf_compress(r), ("", ".gz")))
    _same(g, *_write(tmp_path, "bgzf_gzip", synth.bgzf_compress(a), gzip.compress(r)))
    ua, ur = _small(terminated=False)
    assert not ua.endswith(b"\n") and not ur.endswith(b"\n")
    _same(g, *_write(tmp_path, "unterminated", synth.bgzf_compress(ua, block=700), synth.bgzf_compress(ur, block=700, eof_block=False)),
          )


def _members(blob):
    out, pos = [], 0
    while pos < len(blob):
        clen = struct.unpack_from("<H", blob, pos + 16)[0] + 1
        out.append((pos, clen))
        pos += clen
    return out


def _flip(blob, at):
    return blob[:at] + bytes([blob[at] ^ 0x55]) + blob[at + 1:]


def _damaged(a, r, what, k):
    """member k of the ALT file (flip, crc, cut) or of the REF file (isize) damaged, as tests/test_host_mtx_bytes.py does"""
    off, clen = _members(a)[k]
    if what == "flip":
        return _flip(a, off + 18 + (clen - 26) // 2), r
    if what == "crc":
        return _flip(a, off + clen - 7), r
    if what == "cut":
        return a[:off + clen // 2], r
    off, clen = _members(r)[k]
    return a, r[:off + clen - 4] + struct.pack("<I", 70000) + r[off + clen - 4:]


@pytest.fixture(scope="module")
def long_pair():
    """a pair of more than a MiB of text a file (the open inflates only the first MiB on the host), as BGZF of 65280-byte blocks"""
    L, N = 2500, 1500
    coo = synth.generate_coo(L, N, 0.04, seed=13)
    text = tuple(mtx_write.file_bytes(L, N, *coo, k, "aligned") for k in (0, 1))
    assert min(len(t) for t in text) > (1 << 20) + 2 * 65280
    return tuple(synth.bgzf_compress(t) for t in text)


def test_long_pair_in_many_launches(g, tmp_path, long_pair):
    """1.6 MB of text a file: windows of 65536 and 300000 bytes each need a launch of their own (the look-ahead ends inside the
    file), start inside members and share members with their neighbours; whole, CELLECTOR_INFLATE_CHUNK cuts the upload in pieces"""
    _same(g, *_write(tmp_path, "long", *long_pair), windows=(65536, 300000), iterate=False)
    os.environ["CELLECTOR_INFLATE_CHUNK"] = "5"
    try:
        _same(g, *_write(tmp_path, "long", *long_pair), windows=(0,), iterate=False)
    finally:
        del os.environ["CELLECTOR_INFLATE_CHUNK"]


@pytest.mark.parametrize("what", ["flip", "crc", "cut", "isize"])
@pytest.mark.parametrize("where", ["early", "late"])
def test_damaged_pairs_fail_alike(g, tmp_path, long_pair, what, where):
    if where == "early":
        good = tuple(synth.bgzf_compress(x, block=700) for x in PAIRS["small"])
        bad = _damaged(*good, what, 1)
    else:
        good = long_pair
        bad = _damaged(*good, what, len(_members(good[0])) - 2)   # the last member with text: behind the first MiB
    pa, pr = _write(tmp_path, what, *bad)
    ga, gr = _write(tmp_path, "good", *good)
    for blob in bad:
        try:
            gzip.decompress(blob)
        except Exception:
            break
    else:
        raise AssertionError("the damaged pair inflates")
    status = {}
    for gz_device in (0, 1):
        for window in (0, 65536):
            with pytest.raises(CellectorError) as e:
                _load(g, pa, pr, gz_device, window, iterate=False)
            status[gz_device, window] = e.value.status
            if where == "early" or (gz_device, window) == (1, 65536):   # (the ctx loads a good pair afterwards)
                _load(g, ga, gr, gz_device, window, iterate=False)
    assert set(status.values()) == {EIO}, status


INFLATE_LINE = re.compile(r"inflate on the device: (\S+): (\d+) members, (\d+) -> (\d+) bytes")


def _device_lines(err):
    return {os.path.basename(p): (int(m), int(i), int(o)) for p, m, i, o in INFLATE_LINE.findall(err)}


def _expected_line(blob, text):
    """(members, bytes in, bytes out) the whole-file path reports: from the first member that holds data-section text to the end"""
    data_off = len(text) - len(mt.split_header(text)[1])
    out, first = 0, None
    members = _members(blob)
    for k, (off, clen) in enumerate(members):
        isize = struct.unpack_from("<I", blob, off + clen - 4)[0]
        if first is None and out <= data_off < out + isize:
            first = (k, off, out)
        out += isize
    k, off, at = first
    return len(members) - k, len(blob) - off, len(text) - at


@pytest.mark.parametrize("window", [0, 65536])
def test_the_device_path_runs(g, tmp_path, long_pair, monkeypatch, capfd, window):
    """the library's own account under CELLECTOR_TIMING: with gz_device 1 one line per BGZF file with its members and bytes, none for
    the plain-gzip file of a pair, none at all with gz_device 0"""
    monkeypatch.setenv("CELLECTOR_TIMING", "1")
    texts = tuple(gzip.decompress(x) for x in long_pair)
    pa, pr = _write(tmp_path, "ran", *long_pair)
    capfd.readouterr()
    _load(g, pa, pr, 0, window, iterate=False)
    assert _device_lines(capfd.readouterr().err) == {}
    _load(g, pa, pr, 1, window, iterate=False)
    got = _device_lines(capfd.readouterr().err)
    assert set(got) == {"ran_alt.mtx.gz", "ran_ref.mtx.gz"}
    for name, blob, text in zip(("ran_alt.mtx.gz", "ran_ref.mtx.gz"), long_pair, texts):
        members, n_in, n_out = _expected_line(blob, text)
        if window == 0:
            assert got[name] == (members, n_in, n_out), name
        else:   # (windows share the look-ahead's members: every member at least once, those of the look-ahead again)
            assert got[name][0] >= members and got[name][1] >= n_in and got[name][2] >= n_out, name
    pg = str(tmp_path / "ran_ref_plain.mtx.gz")
    open(pg, "wb").write(gzip.compress(texts[1]))
    _load(g, pa, pg, 1, window, iterate=False)
    assert set(_device_lines(capfd.readouterr().err)) == {"ran_alt.mtx.gz"}


def _with_unused_byte(blob, k):
    """member k with one byte between its deflate stream and its trailer: the host's block reader does not look at it, zlib's
    inflate(Z_FINISH) on the exact body, the device's rule, does"""
    off, clen = _members(blob)[k]
    m = blob[off:off + clen]
    m = m[:16] + struct.pack("<H", clen) + m[18:-8] + b"\0" + m[-8:]
    return blob[:off] + m + blob[off + clen:]


@pytest.mark.parametrize("window", [0, 65536])
def test_a_refusal_leaves_a_trace(g, tmp_path, long_pair, capfd, window):
    """a member behind the first MiB that the device refuses: when the host reader refuses the file too, the error keeps the file,
    the member and the reason; when the host reader accepts it, the load is the one of gz_device 0 and stderr says what happened"""
    a, r = long_pair
    k = len(_members(a)) - 3   # behind the first MiB, and not the member with the last byte (which the host looks at before the parse)
    pa, pr = _write(tmp_path, "crc", *_damaged(a, r, "crc", k))
    with pytest.raises(CellectorError) as e:
        _load(g, pa, pr, 1, window, iterate=False)
    assert e.value.status == EIO and "couldn't open file " + pa in str(e.value)
    assert "member %d is refused: the CRC-32 is not the trailer's" % k in str(e.value)
    pa, pr = _write(tmp_path, "unused", _with_unused_byte(a, k), r)
    capfd.readouterr()
    want = _load(g, pa, pr, 0, window, iterate=False)
    assert "gz_device" not in capfd.readouterr().err
    got = _load(g, pa, pr, 1, window, iterate=False)
    err = capfd.readouterr().err
    assert "member %d is refused: unused bytes behind the final block" % k in err and "the host reader accepts the file" in err and pa in err
    pa, pr = _write(tmp_path, "unused_last", _with_unused_byte(a, k + 1), r)   # ... and the member with the last byte
    want = _load(g, pa, pr, 0, window, iterate=False)
    got = _load(g, pa, pr, 1, window, iterate=False)
    assert "member %d is refused: " % (k + 1) in capfd.readouterr().err and all(np.array_equal(x, y) for x, y in zip(got[0], want[0]))
    for x, y in zip(got[0], want[0]):
        assert np.array_equal(x, y)
    assert got[1] == want[1]


def test_option_values(g):
    for v in (2, -1, 7):
        with pytest.raises(CellectorError) as e:
            g.set_option("gz_device", v)
        assert e.value.status == EINVAL
    g.set_option("gz_device", 1)
    g.set_option("gz_device", 0)
