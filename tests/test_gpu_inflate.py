"""GPU: cellector_bgzf_decompress (csrc/kernels_inflate.hip) over every stream of tests/inflate_cases.py wrapped into BGZF members: the
ones zlib makes, the library's own, the hand-made ones zlib never emits, the refusals and the mutations.  The text must be
gzip.decompress's byte for byte; a member the reference refuses (inflate_cases.reference) must come back as CELLECTOR_EIO naming that
member, the smallest one when several are damaged, and the ctx must work afterwards.  Sizing, the capacity refusal with canaries on
both sides, several launches per call (CELLECTOR_INFLATE_CHUNK), a plain gzip stream (CELLECTOR_EPARSE), and the round trip through
cellector_bgzf_compress."""
import ctypes as C
import gzip
import re

import numpy as np
import pytest

import bgzf_cases
import inflate_cases as ic
from cellector_amd import Cellector, CellectorError, bgzf

pytestmark = pytest.mark.gpu

EINVAL, EIO, EPARSE = 1, 2, 3
GROUPS = {"zlib": ic.zlib_cases, "library": ic.library_cases, "hand": lambda: {k: v[:3] for k, v in ic.hand_cases().items()}}
GROUPS.update({"mutations_" + n: (lambda n=n: {k: v for k, v in ic.mutation_cases().items() if k.rsplit("_", 1)[0] == "mut_" + n}) for n in ic.MUTATED})


@pytest.fixture(scope="module")
def g():
    with Cellector(0) as c:  # state EMPTY throughout
        yield c


def _decompress(c, data, pad=64):
    """the raw call into the middle of a canary-filled buffer: (text, n_blocks); the canaries must survive, also when it fails"""
    lib = c._lib
    src = np.frombuffer(data, np.uint8)
    ptr = src.ctypes.data_as(C.c_void_p) if len(src) else None
    n_out, n_blocks = C.c_uint64(12345), C.c_uint64(12345)
    c._ck(lib.cellector_bgzf_decompress(c.h, ptr, len(src), None, 0, C.byref(n_out), C.byref(n_blocks)))  # out = NULL: the sizes only
    buf = np.full(pad + n_out.value + pad, 0xA5, np.uint8)
    n2, b2 = C.c_uint64(0), C.c_uint64(0)
    try:
        c._ck(lib.cellector_bgzf_decompress(c.h, ptr, len(src), buf[pad:].ctypes.data_as(C.c_void_p), n_out.value, C.byref(n2), C.byref(b2)))
    finally:
        assert (buf[:pad] == 0xA5).all() and (buf[pad + n_out.value:] == 0xA5).all(), "a byte outside [0, n_out) was written"
    assert (n2.value, b2.value) == (n_out.value, n_blocks.value)
    return buf[pad:pad + n_out.value].tobytes(), n_blocks.value


def _refused_member(c, data):
    with pytest.raises(CellectorError) as e:
        _decompress(c, data)
    assert e.value.status == EIO, str(e.value)
    return int(re.search(r"member (\d+) ", str(e.value)).group(1))


GOOD = ic.member(*ic.zlib_cases()["fixed"])


@pytest.mark.parametrize("group", list(GROUPS))
def test_single_members(g, group):
    refused = 0
    for name, m in sorted(GROUPS[group]().items()):
        stream, want = ic.member(*m), ic.reference(*m)
        if want is None:
            assert _refused_member(g, stream) == 0, name
            refused += 1
            if refused % 50 == 1:   # (the ctx works after a refusal)
                assert _decompress(g, GOOD)[0] == gzip.decompress(GOOD), name
            continue
        text, blocks = _decompress(g, stream)
        assert blocks == 1 and text == want == gzip.decompress(stream), name
    print(group, "refused:", refused)
    if group.startswith("mutations"):
        assert refused >= 150


@pytest.mark.parametrize("chunk", [None, "7", "1"])
def test_concatenated(g, monkeypatch, chunk):
    """every accepted stream in one file, EOF members between and behind; with CELLECTOR_INFLATE_CHUNK in several launches"""
    if chunk:
        monkeypatch.setenv("CELLECTOR_INFLATE_CHUNK", chunk)
    parts = []
    for group in ("zlib", "hand", "library"):
        for name, m in sorted(GROUPS[group]().items()):
            if ic.reference(*m) is not None and (chunk != "1" or group != "library"):
                parts.append(ic.member(*m))
        parts.append(bgzf.EOF)
    stream = b"".join(parts)
    text, blocks = _decompress(g, stream)
    assert blocks == len(parts) and text == gzip.decompress(stream)


def test_capacity_refusal(g):
    stream = ic.member(*ic.zlib_cases()["text_level6"]) + bgzf.EOF
    want = gzip.decompress(stream)
    src = np.frombuffer(stream, np.uint8)
    buf = np.full(len(want) + 128, 0xA5, np.uint8)
    n_out, n_blocks = C.c_uint64(0), C.c_uint64(0)
    st = g._lib.cellector_bgzf_decompress(g.h, src.ctypes.data_as(C.c_void_p), len(src), buf[64:].ctypes.data_as(C.c_void_p), len(want) - 1,
                                          C.byref(n_out), C.byref(n_blocks))
    assert st == EINVAL and (n_out.value, n_blocks.value) == (len(want), 2)
    assert (buf == 0xA5).all(), "a refused call wrote to out"
    assert g.bgzf_decompress(stream) == want


@pytest.mark.parametrize("chunk", [None, "3"])
def test_refusal_names_the_smallest_member(g, monkeypatch, chunk):
    if chunk:
        monkeypatch.setenv("CELLECTOR_INFLATE_CHUNK", chunk)
    h = ic.hand_cases()
    bad1, bad2 = ic.member(*h["wrong_crc"][:3]), ic.member(*h["distance_before_first_byte"][:3])
    assert _refused_member(g, GOOD * 5 + bad1 + GOOD * 3 + bad2 + bgzf.EOF) == 5
    assert _decompress(g, GOOD * 5)[0] == gzip.decompress(GOOD) * 5
    assert _refused_member(g, GOOD * 4 + bad2 + bad1 + GOOD) == 4
    assert _refused_member(g, bad2 + bad1) == 0
    assert _refused_member(g, GOOD * 7 + bad1) == 7
    assert g.bgzf_decompress(GOOD + bgzf.EOF) == gzip.decompress(GOOD)


def test_no_bgzf_stream(g):
    for data in (gzip.compress(b"plain gzip"), GOOD + gzip.compress(b"x"), GOOD[:-1], b"", b"\x1f\x8b"):
        with pytest.raises(CellectorError) as e:
            g.bgzf_decompress(data)
        assert e.value.status == EPARSE, (data[:20], str(e.value))
    assert g.bgzf_decompress(bgzf.EOF) == b""


def test_round_trip(g):
    with Cellector(0) as loaded:
        L, N = 300, 200
        from cellector_amd import synth
        loaded.load_coo(L, N, *synth.generate_coo(L, N, 0.05, seed=3))
        for k, name in enumerate(sorted(bgzf_cases.cases())):
            data = bgzf_cases.cases()[name]
            c = loaded if k % 2 else g   # (a ctx with a matrix and an empty one)
            assert c.bgzf_decompress(c.bgzf_compress(data)) == data, name
        assert loaded.dims().total_loci == L
