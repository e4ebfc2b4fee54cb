"""GPU: cellector_bgzf_compress (csrc/kernels_bgzf.hip) against the numpy twin (cellector_amd/bgzf.py), exact bytes on every input of
tests/bgzf_cases.py: sizes around the block cut, only newlines, stored blocks and the tie at len + 5, runs cut into 258s with tails of
0 to 3 bytes, a line longer than a block, changing line lengths, all byte values, a block that opens inside a line, and the writer's
text in its three modes; canaries behind n_out, the capacity refusal, a ctx in state EMPTY and one with a loaded matrix, both
engines."""
import ctypes as C
import gzip

import numpy as np
import pytest

import bgzf_cases
from cellector_amd import Cellector, CellectorError, bgzf, synth

pytestmark = pytest.mark.gpu

NAMES = sorted(bgzf_cases.cases())
EINVAL = 1


@pytest.fixture(scope="module")
def g():
    with Cellector(0) as c:  # state EMPTY throughout
        yield c


def _compress(c, data, pad=64):
    """the raw call into the middle of a canary-filled buffer: (stream, n_blocks); the canaries must survive"""
    lib = c._lib
    src = np.frombuffer(data, np.uint8)
    ptr = src.ctypes.data_as(C.c_void_p) if len(src) else None
    n_out, n_blocks = C.c_uint64(12345), C.c_uint64(12345)
    c._ck(lib.cellector_bgzf_compress(c.h, ptr, len(src), None, 0, C.byref(n_out), C.byref(n_blocks)))  # out = NULL: the sizes only
    buf = np.full(pad + n_out.value + pad, 0xA5, np.uint8)
    n2, b2 = C.c_uint64(0), C.c_uint64(0)
    c._ck(lib.cellector_bgzf_compress(c.h, ptr, len(src), buf[pad:].ctypes.data_as(C.c_void_p), n_out.value, C.byref(n2), C.byref(b2)))
    assert (n2.value, b2.value) == (n_out.value, n_blocks.value)
    assert (buf[:pad] == 0xA5).all() and (buf[pad + n_out.value:] == 0xA5).all(), "a byte outside [0, n_out) was written"
    return buf[pad:pad + n_out.value].tobytes(), n_blocks.value


@pytest.mark.parametrize("name", NAMES)
def test_stream_is_the_twins(g, name):
    data = bgzf_cases.cases()[name]
    want, stats = bgzf_cases.expected(name)
    got, blocks = _compress(g, data)
    assert blocks == stats["blocks"]
    assert got == want, "first difference at byte %d of %d" % (next((k for k, (x, y) in enumerate(zip(got, want)) if x != y), -1), len(want))


def test_python_binding_and_gzip(g):
    data = bgzf_cases.cases()["mtx_locus_sparse_tab_1"]
    stream = g.bgzf_compress(data)
    assert stream == bgzf_cases.expected("mtx_locus_sparse_tab_1")[0] and gzip.decompress(stream) == data
    assert g.bgzf_compress(b"") == bgzf.EOF


def test_capacity_refusal(g):
    data = bgzf_cases.cases()["size_P+1"]
    want = bgzf_cases.expected("size_P+1")[0]
    src = np.frombuffer(data, np.uint8)
    for cap in (0, 27, len(want) - 28, len(want) - 1):  # (also: room for the members but not for the EOF member)
        buf = np.full(len(want) + 32, 0xA5, np.uint8)
        n_out, n_blocks = C.c_uint64(0), C.c_uint64(0)
        with pytest.raises(CellectorError) as e:
            g._ck(g._lib.cellector_bgzf_compress(g.h, src.ctypes.data_as(C.c_void_p), len(src), buf.ctypes.data_as(C.c_void_p), cap,
                                                 C.byref(n_out), C.byref(n_blocks)))
        assert e.value.status == EINVAL and "capacity" in str(e.value)
        assert (n_out.value, n_blocks.value) == (len(want), 2) and (buf == 0xA5).all()
    with pytest.raises(CellectorError) as e:
        g._ck(g._lib.cellector_bgzf_compress(g.h, None, 5, None, 0, None, None))
    assert e.value.status == EINVAL and "NULL" in str(e.value)
    assert g._lib.cellector_bgzf_compress(None, None, 0, None, 0, None, None) == EINVAL


@pytest.mark.parametrize("engine", [2, 1], ids=["tiled", "csr"])
def test_a_loaded_ctx_of_either_engine_is_left_alone(engine):
    L, N = 400, 150
    coo = synth.generate_coo(L, N, 0.2, seed=3, minority_fraction=0.1)
    name = "mtx_cell_aligned_space_0"
    with Cellector(0) as c:
        c.set_option("engine", engine)
        c.load_coo(L, N, *coo)
        c.em_iteration(5.0)
        before = c.cell_outputs()
        assert _compress(c, bgzf_cases.cases()[name])[0] == bgzf_cases.expected(name)[0]
        after = c.cell_outputs()
        for k in before:
            assert np.array_equal(np.asarray(before[k]), np.asarray(after[k])), k
        c.em_iteration(5.0)  # ... and goes on working
    with Cellector(devices=[0, 0]) as m:
        with pytest.raises(CellectorError) as e:
            m.bgzf_compress(b"1 2 3\n")
        assert e.value.status == EINVAL and "single-device" in str(e.value)
