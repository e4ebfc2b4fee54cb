"""CPU: the BGZF reader's interface without a GPU.  The library loads and exports cellector_bgzf_decompress, the header declares it
and documents option gz_device, and the compressed kind of the host byte reader (csrc/mtx_bytes.cpp: a BGZF ".gz" left compressed for
the device, with its member index) serves the head, the last byte and random ranges through FileBytes::read as gzip.decompress has
them.  tools/gz_bytes_check.cpp opens a pair the way option gz_device does; what it must print comes from Python alone."""
import gzip
import os
import subprocess

import pytest

import mtx_text_reference as mt
from cellector_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK = (1 << 64) - 1


def test_library_exports_the_call(hip_lib_path):
    from cellector_amd import ffi
    lib = ffi.load_library()
    assert hasattr(lib, "cellector_bgzf_decompress")
    assert callable(getattr(ffi.Cellector, "bgzf_decompress"))


def test_header_declares_it():
    text = open(os.path.join(ROOT, "include", "cellector_ffi.h")).read()
    assert "cellector_status cellector_bgzf_decompress(cellector_ctx *ctx, const uint8_t *in, uint64_t n, uint8_t *out, uint64_t capacity," in text
    assert '"gz_device"' in text and "CELLECTOR_INFLATE_CHUNK" in text
    fmt = open(os.path.join(ROOT, "cellector_amd", "csrc", "inflate_format.h")).read()
    assert "inflate_member_host(const uint8_t *in, uint32_t n_in, uint8_t *out, uint32_t isize, int *err)" in fmt


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gz_bytes_check") / "gz_bytes_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-Wall",
                           os.path.join(ROOT, "cellector_amd", "csrc", "mtx_bytes.cpp"),
                           os.path.join(ROOT, "tools", "gz_bytes_check.cpp"), "-lz", "-pthread", "-o", exe])
    return exe


def _pair(n=260, seed=5, terminated=True):
    L, N = 40, 30
    entries = mt.locus_major_entries(L, N, n, seed)
    la, lr = mt.build_sections(entries, [None] * n, seed, terminated=terminated)
    return mt.mtx_file(L, N, b"".join(la), nnz=n), mt.mtx_file(L, N, b"".join(lr), nnz=n)


def _fnv(data):
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & MASK
    return h


def _expected(blob, text, kind, seed, n_ranges):
    members = 0
    if kind:
        pos = 0
        while pos < len(blob):
            pos += int.from_bytes(blob[pos + 16:pos + 18], "little") + 1
            members += 1
    out = ["kind %d" % kind, "size %d" % len(text), "members %d" % members, "head " + text[:64].hex(), "last %d" % (text[-1] if text else -1)]
    for r in range(n_ranges):
        seed = (seed * 6364136223846793005 + 1442695040888963407) & MASK
        off = (seed >> 33) % len(text) if text else 0
        seed = (seed * 6364136223846793005 + 1442695040888963407) & MASK
        ln = ((seed >> 33) % (200000 if r % 4 == 0 else 3000)) % (len(text) - off + 1)
        out.append("range %d %d %d" % (off, ln, _fnv(text[off:off + ln])))
    return out


ALT, REF = _pair()
BIG = _pair(n=9000, seed=7)      # ~100 KB a file: members of 65280 bytes are more than one
CASES = {
    # id -> (alt blob, ref blob, kind of alt, kind of ref, environment)
    "bgzf_700": (synth.bgzf_compress(ALT, block=700), synth.bgzf_compress(REF, block=700), 1, 1, {}),
    "bgzf_700_no_eof": (synth.bgzf_compress(ALT, block=700, eof_block=False), synth.bgzf_compress(REF, block=700, eof_block=False), 1, 1, {}),
    "bgzf_ff00_big": (synth.bgzf_compress(BIG[0], block=0xff00), synth.bgzf_compress(BIG[1], block=0xff00, eof_block=False), 1, 1, {}),
    "bgzf_and_plain_gzip": (synth.bgzf_compress(ALT, block=700), gzip.compress(REF), 1, 0, {}),
    "no_bgzf_in_the_environment": (synth.bgzf_compress(ALT, block=700), synth.bgzf_compress(REF, block=700), 0, 0, {"CELLECTOR_NO_BGZF": "1"}),
    "unterminated": tuple(synth.bgzf_compress(x, block=700) for x in _pair(terminated=False)) + (1, 1, {}),
    "eof_members_inside": (synth.bgzf_compress(ALT[:900], block=700) + synth.bgzf_compress(ALT[900:], block=333),
                           synth.bgzf_compress(REF[:5], block=700) + synth.bgzf_compress(REF[5:], block=64), 1, 1, {}),
}


@pytest.mark.parametrize("case", list(CASES))
def test_compressed_kind(driver, tmp_path, case):
    alt_blob, ref_blob, kind_a, kind_r, env = CASES[case]
    alt_path, ref_path = str(tmp_path / "alt.mtx.gz"), str(tmp_path / "ref.mtx.gz")
    for path, blob in ((alt_path, alt_blob), (ref_path, ref_blob)):
        with open(path, "wb") as f:
            f.write(blob)
    clean = {k: v for k, v in os.environ.items() if k not in ("CELLECTOR_UNMAPPED_MIN", "CELLECTOR_NO_BGZF")}
    p = subprocess.run([driver, alt_path, ref_path, "11", "40"], env=dict(clean, **env), capture_output=True, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stderr)
    ta, tr = gzip.decompress(alt_blob), gzip.decompress(ref_blob)
    (_, sec_a), (_, sec_r) = mt.split_header(ta), mt.split_header(tr)
    want = _expected(alt_blob, ta, kind_a, 11, 40) + _expected(ref_blob, tr, kind_r, 12, 40)
    want += ["loci 40", "cells 30", "off_alt %d" % (len(ta) - len(sec_a)), "off_ref %d" % (len(tr) - len(sec_r))]
    assert p.stdout.decode().splitlines() == want


def test_damaged_member_in_the_head_goes_to_the_host_reader(driver, tmp_path):
    """the open inflates the first members on the host; one it refuses leaves the file to the host reader, which fails as it does
    without the option"""
    a, r = synth.bgzf_compress(ALT, block=700), synth.bgzf_compress(REF, block=700)
    clen = int.from_bytes(a[16:18], "little") + 1
    at = clen + 18 + 20   # inside the deflate data of member 1
    bad = a[:at] + bytes([a[at] ^ 0x55]) + a[at + 1:]
    alt_path, ref_path = str(tmp_path / "alt.mtx.gz"), str(tmp_path / "ref.mtx.gz")
    open(alt_path, "wb").write(bad)
    open(ref_path, "wb").write(r)
    with pytest.raises(Exception):
        gzip.decompress(bad)
    p = subprocess.run([driver, alt_path, ref_path, "1", "1"], capture_output=True, timeout=60)
    assert p.returncode == 1 and p.stderr.decode() == "status 2: couldn't open file %s\n" % alt_path
