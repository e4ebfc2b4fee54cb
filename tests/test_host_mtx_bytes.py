"""The host byte reader of the mtx ingest (csrc/mtx_bytes.cpp) on a CPU: plain files mapped and unmapped, gzip, BGZF block-parallel
and serial, damaged members, the size line.  tools/mtx_bytes_check.cpp opens a pair through mtx_input_open and reads both data
sections back through FileBytes::read; what it must print and write comes from Python alone (gzip.decompress and
tests/mtx_text_reference.py).  The rule for a ".gz": wherever gzip.decompress raises, the open fails — it never returns bytes."""
import gzip
import os
import struct
import subprocess

import pytest

import mtx_text_reference as mt
from cellector_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EIO, EPARSE = 2, 3


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mtx_bytes_check") / "mtx_bytes_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-Wall",
                           os.path.join(ROOT, "cellector_amd", "csrc", "mtx_bytes.cpp"),
                           os.path.join(ROOT, "tools", "mtx_bytes_check.cpp"), "-lz", "-pthread", "-o", exe])
    return exe


def _pair(size_line=None, terminated=True, n=260, seed=5):
    """(alt file, ref file) of a few KB; size_line replaces the ref file's third header line"""
    L, N = 40, 30
    entries = mt.locus_major_entries(L, N, n, seed)
    la, lr = mt.build_sections(entries, [None] * n, seed, terminated=terminated)
    alt, ref = mt.mtx_file(L, N, b"".join(la), nnz=n), mt.mtx_file(L, N, b"".join(lr), nnz=n)
    if size_line is not None:
        head = ref.split(b"\n", 3)
        ref = b"\n".join([head[0], head[1], size_line, head[3]])
    return alt, ref


ALT, REF = _pair()


def _members(blob):
    """[(offset, length)] of the members of a BGZF file, hopping over the 'BC' size fields"""
    out, pos = [], 0
    while pos < len(blob):
        assert blob[pos + 12:pos + 16] == b"BC\x02\x00"
        clen = struct.unpack_from("<H", blob, pos + 16)[0] + 1
        out.append((pos, clen))
        pos += clen
    return out


def _patched(blob, at, new):
    return blob[:at] + new + blob[at + len(new):]


def _flip(blob, at):
    return _patched(blob, at, bytes([blob[at] ^ 0x55]))


def _bgzf(block, eof_block=True):
    return tuple(synth.bgzf_compress(x, block=block, eof_block=eof_block) for x in (ALT, REF))


def _damaged(what):
    """the BGZF pair with member 1 of the ALT file (flip, crc, cut) or of the REF file (isize) damaged"""
    a, r = _bgzf(700)
    off, clen = _members(a)[1]
    if what == "flip":     # one byte inside the member's deflate data
        return _flip(a, off + 18 + (clen - 26) // 2), r
    if what == "crc":      # one byte inside its CRC-32
        return _flip(a, off + clen - 7), r
    if what == "cut":      # the file ends in the middle of the member
        return a[:off + clen // 2], r
    off, clen = _members(r)[1]   # 'BC' intact, ISIZE above 64 KB: no BGZF index, the serial reader decides
    return a, _patched(r, off + clen - 4, struct.pack("<I", 70000))


def _mixed():
    out = []
    for x in (ALT, REF):
        cut = len(x) * 2 // 3
        out.append(synth.bgzf_compress(x[:cut], block=700, eof_block=False) + gzip.compress(x[cut:]))
    return tuple(out)


UNMAPPED, NO_BGZF = {"CELLECTOR_UNMAPPED_MIN": "1"}, {"CELLECTOR_NO_BGZF": "1"}
# id -> (alt file bytes, ref file bytes, ".gz" or "", environment)
CASES = {
    "plain_mapped": (ALT, REF, "", {}),
    "plain_unmapped": (ALT, REF, "", UNMAPPED),
    "plain_empty_alt": (b"", REF, "", {}),
    "plain_empty_ref": (ALT, b"", "", {}),
    "plain_empty_ref_unmapped": (ALT, b"", "", UNMAPPED),
    "plain_two_header_lines_alt": (b"%%MatrixMarket\n% two lines, the second without its end", REF, "", {}),
    "plain_two_header_lines_ref": (ALT, b"%%MatrixMarket\n40 30 260", "", {}),
    "plain_header_only_ref": (ALT, b"%%MatrixMarket\n%\n40 30", "", {}),
    "plain_unterminated": _pair(terminated=False) + ("", {}),
    "plain_unterminated_unmapped": _pair(terminated=False) + ("", UNMAPPED),
    "gzip_one_member": (gzip.compress(ALT), gzip.compress(REF), ".gz", {}),
    "gzip_two_members": (gzip.compress(ALT[:1500]) + gzip.compress(ALT[1500:]), gzip.compress(REF[:77]) + gzip.compress(REF[77:]), ".gz", {}),
    "bgzf_700": _bgzf(700) + (".gz", {}),
    "bgzf_700_no_eof": _bgzf(700, False) + (".gz", {}),
    "bgzf_ff00": _bgzf(0xff00) + (".gz", {}),
    "bgzf_ff00_no_eof": _bgzf(0xff00, False) + (".gz", {}),
    "bgzf_700_serial": _bgzf(700) + (".gz", NO_BGZF),
    "bgzf_700_no_eof_serial": _bgzf(700, False) + (".gz", NO_BGZF),
    "mixed_bgzf_then_gzip": _mixed() + (".gz", {}),
    "bgzf_isize_above_64k": _damaged("isize") + (".gz", {}),
    "damaged_deflate_byte": _damaged("flip") + (".gz", {}),
    "damaged_crc": _damaged("crc") + (".gz", {}),
    "damaged_cut_in_member": _damaged("cut") + (".gz", {}),
    "damaged_crc_serial": _damaged("crc") + (".gz", NO_BGZF),
    "size_plus_tab_zeros": _pair(b" +5\t007 12") + ("", {}),
    "size_hint_beyond_bytes": _pair(b"40 30 %d" % (len(REF) // 4)) + ("", {}),
    "size_hint_at_bytes": _pair(b"40 30 500") + ("", {}),
    "size_no_third": _pair(b"40 30") + ("", {}),
    "size_third_malformed": _pair(b"40 30 2x0") + ("", {}),
    "size_first_malformed": _pair(b"4o 30 260") + ("", {}),
    "size_second_malformed": _pair(b"40 -30 260") + ("", {}),
    "size_second_missing": _pair(b"40") + ("", {}),
    "size_malformed_gz": tuple(gzip.compress(x) for x in _pair(b"x 30 260")) + (".gz", {}),
}


def _expected(alt_file, ref_file, gz, alt_path, ref_path):
    """what the driver prints and writes: (status, message) or (0, {loci, cells, nnz_hint, off_alt, off_ref}, alt section, ref section)"""
    texts = []
    for blob, path in ((alt_file, alt_path), (ref_file, ref_path)):
        try:
            texts.append(gzip.decompress(blob) if gz else blob)
        except Exception:   # (BadGzipFile, EOFError, zlib.error: the reference's decoder fails the read as well)
            return EIO, "couldn't open file " + path
    (_, sec_a), (third, sec_r) = mt.split_header(texts[0]), mt.split_header(texts[1])
    tok = [mt.token_value(t, limit=(1 << 64) - 1) for t in third.split()[:3]]
    if len(tok) < 2 or None in tok[:2]:
        return EPARSE, "cannot parse the matrix market size line of " + ref_path
    hint = tok[2] if len(tok) == 3 and tok[2] is not None and tok[2] <= len(sec_r) // 4 else 0
    return 0, dict(loci=tok[0], cells=tok[1], nnz_hint=hint, off_alt=len(texts[0]) - len(sec_a), off_ref=len(texts[1]) - len(sec_r)), sec_a, sec_r


@pytest.mark.parametrize("case", list(CASES))
def test_mtx_bytes(driver, tmp_path, case):
    alt_file, ref_file, ext, env = CASES[case]
    alt_path, ref_path = str(tmp_path / ("alt.mtx" + ext)), str(tmp_path / ("ref.mtx" + ext))
    out_a, out_r = str(tmp_path / "alt.section"), str(tmp_path / "ref.section")
    for path, blob in ((alt_path, alt_file), (ref_path, ref_file)):
        with open(path, "wb") as f:
            f.write(blob)
    clean = {k: v for k, v in os.environ.items() if k not in ("CELLECTOR_UNMAPPED_MIN", "CELLECTOR_NO_BGZF")}
    p = subprocess.run([driver, alt_path, ref_path, out_a, out_r], env=dict(clean, **env), capture_output=True, timeout=60)
    want = _expected(alt_file, ref_file, bool(ext), alt_path, ref_path)
    if want[0] != 0:
        assert p.returncode == 1, (p.returncode, p.stdout, p.stderr)
        assert p.stderr.decode() == "status %d: %s\n" % want
        assert p.stdout == b"" and not os.path.exists(out_a) and not os.path.exists(out_r)   # (no bytes of a failed open)
        return
    assert p.returncode == 0, (p.returncode, p.stderr)
    got = dict((k, int(v)) for k, v in (line.split() for line in p.stdout.decode().splitlines()))
    assert got == want[1]
    assert open(out_a, "rb").read() == want[2]
    assert open(out_r, "rb").read() == want[3]


def test_cases_are_what_they_claim():
    """the inputs themselves: which ones Python's gzip refuses, where the hint's bound falls, what the index walk sees"""
    refused = {c for c, (a, r, ext, _) in CASES.items() if ext and _expected(a, r, True, "a", "r")[0] == EIO}
    assert refused == {"bgzf_isize_above_64k", "damaged_deflate_byte", "damaged_crc", "damaged_cut_in_member", "damaged_crc_serial"}
    assert len(_members(_bgzf(700)[0])) > 4 and len(_members(_bgzf(0xff00)[0])) == 2 and len(_members(_bgzf(0xff00, False)[1])) == 1
    a, r = CASES["bgzf_isize_above_64k"][:2]
    assert _members(r) == _members(_bgzf(700)[1])   # (the 'BC' chain is intact)
    sec = len(mt.split_header(REF)[1])
    assert _expected(*CASES["size_hint_beyond_bytes"][:2], False, "a", "r")[1]["nnz_hint"] == 0 and len(REF) // 4 > sec // 4
    assert _expected(*CASES["size_hint_at_bytes"][:2], False, "a", "r")[1]["nnz_hint"] == 500 and 500 <= sec // 4
    assert _expected(*CASES["size_plus_tab_zeros"][:2], False, "a", "r")[1] == dict(
        loci=5, cells=7, nnz_hint=12, off_alt=len(ALT) - len(mt.split_header(ALT)[1]), off_ref=len(b"%%MatrixMarket matrix coordinate integer general\n%\n +5\t007 12\n"))
