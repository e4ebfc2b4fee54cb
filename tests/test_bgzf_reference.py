"""CPU: the BGZF writer's numpy twin (cellector_amd/bgzf.py) against gzip and zlib: every stream inflates to its input as one gzip
file and member by member (raw inflate of each body, CRC-32 and ISIZE of each trailer, the hop by BSIZE), ends with the EOF member,
cuts its blocks at multiples of PAYLOAD, stores what the preset does not shrink (the tie at exactly len + 5 bytes from both sides),
and the preset is a complete code of lengths 1..15.

On the writer's text of the project's synthetic matrix (2500 x 1500 at 1 %, aligned mode, both files, tabs and spaces) the stream
must be smaller than zlib.compress(text, 1).  Measured (stream bytes, EOF member included, over zlib level 1 / level 6 bytes):
  locus-major  alt 0.771 / 0.913   ref 0.784 / 0.924     (407 683 bytes of text -> 111 571 / 115 305: 3.65x / 3.54x)
  cell-major   alt 0.839 / 0.983   ref 0.852 / 0.996     (-> 124 052 / 128 482: 3.29x / 3.17x)
(tabs and spaces agree to the third digit; the test prints the figures)."""
import gzip
import struct
import zlib

import pytest

import bgzf_cases
from cellector_amd import bgzf, mtx_write

P = bgzf.PAYLOAD
NAMES = sorted(bgzf_cases.cases())


def _check_stream(data, stream):
    """the member-by-member contract; returns [(input bytes, stored)] per data member"""
    assert gzip.decompress(stream) == data
    assert stream.endswith(bgzf.EOF) and len(bgzf.EOF) == 28
    out, at = [], 0
    mem = bgzf.members(stream)
    assert mem[-1] == (len(stream) - 28, 28)
    for off, size in mem[:-1]:
        m = stream[off:off + size]
        assert m[:16] == bytes.fromhex("1f8b08040000000000ff060042430200") and size <= 65536
        body, (crc, isize) = m[18:-8], struct.unpack("<II", m[-8:])
        z = zlib.decompressobj(-15)
        piece = z.decompress(body)
        assert z.eof and z.unused_data == b"", "the body is one complete deflate stream with BFINAL set"
        assert piece == data[at:at + isize] and isize == len(piece) and crc == zlib.crc32(piece)
        assert 0 < isize <= P and (isize == P or at + isize == len(data)), "blocks are cut at multiples of PAYLOAD"
        assert body[0] & 1 == 1 and (body[0] >> 1) & 3 in (0, 2)
        stored = (body[0] >> 1) & 3 == 0
        if stored:
            assert body == b"\x01" + struct.pack("<HH", isize, isize ^ 0xFFFF) + piece
        else:
            assert len(body) < isize + 5
        out.append((isize, stored))
        at += isize
    assert at == len(data)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_stream_inflates_member_by_member(name):
    data = bgzf_cases.cases()[name]
    stream, stats = bgzf_cases.expected(name)
    blocks = _check_stream(data, stream)
    assert stats == dict(blocks=(len(data) + P - 1) // P, stored_blocks=sum(s for _, s in blocks))
    assert len(blocks) == stats["blocks"]


def test_sizes_around_the_block_cut():
    c = bgzf_cases.cases()
    assert [len(c["size_" + k]) for k in ("0", "1", "P-1", "P", "P+1", "2P", "2P+1")] == [0, 1, P - 1, P, P + 1, 2 * P, 2 * P + 1]
    assert bgzf_cases.expected("size_0")[0] == bgzf.EOF
    for k, n in (("1", 1), ("P-1", 1), ("P", 1), ("P+1", 2), ("2P", 2), ("2P+1", 3)):
        assert bgzf_cases.expected("size_" + k)[1]["blocks"] == n
    # a block depends on nothing before it: the stream of two blocks is the two blocks' streams
    two = c["size_2P"]
    assert bgzf_cases.expected("size_2P")[0] == bgzf.member(two[:P]) + bgzf.member(two[P:]) + bgzf.EOF


def test_stored_blocks_and_the_tie():
    for name in ("no_newline", "random", "size_1", "one_newline"):
        stats = bgzf_cases.expected(name)[1]
        assert stats["stored_blocks"] == stats["blocks"] > 0, name
    tie, kept = bgzf_cases.cases()["tie_stored"], bgzf_cases.cases()["tie_kept"]
    assert len(bgzf.deflate_preset(tie)) == len(tie) + 5 and bgzf_cases.expected("tie_stored")[1]["stored_blocks"] == 1
    assert len(bgzf.deflate_preset(kept)) == len(kept) + 4 and bgzf_cases.expected("tie_kept")[1]["stored_blocks"] == 0
    assert zlib.decompress(bgzf.deflate_preset(tie), -15) == tie  # (the form that lost the tie is valid too)
    assert bgzf_cases.expected("only_newlines")[1]["stored_blocks"] == 0


@pytest.mark.parametrize("L,lengths", [(255, [255]), (257, [257]), (258, [258]), (259, [258, 1]), (260, [258, 1, 1]), (261, [258, 3]),
                                       (262, [258, 4]), (513, [258, 255]), (516, [258, 258]), (517, [258, 258, 1]),
                                       (518, [258, 258, 1, 1]), (519, [258, 258, 3])])
def test_pieces_of_258_and_their_tails(L, lengths):
    """two equal lines: the second is one run of L, cut into 258s; a tail of 1 or 2 bytes is literals"""
    data = bgzf_cases.cases()["equal_lines_%d" % L]
    pos, length, dist = bgzf.tokens(data)
    second = pos >= L
    assert length[second].tolist() == lengths
    assert [int(d) for d, n in zip(dist[second], lengths)] == [L if n >= 3 else 0 for n in lengths]
    assert (dist[~second] == 0).all() and (~second).sum() == L


def test_tokens_follow_the_definition():
    # segment 0 has no candidate; d is the length of the line before; a longer line reads its own bytes
    pos, length, dist = bgzf.tokens(b"ab\nab\nabXabXabX\n")
    assert list(zip(pos.tolist(), length.tolist(), dist.tolist())) == [(0, 1, 0), (1, 1, 0), (2, 1, 0), (3, 5, 3), (8, 1, 0), (9, 6, 3),
                                                                      (15, 1, 0)]
    # the run goes on over a newline while d stays, and ends where d changes
    pos, length, dist = bgzf.tokens(b"ab\nab\nab\nabc\nabc\n")
    assert list(zip(pos.tolist(), length.tolist(), dist.tolist()))[3:] == [(3, 8, 3), (11, 1, 0), (12, 1, 0), (13, 4, 4)]
    # a line length that changes on every line: no d is equal across a newline
    pos, length, dist = bgzf.tokens(bgzf_cases.cases()["changing_lengths"])
    assert dist.max() == 299 and (length <= 300).all()


def test_preset_is_a_complete_code():
    p = bgzf.preset()
    assert len(p["litlen"]) == 286 and len(p["dist"]) == 30
    for lengths in (p["litlen"], p["dist"]):
        assert all(1 <= x <= 15 for x in lengths)
        assert sum(1 << (15 - x) for x in lengths) == 1 << 15, "Kraft sum exactly 1"
    assert len(p["header"]) == (p["header_bits"] + 7) // 8 and p["header"][0] & 7 == 0b101  # BFINAL = 1, BTYPE = 10
    # zlib reads the table: an empty block under it
    assert gzip.decompress(bgzf.compress(b"\n" * 10)) == b"\n" * 10


def test_frozen_preset_is_what_the_tool_makes():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bgzf_preset_tool", os.path.join(root, "tools", "bgzf_preset.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    py, c = tool.render(*tool.make())
    assert open(os.path.join(root, "cellector_amd", "bgzf_preset.py")).read() == py
    assert open(os.path.join(root, "cellector_amd", "csrc", "bgzf_preset.h")).read() == c


@pytest.mark.parametrize("order", ["locus", "cell"])
@pytest.mark.parametrize("sep", ["tab", "space"])
@pytest.mark.parametrize("which", [0, 1])
def test_smaller_than_zlib_level_1_on_the_writers_text(order, sep, which):
    name = "mtx_%s_aligned_%s_%d" % (order, sep, which)
    text, stream = bgzf_cases.cases()[name], bgzf_cases.expected(name)[0]
    z1, z6 = len(zlib.compress(text, 1)), len(zlib.compress(text, 6))
    print("%s: %d bytes of text, stream %d, zlib level 1 %d (%.3f), level 6 %d (%.3f)" %
          (name, len(text), len(stream), z1, len(stream) / z1, z6, len(stream) / z6))
    assert len(stream) < z1


def test_write_pair_files_round_trip(tmp_path):
    dims, coo = bgzf_cases.synthetic("locus")
    for mode in ("aligned", "sparse", "depth"):
        for sep in ("\t", " "):
            a, b = tmp_path / "a.mtx", tmp_path / "b.mtx"
            mtx_write.write_pair(a, b, *dims, *coo, mode, sep)
            for k, path in enumerate((a, b)):
                text = path.read_bytes()
                assert text == bgzf_cases.cases()["mtx_locus_%s_%s_%d" % (mode, "tab" if sep == "\t" else "space", k)]
                assert gzip.decompress(bgzf.compress(text)) == text
