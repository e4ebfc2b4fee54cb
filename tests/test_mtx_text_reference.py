"""CPU: tests/mtx_text_reference.py (the text contract on bytes, and the builder of files with exact line lengths) against
hand-written statements of the contract and against the oracle's reader (oracle/cellector_oracle.c, orc_load_mtx: gzgets lines,
its own tokeniser), which is the project's reading of load_data.rs:190-223.  The GPU sweep (test_gpu_text_sweep.py) holds the
device tokeniser to this reference; here the reference is held to something that is not itself."""
import random
import re

import numpy as np
import pytest

import mtx_text_reference as mt

HDR = b"%%MatrixMarket\n%\n"


def _pair(alt_body, ref_body, size=b"2 3 0"):
    return HDR + b"99 99 99\n" + alt_body, HDR + size + b"\n" + ref_body


# ---- the contract, statement by statement -----------------------------------------------------------------------------------
def test_header_dims_come_from_the_ref_files_third_line_and_the_count_is_ignored():
    m = mt.read_pair(*_pair(b"1 1 2\n", b"1 1 1\n", size=b" +2\t003 77777 and more"))
    assert m == mt.Matrix(2, 3, [(0, 0, 2, 1)])
    assert mt.read_pair(*_pair(b"1 1 2\n", b"1 1 1\n", size=b"2")) == mt.TextError("size_line", None)
    assert mt.read_pair(*_pair(b"1 1 2\n", b"1 1 1\n", size=b"2 x")) == mt.TextError("size_line", None)
    # three lines are consumed whatever they hold; headers of different lengths do not matter
    a = b"only\ntwo\n5 5 5\n1 2 3\n"
    r = b"%\n%%%%%%%%%%%%%%%%%%%%%%%%%%%%%%%%%%%%%%%%%%%%%%%%\n1 2\n. . 4\n"
    assert mt.read_pair(a, r) == mt.Matrix(1, 2, [(0, 1, 3, 4)])
    assert mt.read_pair(HDR, HDR) == mt.TextError("size_line", None)   # no third line at all
    assert mt.read_pair(HDR + b"1 1\n", HDR + b"4 5") == mt.Matrix(4, 5, [])   # a size line without newline, no data


def test_lines_a_final_line_without_newline_counts_and_nothing_follows_a_final_newline():
    assert mt.data_lines(b"") == []
    assert mt.data_lines(b"\n") == [b""]
    assert mt.data_lines(b"a\nb") == [b"a", b"b"]
    assert mt.data_lines(b"a\nb\n") == [b"a", b"b"]
    assert mt.data_lines(b"a\n\n") == [b"a", b""]
    m = mt.read_pair(*_pair(b"1 1 2\n2 3 7", b"1 1 1\n1 1 0\n"))
    assert m.entries == [(0, 0, 2, 1), (1, 2, 7, 0)]
    assert mt.read_pair(*_pair(b"1 1 2\n\n", b"1 1 1\n1 1 1\n")) == mt.TextError("parse", 1)   # a blank line is a line


def test_tokens_ascii_whitespace_plus_sign_leading_zeros_extra_tokens():
    m = mt.read_pair(*_pair(b" \t1\f\v+2\r 0003 junk 9 9\r\n", b"x y\t+0065535   z\n"))
    assert m.entries == [(0, 1, 3, 65535)]
    # 0x1c-0x1f, 0x85 and 0xa0 split a str but are no whitespace here: one token "1\x1c1", so a token is missing
    for ch in (b"\x1c", b"\x1d", b"\x1e", b"\x1f", b"\x85", b"\xa0", b"\x00"):
        assert mt.read_pair(*_pair(b"1" + ch + b"1 1\n", b"1 1 1\n")) == mt.TextError("parse", 0), ch
    for bad in (b"1 1 1.0", b"1 1", b"1 -1 1", b"1 1 ++1", b"1 1 +", b"1 1 1e3", b"1 1 0x1", b"", b"   ", b"1 1 4294967296",
                b"4294967296 1 1", b"1 1 1_0"):
        assert mt.read_pair(*_pair(bad + b"\n", b"1 1 1\n")) == mt.TextError("parse", 0), bad
    assert mt.read_pair(*_pair(b"1 1 1\n", b"1 1\n")) == mt.TextError("parse", 0)          # the ref count is missing
    assert mt.read_pair(*_pair(b"1 1 1\n", b"1 1 1.5\n")) == mt.TextError("parse", 0)
    assert mt.read_pair(*_pair(b"1 1 4294967295\n", b"1 1 1\n")) == mt.TextError("count_range", 0)   # parses, then too big
    assert mt.token_value(b"007") == 7 and mt.token_value(b"+0") == 0 and mt.token_value(b"-0") is None


def test_range_kinds_in_their_order_and_the_zip_stops_at_the_shorter_file():
    assert mt.read_pair(*_pair(b"0 9 70000\n", b"1 1 1\n")) == mt.TextError("index0", 0)
    assert mt.read_pair(*_pair(b"9 0 70000\n", b"1 1 1\n")) == mt.TextError("index0", 0)
    assert mt.read_pair(*_pair(b"3 9 70000\n", b"1 1 1\n")) == mt.TextError("locus_range", 0)
    assert mt.read_pair(*_pair(b"2 4 70000\n", b"1 1 1\n")) == mt.TextError("cell_range", 0)
    assert mt.read_pair(*_pair(b"2 3 65536\n", b"1 1 1\n")) == mt.TextError("count_range", 0)
    assert mt.read_pair(*_pair(b"2 3 65535\n", b"1 1 65536\n")) == mt.TextError("count_range", 0)
    assert mt.read_pair(*_pair(b"2 3 65535\n", b"0 0 65535\n")) == mt.Matrix(2, 3, [(1, 2, 65535, 65535)])
    # beyond the shorter file nothing is read: neither a malformed line nor a range error
    assert mt.read_pair(*_pair(b"1 1 1\nx\n0 0 0\n", b"1 1 1\n")) == mt.Matrix(2, 3, [(0, 0, 1, 1)])
    assert mt.read_pair(*_pair(b"1 1 1\n", b"1 1 1\nx\n\n")) == mt.Matrix(2, 3, [(0, 0, 1, 1)])
    assert mt.read_pair(*_pair(b"1 1 1\nx\n", b"1 1 1\n1 1 1")) == mt.TextError("parse", 1)


def test_precedence_a_parse_error_beats_any_range_error_else_the_smallest_entry_with_its_own_kind():
    good = b"1 1 1\n"
    assert mt.read_pair(*_pair(b"0 1 1\n" + good + b"x\n", good * 3)) == mt.TextError("parse", 2)
    assert mt.read_pair(*_pair(b"0 1 1\n" + good * 2, good * 2 + b"1 1\n")) == mt.TextError("parse", 2)
    assert mt.read_pair(*_pair(good + b"1 4 1\n" + b"3 1 1\n0 1 1\n", good * 4)) == mt.TextError("cell_range", 1)
    assert mt.read_pair(*_pair(good + b"x\n" + b"y\n", b"z\n" * 3)) == mt.TextError("parse", 0)   # the ref file's is earlier
    assert mt.read_pair(*_pair(b"0 1 1\n" + good + b"x\n", good * 2)) == mt.TextError("index0", 0)   # the bad line is never read


# ---- the builder ------------------------------------------------------------------------------------------------------------
def test_builder_writes_exact_lengths_that_read_back_and_refuses_what_does_not_fit():
    rng = random.Random(3)
    L, N = 5000, 70000
    entries = mt.locus_major_entries(L, N, 400, seed=1)
    lengths = [rng.choice((None, mt.min_length((l + 1, c + 1, a)), 16, 17, 63, 64, 65, 128, 129, 300, 401)) for l, c, a, r in entries]
    lengths[7] = 5000
    alt, ref = mt.build_sections(entries, lengths, seed=9)
    for k, want in enumerate(lengths):
        if want is not None:
            assert len(alt[k]) == want and len(ref[k]) == want, k
        assert alt[k].endswith(b"\n") and alt[k].count(b"\n") == 1 and ref[k].count(b"\n") == 1
    m = mt.read_pair(mt.mtx_file(L, N, b"".join(alt)), mt.mtx_file(L, N, b"".join(ref), nnz=None))
    assert m == mt.Matrix(L, N, entries)
    text = b"".join(alt) + b"".join(ref)
    for feature in (b"\r\n", b"+", b" 0", b"\t", b"\f", b"\v", b"x 0 "):   # every kind of padding is in there
        assert feature in text, feature
    assert (alt, ref) == mt.build_sections(entries, lengths, seed=9) != mt.build_sections(entries, lengths, seed=10)
    # unterminated: the last line has no newline and its length counts none
    alt_u, ref_u = mt.build_sections(entries[:3], [20, 20, 20], seed=1, terminated=False, ref_lengths=[9, 30, 11])
    assert [len(x) for x in alt_u] == [20, 20, 20] and [len(x) for x in ref_u] == [9, 30, 11]
    assert not alt_u[-1].endswith(b"\n") and not ref_u[-1].endswith(b"\n") and alt_u[0].endswith(b"\n")
    assert mt.read_pair(mt.mtx_file(L, N, b"".join(alt_u)), mt.mtx_file(L, N, b"".join(ref_u))).entries == entries[:3]
    blanks = mt.build_line((12, 345, 6), 1 << 16, rng, style="blanks")
    assert len(blanks) == 1 << 16 and set(blanks) <= set(b" 1234567890\n") and mt.alt_line(blanks[:-1]) == (12, 345, 6)
    with pytest.raises(ValueError):
        mt.build_line((4999, 69999, 300), 14, rng)   # "4999 69999 300\n" needs 15
    assert len(mt.build_line((4999, 69999, 300), 15, rng)) == 15
    with pytest.raises(ValueError):
        mt.build_sections(entries[:2], [6, 5], seed=1)
    with pytest.raises(ValueError):
        mt.build_sections(entries[:2], [30], seed=1)


# ---- against the oracle's reader --------------------------------------------------------------------------------------------
def _write(tmp_path, name, alt_bytes, ref_bytes):
    a, r = tmp_path / (name + "_alt.mtx"), tmp_path / (name + "_ref.mtx")
    a.write_bytes(alt_bytes)
    r.write_bytes(ref_bytes)
    return str(a), str(r)


def _oracle_rows(o):
    """per cell, in the oracle's order (file order): [(locus0, alt, ref), ...]"""
    li, a, r, _ = o.entries()
    ids, rp = o.locus_ids(), o.row_ptr()
    flat = list(zip(ids[li].tolist(), a.tolist(), r.tolist()))
    return [flat[int(rp[c]):int(rp[c + 1])] for c in range(o.total_cells)]


@pytest.mark.parametrize("terminated", [True, False])
def test_reference_equals_the_oracles_reader_on_padded_files(oracle_lib, tmp_path, terminated):
    L, N = 211, 97
    entries = mt.locus_major_entries(L, N, 519, seed=4)
    rng = random.Random(8)
    lengths = [rng.choice((None, None, 15, 16, 17, 40, 63, 64, 65, 127, 128, 129, 255, 256, 257, 401)) for _ in entries]
    ref_lengths = [rng.choice((None, 14, 33, 64, 128, 200, 401)) for _ in entries]
    alt, ref = mt.build_sections(entries, lengths, seed=5, terminated=terminated, ref_lengths=ref_lengths)
    ref += [b"7 7 7\n", b"junk beyond the alt file's last line\n"]   # the zip stops at the shorter file
    a_bytes = mt.mtx_file(999, 999, b"".join(alt), nnz=5)                               # the alt header's dims are not read
    r_bytes = mt.mtx_file(L, N, b"".join(ref), nnz=None, comment=b"% a ref header of another length " * 3)
    m = mt.read_pair(a_bytes, r_bytes)
    assert m == mt.Matrix(L, N, entries)
    o = oracle_lib.Oracle.from_mtx(*_write(tmp_path, "pad", a_bytes, r_bytes), 0, 0)
    assert (o.total_loci, o.total_cells, o.loci_used, o.nnz) == (L, N, L, len(entries))
    assert _oracle_rows(o) == mt.per_cell(m.entries, N)
    o.close()


def test_the_oracle_refuses_exactly_the_files_the_reference_calls_parse_or_index0(oracle_lib, tmp_path):
    L, N = 50, 40
    entries = mt.locus_major_entries(L, N, 300, seed=6)
    lengths = [random.Random(k).choice((None, 31, 64, 150)) for k in range(len(entries))]
    alt0, ref0 = mt.build_sections(entries, lengths, seed=2)
    cases = {   # name: (which file, line, replacement, the reference's answer)
        "valid": (None, 0, b"", None),
        "float": ("alt", 17, b"1 1 1.0\n", ("parse", 17)),
        "blank": ("alt", 120, b"\n", ("parse", 120)),
        "blank_cr": ("ref", 121, b"  \r\n", ("parse", 121)),
        "two_tokens": ("alt", 299, b"1 1\n", ("parse", 299)),
        "ref_two_tokens": ("ref", 0, b"1    1 \n", ("parse", 0)),
        "negative": ("alt", 5, b"1 -1 1\n", ("parse", 5)),
        "ref_count_hex": ("ref", 77, b"1 1 0x10\n", ("parse", 77)),
        "glued_by_0x1f": ("alt", 9, b"1\x1f1 1\n", ("parse", 9)),
        "locus0": ("alt", 33, b"0 1 1\n", ("index0", 33)),
        "cell0": ("alt", 298, b"  1 +000 1\n", ("index0", 298)),
        "ref_indices_0_are_not_read": ("ref", 33, b"0 0 1\n", None),
        "count_65535": ("alt", 3, b"1 1 65535\n", None),
    }
    for name, (which, k, line, want) in cases.items():
        alt, ref = list(alt0), list(ref0)
        if which == "alt":
            alt[k] = line
        elif which == "ref":
            ref[k] = line
        a_bytes, r_bytes = mt.mtx_file(L, N, b"".join(alt)), mt.mtx_file(L, N, b"".join(ref))
        got = mt.read_pair(a_bytes, r_bytes)
        paths = _write(tmp_path, name, a_bytes, r_bytes)
        if want is None:
            assert isinstance(got, mt.Matrix), name
            o = oracle_lib.Oracle.from_mtx(*paths, 0, 0)
            assert _oracle_rows(o) == mt.per_cell(got.entries, N), name
            o.close()
        else:
            assert got == mt.TextError(*want), name
            with pytest.raises(RuntimeError) as ei:
                oracle_lib.Oracle.from_mtx(*paths, 0, 0)
            hit = re.search(r"cannot parse mtx entry (\d+):", str(ei.value))
            assert hit and int(hit.group(1)) == want[1], (name, str(ei.value))
    # the oracle reads line by line, so with several bad lines it stops at the first of either kind; the reference's (the
    # device's) precedence reports the first line that does not parse — the same FILES are refused
    alt = list(alt0)
    alt[10], alt[20] = b"0 1 1\n", b"x\n"
    a_bytes, r_bytes = mt.mtx_file(L, N, b"".join(alt)), mt.mtx_file(L, N, b"".join(ref0))
    assert mt.read_pair(a_bytes, r_bytes) == mt.TextError("parse", 20)
    with pytest.raises(RuntimeError, match="cannot parse mtx entry 10:"):
        oracle_lib.Oracle.from_mtx(*_write(tmp_path, "two_kinds", a_bytes, r_bytes), 0, 0)
    # a bad line beyond the shorter file: both load
    alt = list(alt0) + [b"x\n"]
    a_bytes = mt.mtx_file(L, N, b"".join(alt))
    got = mt.read_pair(a_bytes, r_bytes)
    o = oracle_lib.Oracle.from_mtx(*_write(tmp_path, "beyond", a_bytes, r_bytes), 0, 0)
    assert _oracle_rows(o) == mt.per_cell(got.entries, N)
    o.close()
