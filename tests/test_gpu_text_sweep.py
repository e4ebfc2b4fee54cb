"""GPU: the device text tokeniser (csrc/kernels_parse.hip: k_nl_count, k_parse_lines, k_pair_check / k_pair_fill / k_pair_take,
parse_whole, parse_windowed, the split ingest) swept over its geometry against tests/mtx_text_reference.py.

The tokeniser's dispatch geometry: 16-byte units (newline_mask16: a vector branch and a bytewise one for the last unit),
128-byte segments (NL_SEG: a thread takes the lines that START in its segment, the one on the next segment's first byte
included), blocks of 256 segments = 32768 bytes staged in LDS with a tail of 64 bytes (PARSE_TAIL; a line the tail does not
close is read from global memory), windows with a look-ahead of PW_LOOK bytes, a padding newline behind an unterminated last
line, token arrays that grow, and the first / more protocol between windows.  The files here are made by the reference's
builder, which gives every line an exact byte length, so that lines and newlines sit ON those edges instead of near them.

Every file goes through three paths — the whole file on the device (option parse_window 0), windows (parse_window from
WINDOWS) and windows of a file that is never mapped (CELLECTOR_UNMAPPED_MIN=1) — and is compared with the reference's reading
of the same bytes as exact integers: dims, every cell's (locus, alt, ref) list in file order (the files are locus-major, so
row order is file order), or status, entry number and kind of the first error.  No tolerances, nothing is skipped; a layout
the builder cannot realise raises.

The sizes are the smallest that cross every edge: data sections of 70-100 KB (three blocks), a few thousand entries.
"""
import os
import re

import numpy as np
import pytest

import mtx_text_reference as mt

pytestmark = pytest.mark.gpu

WINDOWS = (512, 640, 32768, 32896, 65536)
BLOCK = 32768            # PB * NL_SEG
PW_LOOK = 1 << 20        # csrc/kernels_parse.hip, #define PW_LOOK: the longest line a windowed file may hold
STATUS = {"parse": 3, "index0": 1, "locus_range": 1, "cell_range": 1, "count_range": 1}
PHRASE = {"index0": "index 0", "locus_range": "locus index out of range", "cell_range": "cell index out of range",
          "count_range": "count above 65535"}
L, N = 300, 200


@pytest.fixture(scope="module")
def mods(oracle_lib, hip_lib_path):
    from cellector_amd import Cellector, ffi
    return dict(Cellector=Cellector, ffi=ffi, ob=oracle_lib)


@pytest.fixture(scope="module")
def base_entries():
    return mt.locus_major_entries(L, N, 8000, seed=11)


# ---- one load, one comparison ------------------------------------------------------------------------------------------------
class Case:
    """a pair of files on disk and the reference's reading of their bytes (computed once)"""

    def __init__(self, tmp_path, name, alt_lines, ref_lines, total_loci=L, total_cells=N, nnz=0, alt_nnz=0):
        a_bytes = mt.mtx_file(total_loci + 7, total_cells + 7, b"".join(alt_lines), nnz=alt_nnz)   # (the alt header's dims are not read)
        r_bytes = mt.mtx_file(total_loci, total_cells, b"".join(ref_lines), nnz=nnz, comment=b"% a ref header of another length")
        self.name = name
        self.alt, self.ref = str(tmp_path / (name + "_alt.mtx")), str(tmp_path / (name + "_ref.mtx"))
        with open(self.alt, "wb") as f:
            f.write(a_bytes)
        with open(self.ref, "wb") as f:
            f.write(r_bytes)
        self.want = mt.read_pair(a_bytes, r_bytes)
        self.alt_data, self.ref_data = len(b"".join(alt_lines)), len(b"".join(ref_lines))
        self._rows = {}

    def rows(self, cb=0, ce=None):
        """(row_ptr, locus, alt, ref) of the cells [cb, ce) in file order, as arrays"""
        ce = self.want.total_cells if ce is None else ce
        if (cb, ce) not in self._rows:
            per = mt.per_cell(self.want.entries, self.want.total_cells, cb, ce)
            rp = np.cumsum([0] + [len(r) for r in per]).astype(np.uint64)
            flat = np.array([x for r in per for x in r], dtype=np.uint64).reshape(-1, 3)
            self._rows[(cb, ce)] = (rp, flat[:, 0], flat[:, 1], flat[:, 2])
        return self._rows[(cb, ce)]


def _device_rows(g, n_rows):
    rp, ent = g.csr_rows(0, n_rows)
    ids = g.locus_ids()
    return rp, ids[(ent & np.uint64(0xffffffff)).astype(np.int64)], (ent >> np.uint64(32)) & np.uint64(0xffff), ent >> np.uint64(48)


def _load(g, case, window, unmapped, call):
    g.set_option("parse_window", window)
    if unmapped:
        os.environ["CELLECTOR_UNMAPPED_MIN"] = "1"
    try:
        call(g, case.alt, case.ref)
    finally:
        os.environ.pop("CELLECTOR_UNMAPPED_MIN", None)


def _check(mods, g, case, window=0, unmapped=False, shard=None, expect=None):
    """load the case through one path and compare with the reference (expect: an answer that differs by path, PW_LOOK)"""
    want = case.want if expect is None else expect
    where = (case.name, "window %d" % window, "unmapped" if unmapped else "mapped", shard)
    if shard is None:
        call = lambda g, a, r: g.load_mtx(a, r, 0, 0)
    else:
        def call(g, a, r):
            g.ingest_mtx(a, r)
            g.ingest_finish(0, 0)
    if isinstance(want, mt.TextError):
        with pytest.raises(mods["ffi"].CellectorError) as ei:
            _load(g, case, window, unmapped, call)
        msg = str(ei.value)
        hit = re.search(r"entry (\d+)", msg)
        assert hit, (where, msg)
        assert (ei.value.status, int(hit.group(1))) == (STATUS[want.kind], want.entry), (where, want, msg)
        if want.kind != "parse":
            assert PHRASE[want.kind] in msg, (where, want, msg)
        return
    _load(g, case, window, unmapped, call)
    cb, ce = shard if shard else (0, want.total_cells)
    d = g.dims()
    assert (d.total_loci, d.total_cells, d.loci_used, d.cell_begin, d.cell_end) == (want.total_loci, want.total_cells, want.total_loci, cb, ce), where
    rp, lo, al, re_ = case.rows(cb, ce)
    assert d.nnz_used == len(lo), where
    g_rp, g_lo, g_al, g_re = _device_rows(g, ce - cb)
    assert np.array_equal(g_rp, rp), where
    for got, exp, what in ((g_lo, lo, "locus"), (g_al, al, "alt"), (g_re, re_, "ref")):
        if not np.array_equal(got, exp):
            bad = np.flatnonzero(got != exp)
            raise AssertionError("%s: %s differs at %d of %d staged entries, first at %d: device %d, reference %d"
                                 % (where, what, len(bad), len(exp), bad[0], got[bad[0]], exp[bad[0]]))


def _all_paths(mods, g, case, windows=WINDOWS, unmapped_windows=WINDOWS):
    _check(mods, g, case)
    for w in windows:
        _check(mods, g, case, w)
    for w in unmapped_windows:
        _check(mods, g, case, w, unmapped=True)


# ---- the planted layouts -----------------------------------------------------------------------------------------------------
def _newline_on(*offsets):
    """anchors that put a newline exactly on each of the data offsets: a line starts on the byte behind it"""
    return [(o + 1, None) for o in offsets]


# Three layouts, because a newline on byte 15 and one on byte 16 cannot share a file (no line is one byte long), nor can lines
# that start 63, 64 and 65 bytes in front of the same block edge.  Together they hold, at the block edges 32768, 65536, 98304:
#   a line that starts k = 65 / 64 / 63 bytes in front of an edge, 10 bytes long (it ends inside the staged tail) and 200 bytes
#   long (the tail does not close it: global fall-back); a line that starts on a block's last byte (k = 1), 10 and 200 bytes;
#   a newline ON a block's last byte (32767, 65535) and ON the next block's first byte (32768, 65536);
# and in front of them lines of exactly 63, 64, 65, 128, 129, 256 and 5000 bytes (the long ones leave runs of segments without
# a newline), a line of 1100 bytes over three windows of 512, and a newline on the last byte of a window / the first byte of
# the next one for the windows 512, 640 and 32896 (32768 and 65536 are block edges).
def planted_anchors(variant):
    k = (65, 64, 63)[variant]
    e1, e2, e3 = BLOCK, 2 * BLOCK, 3 * BLOCK
    a = _newline_on(*[(15, 127), (16, 128), (15, 128)][variant])
    at = 256
    for size in (63, 64, 65, 128, 129, 256):
        a.append((at, size))
        at += size
    a += _newline_on(1023, 1279) + [(1500, 1100)] + _newline_on(3072, 3200)
    a.append((e1 - k, 10))
    if variant == 0:
        a += [(e1 - 1, 200), (e2 - 64, 200), (e3 - 1, 10)]
    elif variant == 1:
        a += _newline_on(e1, 32896, e2) + [(e3 - 63, 200)]
    else:
        a += _newline_on(e1 - 1, 32895, e2 - 1) + [(e3 - 65, 200)]
    a.append((40000, 5000))
    return sorted(a)


PLANTED_BYTES = 100000


def planted_lines(entries, variant, terminated=True):
    """(alt lines, ref lines, lengths) of the planted layout"""
    entries = list(entries)
    for _ in range(16):   # an entry that lands on a 10-byte anchor gets tokens that fit (same locus: the file stays locus-major)
        try:
            lengths = mt.plan_lengths(entries, planted_anchors(variant), end=PLANTED_BYTES, seed=20 + variant)
            break
        except mt.LayoutError as e:
            if e.entry is None:
                raise
            l0, c0, a, r = entries[e.entry]
            if (c0, a, r) == (c0 % 9, a % 10, r % 10):
                raise
            entries[e.entry] = (l0, c0 % 9, a % 10, r % 10)
    alt, ref = mt.build_sections(entries[:len(lengths)], lengths, seed=30 + variant, terminated=terminated)
    return alt, ref, lengths


def planted_case(tmp_path, entries, variant, name=None, terminated=True):
    alt, ref, lengths = planted_lines(entries, variant, terminated)
    return Case(tmp_path, name or "planted%d" % variant, alt, ref), lengths


def newline_offsets(lines):
    out, at = [], 0
    for ln in lines:
        at += len(ln)
        out.append(at - 1)
    return out


# ---- tests -------------------------------------------------------------------------------------------------------------------
def test_planted_edges(mods, tmp_path, base_entries):
    """Newlines exactly on data offsets 15 / 16, 127 / 128, 32767 / 32768, 65535 / 65536 and on the last / first byte of every
    window size; lines that start 1, 63, 64, 65 bytes in front of a block edge, 10 bytes long (they end in the staged tail)
    and 200 bytes long (global fall-back); lines of exactly 63, 64, 65, 128, 129, 256 and 5000 bytes; runs of segments
    without a newline; a line that spans three windows of 512.  The layout is asserted before anything is loaded."""
    g = mods["Cellector"](0)
    seen_nl, seen_len, seen_start = set(), set(), set()
    for variant in range(3):
        case, lengths = planted_case(tmp_path, base_entries, variant)
        assert isinstance(case.want, mt.Matrix) and len(case.want.entries) == len(lengths) > 3000
        assert case.alt_data == case.ref_data == PLANTED_BYTES
        nl = newline_offsets([b"x" * n for n in lengths])
        seen_nl |= set(nl)
        seen_len |= set(lengths)
        starts = [0] + [o + 1 for o in nl[:-1]]
        seen_start |= {(e - s, n) for s, n in zip(starts, lengths) for e in (BLOCK, 2 * BLOCK, 3 * BLOCK) if 0 < e - s <= 65}
        assert any(a // 128 + 3 <= b // 128 for a, b in zip(nl, nl[1:]))   # segments without any newline
        assert any((a + 1) // 512 + 2 <= b // 512 and b - a < 1200 for a, b in zip(nl, nl[1:]))   # a line over three windows of 512
        _all_paths(mods, g, case)
    assert {15, 16, 127, 128, BLOCK - 1, BLOCK, 2 * BLOCK - 1, 2 * BLOCK} <= seen_nl
    for w in WINDOWS:   # a newline on the last byte of a window and on the first byte of the next one
        assert any((o + 1) % w == 0 for o in seen_nl) and any(o % w == 0 for o in seen_nl), w
    assert {63, 64, 65, 128, 129, 256, 5000} <= seen_len
    for k in (1, 63, 64, 65):
        assert (k, 10) in seen_start and (k, 200) in seen_start, (k, sorted(seen_start))
    g.close()


def test_alignment_sweep(mods, tmp_path, base_entries):
    """One planted file, its first line lengthened by s blanks, s in 0..17, 62..66, 126..130: every later newline visits
    every residue of 16 and the listed residues of 128 (and the lines in front of the block edges slide over them).  Every s
    on the whole-file path, a subset on the windowed paths."""
    g = mods["Cellector"](0)
    shifts = list(range(0, 18)) + list(range(62, 67)) + list(range(126, 131))
    windowed = {1: WINDOWS, 15: WINDOWS, 16: WINDOWS, 17: (512, 32768), 63: WINDOWS, 64: WINDOWS, 65: (640, 65536), 127: WINDOWS,
                128: WINDOWS, 129: (512, 32896)}
    first = None
    alt, ref, _ = planted_lines(base_entries, 0)
    for i, s in enumerate(shifts):
        case = Case(tmp_path, "shift%d" % s, [b" " * s + alt[0]] + alt[1:], [b" " * s + ref[0]] + ref[1:])
        first = first or case.want
        assert case.want == first   # (blanks in front of a line change no entry)
        _check(mods, g, case)
        for w in windowed.get(s, ()):
            _check(mods, g, case, w)
        if s in windowed:
            _check(mods, g, case, WINDOWS[i % len(WINDOWS)], unmapped=True)
        os.remove(case.alt), os.remove(case.ref)
    g.close()


def small_entries(n, seed):
    """entries whose shortest line is "1 1 1\\n": six bytes"""
    import random
    rng = random.Random(seed)
    loci = sorted(rng.randrange(9) for _ in range(n))
    return [(l0, rng.randrange(7), rng.randrange(10), rng.randrange(10)) for l0 in loci]


def ends_cases(tmp_path):
    """short files for every way a data section can end"""
    ent = small_entries(400, seed=3)
    cases = []

    def add(name, alt, ref, **kw):
        cases.append(Case(tmp_path, "end_" + name, alt, ref, total_loci=9, total_cells=7, **kw))

    # data lengths around a unit (1600 = 100 units; 1536 and 1280 are whole windows of 512 and 640 too) and tiny sections
    for total in (1599, 1600, 1601, 1615, 1616, 1617, 1536, 1537, 1280, 1281, 1535, 15, 16, 17, 31, 32, 33, 6):
        for terminated in (True, False):
            lengths = mt.plan_lengths(ent, end=total, seed=total)
            alt, ref = mt.build_sections(ent[:len(lengths)], lengths, seed=total, terminated=terminated)
            assert len(b"".join(alt)) == len(b"".join(ref)) == total
            add("%d_%s" % (total, "t" if terminated else "u"), alt, ref)
    # one line only: of 6 bytes, of 15 (a byte short of a unit), of 16, of 70 (longer than the tail), with and without newline
    for n in (6, 15, 16, 17, 63, 64, 65, 70, 200):
        for terminated in (True, False):
            alt, ref = mt.build_sections(ent[:1], [n], seed=n, terminated=terminated)
            add("one_%d_%s" % (n, "t" if terminated else "u"), alt, ref)
    # the last 64 bytes hold 1, 2 and 10 lines (a line that starts there cannot be read from the staged tail)
    for total in (1600, 1000):
        for terminated in (True, False):
            for name, tail in (("1", [(total - 70, 70)]), ("2", [(total - 64, 40), (total - 24, 24)]),
                               ("10", [(total - 60 + 6 * j, 6) for j in range(10)])):
                lengths = mt.plan_lengths(ent, tail, end=total, seed=7)
                alt, ref = mt.build_sections(ent[:len(lengths)], lengths, seed=total, terminated=terminated)
                add("tail%s_%d_%s" % (name, total, "t" if terminated else "u"), alt, ref)
    # files of different line counts: by one line and by a third, either way; different lengths line by line as well
    lengths = mt.plan_lengths(ent[:300], seed=5)
    ref_lengths = mt.plan_lengths(ent[:300], seed=6, slack=9)
    alt, ref = mt.build_sections(ent[:300], lengths, seed=5, ref_lengths=ref_lengths)
    for name, na, nr in (("alt_short1", 299, 300), ("ref_short1", 300, 299), ("alt_short_third", 200, 300), ("ref_short_third", 300, 200)):
        add(name, alt[:na], ref[:nr])
        add(name + "_u", alt[:na - 1] + [alt[na - 1].rstrip(b"\n")], ref[:nr - 1] + [ref[nr - 1].rstrip(b"\r\n")])
    # a lying entry count on the size line: absent, 1 (the token arrays grow through several windows), far too large
    for name, nnz in (("nnz_absent", None), ("nnz_1", 1), ("nnz_huge", 10 ** 15), ("nnz_plausible_but_big", 500)):
        add(name, alt, ref, nnz=nnz, alt_nnz=nnz)
    return cases


def test_ends_of_the_data(mods, tmp_path):
    """Terminated and unterminated; data lengths = 0, 1, 15 mod 16 and = 0, 1 mod the window, sections of 15, 16, 17 bytes,
    of one line, and empty; the last 64 bytes holding 1, 2 and 10 lines; ALT shorter than REF and the reverse, by one line
    and by a third; an entry count on the size line that is absent, 1, or far larger than the file."""
    g = mods["Cellector"](0)
    cases = ends_cases(tmp_path)
    assert all(isinstance(c.want, mt.Matrix) and c.want.entries for c in cases)
    for i, case in enumerate(cases):
        _check(mods, g, case)
        _check(mods, g, case, 512)
        _check(mods, g, case, (640, 32768)[i % 2], unmapped=i % 3 == 0)
        _check(mods, g, case, 512, unmapped=True)
    # an empty data section (both files, or one of them): no entries, every locus kept by min_alt = min_ref = 0
    ent = small_entries(5, seed=1)
    alt, ref = mt.build_sections(ent, [None] * 5, seed=1)
    for name, a, r in (("both", [], []), ("alt", [], ref), ("ref", alt, [])):
        case = Case(tmp_path, "empty_" + name, a, r, total_loci=9, total_cells=7)
        assert case.want == mt.Matrix(9, 7, [])
        _check(mods, g, case)
        _check(mods, g, case, 512)
        _check(mods, g, case, 512, unmapped=True)
    g.close()


def test_pw_look_both_sides(mods, tmp_path):
    """A windowed file may hold lines of up to PW_LOOK bytes (the look-ahead behind a window; 2^20, from csrc/kernels_parse.hip).
    The line that needs all of it starts on the last position a window owns — right behind a newline on the window's last
    byte — and is PW_LOOK bytes long with its newline: it loads on every path.  One byte more and the windowed paths refuse
    it, with a parse error at that line's entry number; the whole-file path has no such limit and loads it."""
    W = 65536
    ent = mt.locus_major_entries(L, N, 6000, seed=12)
    g = mods["Cellector"](0)
    for name, extra_alt, extra_ref in (("fits", 0, 0), ("alt_too_long", 1, 0), ("ref_too_long", 0, 1)):
        base = mt.plan_lengths(ent, [(W, 40)], seed=2)
        k = newline_offsets([b"x" * n for n in base]).index(W - 1) + 1   # the entry that starts on byte W
        la, lr = list(base), list(base)
        la[k] = PW_LOOK + extra_alt if (extra_alt or not extra_ref) else 40
        lr[k] = PW_LOOK + extra_ref if (extra_ref or not extra_alt) else 40
        n = k + 400
        assert n <= len(ent)
        alt_h, ref_h = mt.build_sections(ent[:k], base[:k], seed=1)
        alt_l, ref_l = mt.build_sections(ent[k:k + 1], la[k:k + 1], seed=1, style="blanks", ref_lengths=lr[k:k + 1])
        alt_t, ref_t = mt.build_sections(ent[k + 1:n], base[k + 1:n], seed=2)
        case = Case(tmp_path, "pwlook_" + name, alt_h + alt_l + alt_t, ref_h + ref_l + ref_t)
        assert sum(len(x) for x in alt_h) == sum(len(x) for x in ref_h) == W
        assert (len(alt_l[0]), len(ref_l[0])) == (la[k], lr[k]) and max(la[k], lr[k]) == PW_LOOK + (name != "fits")
        assert isinstance(case.want, mt.Matrix) and len(case.want.entries) == n
        refused = None if name == "fits" else mt.TextError("parse", k)
        _check(mods, g, case)
        _check(mods, g, case, W, expect=refused)
        _check(mods, g, case, W, unmapped=True, expect=refused)
    g.close()


def test_first_error(mods, tmp_path, base_entries):
    """Several bad lines far apart — other segments, blocks, windows, the other file: the smallest entry that does not parse
    wins; a malformed line at or behind the shorter file's line count is no error; a range error at entry i followed by
    many range errors of other kinds reports i with i's kind (one atomicMin carries entry and kind: the kind is the
    smallest entry's own, not the last writer's); a parse error beats an earlier range error (the stated precedence)."""
    g = mods["Cellector"](0)
    ent = base_entries[:6000]
    lengths = mt.plan_lengths(ent, seed=3)
    alt0, ref0 = mt.build_sections(ent, lengths, seed=4)
    nl = newline_offsets(alt0)
    b0, b1, b2 = (next(i for i, o in enumerate(nl) if o > x) for x in (9000, BLOCK + 9000, 2 * BLOCK + 3000))   # one entry per block
    assert nl[b2] < len(b"".join(alt0)) - 2000
    bad_range = {"index0": b"0 1 1\n", "locus_range": b"%d 1 1\n" % (L + 1), "cell_range": b"1 %d 1\n" % (N + 1), "count_range": b"1 1 65536\n"}
    malformed = (b"1 1 1.0\n", b"\n", b"1 1\n", b"1 -1 1\n", b"  \r\n", b"1 1 4294967296\n", b"x " * 40 + b"\n")
    cases = []

    def add(name, alt_edits, ref_edits, want, cut_alt=None, cut_ref=None):
        alt, ref = list(alt0), list(ref0)
        for k, line in alt_edits.items():
            alt[k] = line
        for k, line in ref_edits.items():
            ref[k] = line
        case = Case(tmp_path, "err_" + name, alt[:cut_alt], ref[:cut_ref])
        assert isinstance(case.want, mt.Matrix) if want is None else case.want == want, (name, case.want)
        cases.append(case)

    P = mt.TextError
    add("blocks", {b2: malformed[0], b1: malformed[1]}, {}, P("parse", b1))
    add("blocks_first", {b0: malformed[2], b1: malformed[3], b2: malformed[4]}, {}, P("parse", b0))
    add("files_ref_first", {b2: malformed[5], b1 + 1: malformed[6]}, {b1: b"1 1 x\n"}, P("parse", b1))
    add("files_alt_first", {b0 + 3: malformed[6]}, {b0 + 4: b"1 1\n", b2: b"\n"}, P("parse", b0 + 3))
    add("neighbours", {b1: malformed[1], b1 + 1: malformed[0]}, {b1 + 1: b"1\n"}, P("parse", b1))
    add("ref_indices_are_not_read", {}, {b0: b"0 0 1\n", b1: b"x -1 1 1.0\n", b2: b"99999 99999 1\n"}, None)
    add("last_line", {5999: malformed[2]}, {}, P("parse", 5999))
    add("first_line", {0: malformed[1], 5999: malformed[2]}, {}, P("parse", 0))
    # at or behind the shorter file's count nothing is read
    add("beyond_short_ref", {b2: malformed[0], 5990: bad_range["index0"]}, {}, None, cut_ref=b2)
    add("beyond_short_alt", {}, {b1: b"\n"}, None, cut_alt=b1)
    add("just_inside_short_ref", {b2: malformed[0]}, {}, P("parse", b2), cut_ref=b2 + 1)
    # range errors: the smallest entry, with its own kind, whatever comes after it in other waves, blocks and windows
    kinds = list(bad_range)
    for j, kind in enumerate(kinds):
        others = [x for x in kinds if x != kind]
        edits = {b0 + 1: bad_range[kind]}
        edits.update({i: bad_range[others[i % 3]] for i in range(b0 + 2, 6000, 2)})
        add("kind_" + kind, edits, {}, P(kind, b0 + 1))
    add("range_blocks", {b2: bad_range["index0"], b1: bad_range["count_range"]}, {}, P("count_range", b1))
    add("range_ref_count", {b2: bad_range["locus_range"]}, {b1: b"1 1 65536\n"}, P("count_range", b1))
    add("range_order_in_an_entry", {b1: b"0 %d 70000\n" % (N + 1), b2: b"%d %d 70000\n" % (L + 1, N + 1)}, {}, P("index0", b1))
    add("range_order_in_an_entry2", {b1: b"%d %d 70000\n" % (L + 1, N + 1)}, {}, P("locus_range", b1))
    add("range_order_in_an_entry3", {b1: b"%d %d 70000\n" % (L, N + 1)}, {}, P("cell_range", b1))
    # the stated precedence: the tokeniser runs first, a line that does not parse beats an EARLIER range error
    add("parse_beats_range", {b0: bad_range["cell_range"], b2: malformed[0]}, {}, P("parse", b2))
    add("parse_in_ref_beats_range", {b0: bad_range["index0"]}, {b1: b"1 1\n"}, P("parse", b1))
    for i, case in enumerate(cases):
        _check(mods, g, case)
        _check(mods, g, case, WINDOWS[i % 5])
        _check(mods, g, case, WINDOWS[(i + 2) % 5])
        _check(mods, g, case, WINDOWS[(i + 1) % 5], unmapped=True)
    g.close()


def test_shard_and_split_paths(mods, tmp_path, base_entries):
    """The planted file through the other routes out of the tokeniser: a ctx that holds a cell range (set_shard + ingest_mtx +
    ingest_finish: k_pair_fill and the keep scan — only cells in range are staged, with local cell indices), and the split
    ingest of a multi-device ctx (every shard tokenises a range of windows of both files: the same line arithmetic one
    level up), valid files and first errors."""
    case, _ = planted_case(tmp_path, base_entries, 0)
    case_u, _ = planted_case(tmp_path, base_entries, 1, name="planted1_u", terminated=False)
    for cb, ce in ((0, 37), (37, 151), (151, N), (93, 94)):
        for window, unmapped in ((0, False), (640, False), (512, True)):
            g = mods["Cellector"](0)
            g.set_shard(cb, ce)
            _check(mods, g, case if cb != 37 else case_u, window, unmapped, shard=(cb, ce))
            g.close()
    # errors on a ctx with a cell range: same entry, same kind
    ent = base_entries[:3000]
    alt, ref = mt.build_sections(ent, mt.plan_lengths(ent, seed=8), seed=8)
    alt_bad = list(alt)
    alt_bad[1500] = b"1 %d 1\n" % (N + 1)
    for i in range(1501, 3000, 3):
        alt_bad[i] = (b"0 1 1\n", b"1 1 70000\n")[i % 2]
    bad_range = Case(tmp_path, "split_range", alt_bad, ref)
    alt_bad = list(alt)
    alt_bad[2900], alt_bad[700] = b"x\n", b"0 1 1\n"
    ref_bad = list(ref)
    ref_bad[1700] = b"1 1\n"
    bad_parse = Case(tmp_path, "split_parse", alt_bad, ref_bad)
    assert bad_range.want == mt.TextError("cell_range", 1500) and bad_parse.want == mt.TextError("parse", 1700)
    g = mods["Cellector"](0)
    g.set_shard(37, 151)
    for bad in (bad_range, bad_parse):
        _check(mods, g, bad, 0, shard=(37, 151))
        _check(mods, g, bad, 640, shard=(37, 151))
    g.close()
    os.environ["CELLECTOR_MULTI_SPLIT"] = "1"
    try:
        m = mods["Cellector"](devices=[0, 0, 0])
        for c in (case, case_u, bad_range, bad_parse):
            _check(mods, m, c, 640)
        _check(mods, m, case, 512, unmapped=True)
        _check(mods, m, bad_range, 32768)
        m.close()
    finally:
        os.environ.pop("CELLECTOR_MULTI_SPLIT", None)
