"""The text contract of the alt.mtx / ref.mtx pair in plain Python, on bytes — and a builder of files with exact line lengths.

No project code is used here: this is a restatement of what the reference reads (load_data.rs:190-223, SURVEY's quirk
list), to hold the device tokeniser (csrc/kernels_parse.hip) and the oracle's reader against.

The contract
  Header   three lines are consumed from each file, whatever they hold.  The dims are tokens 0 and 1 of the REF file's third
           line; the third number (the entry count) is never trusted.
  Lines    the rest of a file is split at b"\\n".  A final line without b"\\n" counts; nothing follows a final b"\\n".
  Tokens   a line is split at ASCII whitespace only (space, \\t, \\r, \\n, \\f, \\v: bytes.split(), not str.split(), which also
           splits at 0x1c-0x1f).  ALT tokens 0, 1, 2 are locus, cell (both 1-based) and alt count; REF token 2 is the ref count,
           REF tokens 0 and 1 are never looked at; further tokens are ignored.  A token is an optional '+' and one or more
           ASCII digits; leading zeros are fine.
  Zip      entry i is line i of both files; the zip stops at the shorter file.
  Errors   parse         a needed token is missing or malformed in either file (a blank line included), or above 2^32 - 1;
           index0        locus or cell token 0 (the reference's `tok - 1` underflows);
           locus_range   locus above the REF header's first number;   cell_range   cell above its second number;
           count_range   alt or ref count above 65535 (the staged counts are 16 bits wide);
           the four range kinds are checked in that order per entry.
  Precedence (the device's documented behaviour: the tokeniser runs over both files before the zip validates the entries)
           the smallest entry that does not parse, among the first min(lines) entries, wins over ANY range error, also an
           earlier one; otherwise the smallest range-offending entry wins, with its own kind.  A bad line at or beyond the
           shorter file's line count is never read and is no error.

Not covered: Unicode whitespace and bytes that are not UTF-8 (the Rust reader treats them differently from an ASCII
tokeniser).  The .gz readers: tests/test_host_mtx_bytes.py.
"""
import random
from collections import namedtuple

U32_MAX = 0xFFFFFFFF
MAX_COUNT = 65535
KINDS = ("parse", "index0", "locus_range", "cell_range", "count_range")

TextError = namedtuple("TextError", "kind entry")   # entry: 0-based position in the zip; None for the size line
Matrix = namedtuple("Matrix", "total_loci total_cells entries")   # entries: [(locus0, cell0, alt, ref), ...] in file order


# ---- reading --------------------------------------------------------------------------------------------------------------
def split_header(data):
    """(third line, data section) of one file: three lines consumed, a missing one is empty"""
    pos, third = 0, b""
    for x in range(3):
        nl = data.find(b"\n", pos)
        end = len(data) if nl < 0 else nl
        if x == 2:
            third = data[pos:end]
        pos = len(data) if nl < 0 else nl + 1
    return third, data[pos:]


def data_lines(section):
    """lines of a data section without their b"\\n": a final unterminated line counts, nothing follows a final b"\\n\""""
    parts = section.split(b"\n")
    if parts[-1] == b"":
        parts.pop()
    return parts


def token_value(tok, limit=U32_MAX):
    """parse::<usize>() of one token, None if it is no number or above `limit`"""
    if tok[:1] == b"+":
        tok = tok[1:]
    if not tok or any(ch < 0x30 or ch > 0x39 for ch in tok):
        return None
    v = int(tok)
    return v if v <= limit else None


def alt_line(line):
    """(locus1, cell1, alt) or None"""
    t = line.split()
    if len(t) < 3:
        return None
    v = tuple(token_value(x) for x in t[:3])
    return None if None in v else v


def ref_line(line):
    """ref count or None: token 2 only, tokens 0 and 1 may be anything"""
    t = line.split()
    return token_value(t[2]) if len(t) >= 3 else None


def range_kind(locus1, cell1, alt, ref, total_loci, total_cells):
    if locus1 == 0 or cell1 == 0:
        return "index0"
    if locus1 > total_loci:
        return "locus_range"
    if cell1 > total_cells:
        return "cell_range"
    if alt > MAX_COUNT or ref > MAX_COUNT:
        return "count_range"
    return None


def read_pair(alt_bytes, ref_bytes):
    """Matrix(total_loci, total_cells, entries) or the first error, TextError(kind, entry), of an alt / ref pair of whole files"""
    _, alt_sec = split_header(alt_bytes)
    third, ref_sec = split_header(ref_bytes)
    t = third.split()
    dims = [token_value(x, limit=(1 << 64) - 1) for x in t[:2]]
    if len(dims) < 2 or None in dims:
        return TextError("size_line", None)
    total_loci, total_cells = dims
    la, lr = data_lines(alt_sec), data_lines(ref_sec)
    n = min(len(la), len(lr))
    parsed = []
    for i in range(n):
        a, r = alt_line(la[i]), ref_line(lr[i])
        if a is None or r is None:
            return TextError("parse", i)
        parsed.append(a + (r,))
    for i, (l1, c1, a, r) in enumerate(parsed):
        kind = range_kind(l1, c1, a, r, total_loci, total_cells)
        if kind:
            return TextError(kind, i)
    return Matrix(total_loci, total_cells, [(l1 - 1, c1 - 1, a, r) for l1, c1, a, r in parsed])


def per_cell(entries, total_cells, cell_begin=0, cell_end=None):
    """[[(locus0, alt, ref), ...] in file order] for the cells [cell_begin, cell_end)"""
    cell_end = total_cells if cell_end is None else cell_end
    rows = [[] for _ in range(cell_end - cell_begin)]
    for l0, c0, a, r in entries:
        if cell_begin <= c0 < cell_end:
            rows[c0 - cell_begin].append((l0, a, r))
    return rows


# ---- writing --------------------------------------------------------------------------------------------------------------
_BLANKS = b"    \t\t\r\f\v"   # what the padding between tokens is drawn from in the "mix" style (mostly spaces)


def _blank_run(n, rng, style):
    if n == 0:
        return b""
    if style == "blanks" or n > 64:   # a long run: spaces, a few others at random places
        run = bytearray(b" " * n)
        if style != "blanks":
            for _ in range(4):
                run[rng.randrange(n)] = _BLANKS[rng.randrange(len(_BLANKS))]
        return bytes(run)
    return bytes(_BLANKS[rng.randrange(len(_BLANKS))] for _ in range(n))


def build_line(tokens, length, rng, style="mix", terminated=True):
    """One line of exactly `length` bytes (its b"\\n" included if `terminated`) whose first three whitespace-separated tokens
    read as `tokens` (numbers, or bytes taken as they are).  The bytes beyond the shortest spelling are a seeded mix of
    blanks before / between / after the tokens, leading zeros, '+', a b"\\r" before the b"\\n" and a trailing fourth token;
    style "blanks": spaces only, before / between / after.  ValueError if the tokens need more than `length` bytes."""
    toks = [t if isinstance(t, bytes) else b"%d" % t for t in tokens]
    numeric = [not isinstance(t, bytes) for t in tokens]
    need = sum(len(t) for t in toks) + (len(toks) - 1) + (1 if terminated else 0)
    pad = length - need
    if pad < 0:
        raise ValueError("a line of %d bytes cannot hold %r (%d needed)" % (length, tokens, need))
    cr, extra = b"", b""
    if style == "mix":
        if pad >= 1 and terminated and rng.random() < 0.3:
            cr, pad = b"\r", pad - 1
        for k in range(len(toks)):
            if numeric[k] and pad >= 1 and rng.random() < 0.2:
                toks[k], pad = b"+" + toks[k], pad - 1
        if pad >= 2 and rng.random() < 0.4:
            m = rng.randint(1, min(pad - 1, 12))
            extra = b" " + bytes(rng.choice(b"0123456789xyz.-+%") for _ in range(m))
            pad -= m + 1
        for k in range(len(toks)):
            if numeric[k] and pad >= 1 and rng.random() < 0.4:
                z = rng.randint(1, min(pad, 20))
                sign = toks[k][:1] if toks[k][:1] == b"+" else b""
                toks[k], pad = sign + b"0" * z + toks[k][len(sign):], pad - z
    # the rest: blanks in the slots before, between and after the tokens
    slots = len(toks) + 1
    cuts = sorted(rng.randint(0, pad) for _ in range(slots - 1))
    runs = [b - a for a, b in zip([0] + cuts, cuts + [pad])]
    out = bytearray()
    for k, t in enumerate(toks):
        out += _blank_run(runs[k] + (1 if k else 0), rng, style)
        out += t
    if extra:   # (the fourth token goes behind the trailing blanks' first half)
        half = runs[-1] // 2
        out += _blank_run(half, rng, style) + extra + _blank_run(runs[-1] - half, rng, style)
    else:
        out += _blank_run(runs[-1], rng, style)
    out += cr + (b"\n" if terminated else b"")
    assert len(out) == length
    return bytes(out)


def min_length(tokens, terminated=True):
    """the shortest line that holds the tokens"""
    return sum(len(t if isinstance(t, bytes) else b"%d" % t) for t in tokens) + len(tokens) - 1 + (1 if terminated else 0)


def build_sections(entries, lengths, seed, style="mix", terminated=True, ref_lengths=None):
    """(alt lines, ref lines): lists of the data sections' lines for `entries` [(locus0, cell0, alt, ref), ...]; line k of the
    alt file has exactly lengths[k] bytes and line k of the ref file ref_lengths[k] (default: the same), terminator included
    — None: the shortest spelling.  The ref file's index tokens are the alt file's, or junk (they are never read).
    terminated=False leaves the last line of both files without its b"\\n" (its length then counts none).
    b"".join(lines) is the data section; a test that plants a malformed line replaces a list element."""
    rng = random.Random(seed)
    ref_lengths = lengths if ref_lengths is None else ref_lengths
    if len(lengths) != len(entries) or len(ref_lengths) != len(entries):
        raise ValueError("one length per entry")
    alt_lines, ref_lines = [], []
    for k, (l0, c0, a, r) in enumerate(entries):
        term = terminated or k + 1 < len(entries)
        ta = (l0 + 1, c0 + 1, a)
        junk = rng.random()
        tr = (l0 + 1, c0 + 1, r) if junk < 0.7 else (b"x", b"0", r) if junk < 0.8 else (rng.randrange(10 ** 6), b"-1", r) if junk < 0.9 else (b"%", c0 + 1, r)
        la = min_length(ta, term) if lengths[k] is None else lengths[k]
        lr = min_length(tr, term) if ref_lengths[k] is None else ref_lengths[k]
        if lr < min_length(tr, term):
            tr = (b"x", b"0", r)   # (the shortest spelling; still too long: build_line raises)
        alt_lines.append(build_line(ta, la, rng, style, term))
        ref_lines.append(build_line(tr, lr, rng, style, term))
    return alt_lines, ref_lines


class LayoutError(ValueError):
    """plan_lengths cannot realise the layout; .entry: the entry whose line is too short for it, if that is the reason"""

    def __init__(self, message, entry=None):
        super().__init__(message)
        self.entry = entry


def entry_min_length(entry):
    """the shortest line, newline included, that holds the entry in the alt file AND in the ref file"""
    l0, c0, a, r = entry
    return max(min_length((l0 + 1, c0 + 1, a)), min_length((b"x", b"0", r)))


def plan_lengths(entries, anchors=(), end=None, seed=0, slack=4):
    """Line lengths (for build_sections) that put lines at exact byte offsets of the data section.
    anchors: [(start, length or None), ...], ascending: a line starts exactly at offset `start` — the newline before it sits
    on start - 1 — and is `length` bytes long (None: its shortest spelling plus up to `slack` bytes, like every other line).
    end: the data section is exactly `end` bytes long; entries that do not fit any more are left out (None: all of them).
    The line in front of an anchor is stretched to reach it.  LayoutError (a ValueError) if the layout cannot be realised: a
    test that asks for an impossible one has to fail, not to run on something else."""
    rng = random.Random(seed)
    stops = [(s, n) for s, n in anchors] + ([(end, None)] if end is not None else [])
    if any(b[0] <= a[0] for a, b in zip(stops, stops[1:])):
        raise LayoutError("anchors must ascend (and lie before the end)")
    lengths, cum, ai = [], 0, 0
    for k, e in enumerate(entries):
        if end is not None and cum == end:
            break
        ml = entry_min_length(e)
        ln, fixed = ml + rng.randint(0, slack), False
        if ai < len(anchors) and cum == anchors[ai][0]:
            if anchors[ai][1] is not None:
                ln, fixed = anchors[ai][1], True
            ai += 1
        if ln < ml:
            raise LayoutError("entry %d needs %d bytes, the anchor at %d gives it %d" % (k, ml, cum, ln), entry=k)
        if ai < len(stops):
            nxt = stops[ai][0]
            nml = entry_min_length(entries[k + 1]) if k + 1 < len(entries) else 1 << 62
            gap = nxt - (cum + ln)
            if gap < 0 or 0 < gap < nml:
                if fixed or nxt - cum < ml:
                    raise LayoutError("cannot reach offset %d from the line of %d bytes at %d" % (nxt, ln, cum))
                ln = nxt - cum
        lengths.append(ln)
        cum += ln
    if ai < len(anchors) or (end is not None and cum != end):
        raise LayoutError("the entries ran out at offset %d before every anchor / the end was reached" % cum)
    return lengths


def mtx_file(total_loci, total_cells, section, nnz=0, comment=b"%"):
    """a whole file: banner, one comment line, size line (nnz None: no third number), data section"""
    size = b"%d %d" % (total_loci, total_cells) + (b"" if nnz is None else b" %d" % nnz)
    return b"%%MatrixMarket matrix coordinate integer general\n" + comment + b"\n" + size + b"\n" + section


def locus_major_entries(total_loci, total_cells, n, seed, max_count=300):
    """n entries in locus-major order (as vartrix writes them: row order inside a cell is then file order), every locus and
    (almost) every cell hit, a (locus, cell) pair possibly listed twice, counts 0 .. max_count with a few at 65535"""
    rng = random.Random(seed)
    loci = sorted(rng.randrange(total_loci) for _ in range(n))
    out = []
    for l0 in loci:
        a = MAX_COUNT if rng.random() < 0.01 else rng.randint(0, max_count)
        r = MAX_COUNT if rng.random() < 0.01 else rng.randint(0, max_count)
        out.append((l0, rng.randrange(total_cells), a, r))
    return out
