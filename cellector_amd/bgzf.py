"""Host twin of cellector_bgzf_compress / cellector_write_mtx_bgzf (csrc/kernels_bgzf.hip, csrc/bgzf_format.h): bytes as a BGZF
stream (block-compressed gzip, what `bgzip` writes), by a compressor made for mtx text.  `compress(data)` is the contract: the
device's bytes equal it.

Blocks     The input is cut at multiples of PAYLOAD = 32640 bytes; every piece becomes one gzip member, then comes the 28-byte BGZF
           end-of-file member.  Empty input: that member alone.
Framing    18-byte header (1f 8b 08 04, MTIME 0, XFL 0, OS ff, XLEN 6, 'B' 'C' 02 00, BSIZE = member length - 1), one deflate block
           with BFINAL = 1, CRC-32 of the piece, ISIZE.
Tokens     Inside a block only.  Segments end behind each b"\\n"; segment 0 (what precedes the first newline) has no candidate.  For p
           in segment i >= 1, d(p) = the length of segment i - 1, so p - d(p) is the same column of the line before, and
           eq[p] = data[p] == data[p - d(p)].  A maximal run of positions with eq set and equal d becomes matches (len, d) in pieces of
           258 from the run's start; a last piece below 3 bytes becomes literals, like every position with eq clear.  No hash table, no
           serial parse: run starts and ends are scans.
Codes      BTYPE = 10 with the PRESET table of bgzf_preset.py (tools/bgzf_preset.py makes it): 286 + 30 code lengths, all in 1..15,
           both Kraft sums 1; the table's bits (HEADER) are the same constant string at the head of every block, so any inflater
           reads the table from the file and a later preset never breaks an old file.
Stored     A block whose preset deflate bytes are >= len(block) + 5 is a stored block (BTYPE = 00); a tie goes to stored.
"""
import struct
import zlib

import numpy as np

PAYLOAD = 32640
MAX_MATCH, MIN_MATCH = 258, 3
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
N_LITLEN, N_DIST = 286, 30

# deflate's length and distance symbols (RFC 1951, 3.2.5): base value and extra bits of symbol 257 + k / of distance symbol k
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def _len_symbol_table():
    """match length 3..258 -> (symbol - 257, extra value)"""
    sym = np.zeros(MAX_MATCH + 1, np.int64)
    for k, base in enumerate(LEN_BASE):
        sym[base:] = k
    return sym, np.arange(MAX_MATCH + 1) - np.asarray(LEN_BASE)[sym]


def _dist_symbol(d):
    """distances (array, >= 1) -> (symbol, extra value)"""
    sym = np.searchsorted(np.asarray(DIST_BASE), d, side="right") - 1
    return sym, d - np.asarray(DIST_BASE)[sym]


def tokens(block):
    """The tokens of one block: (pos, length, dist) arrays over the token starts in order; length 1 and dist 0 mark a literal."""
    a = np.frombuffer(bytes(block), np.uint8)
    n = len(a)
    if n == 0:
        z = np.zeros(0, np.int64)
        return z, z.copy(), z.copy()
    idx = np.arange(n)
    nl = np.flatnonzero(a == 10)
    starts = np.concatenate([[0], nl + 1])  # first byte of segment i
    seg = np.zeros(n, np.int64)
    seg[nl[nl + 1 < n] + 1] = 1
    seg = np.cumsum(seg)
    has = seg >= 1
    d = np.where(has, starts[seg] - starts[np.maximum(seg - 1, 0)], 0)
    eq = has & (a == a[idx - d])
    link = np.zeros(n, bool)  # p and p + 1 are of one run
    link[:-1] = eq[:-1] & eq[1:] & (d[:-1] == d[1:])
    cut = np.where(~link, idx + 1, 0)
    s = np.concatenate([[0], np.maximum.accumulate(cut)[:-1]])            # the run's first position
    e = np.minimum.accumulate(np.where(~link, idx + 1, n)[::-1])[::-1]    # one behind its last
    o = idx - s
    piece = np.minimum(MAX_MATCH, (e - s) - (o // MAX_MATCH) * MAX_MATCH)
    in_match = eq & (piece >= MIN_MATCH)
    start = ~in_match | (o % MAX_MATCH == 0)
    pos = idx[start]
    return pos, np.where(in_match[start], piece[start], 1), np.where(in_match[start], d[start], 0)


def histogram(data):
    """(litlen[286], dist[30]) symbol counts of the tokens of every block of `data`, end-of-block symbols included"""
    ll, dd = np.zeros(N_LITLEN, np.int64), np.zeros(N_DIST, np.int64)
    lsym, _ = _len_symbol_table()
    data = bytes(data)
    for at in range(0, len(data), PAYLOAD):
        blk = data[at:at + PAYLOAD]
        pos, length, dist = tokens(blk)
        a = np.frombuffer(blk, np.uint8)
        lit = dist == 0
        ll += np.bincount(a[pos[lit]], minlength=N_LITLEN)
        ll += np.bincount(257 + lsym[length[~lit]], minlength=N_LITLEN)
        ll[256] += 1
        dd += np.bincount(_dist_symbol(dist[~lit])[0], minlength=N_DIST)
    return ll, dd


def canonical_codes(lengths):
    """the canonical Huffman codes of the lengths (RFC 1951, 3.2.2), each with its bits reversed: the order deflate packs them in"""
    lengths = [int(x) for x in lengths]
    count = [0] * 17
    for x in lengths:
        count[x] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for bits in range(1, 17):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = []
    for x in lengths:
        c, r = nxt[x], 0
        nxt[x] += 1
        for _ in range(x):
            r, c = (r << 1) | (c & 1), c >> 1
        out.append(r)
    return out


_tables = None


def preset():
    """the frozen preset: dict(litlen, dist: code lengths; header, header_bits: the block header and table as bits, LSB first)"""
    from . import bgzf_preset as p
    return dict(litlen=list(p.LITLEN_LENGTHS), dist=list(p.DIST_LENGTHS), header=bytes.fromhex(p.HEADER_HEX), header_bits=p.HEADER_BITS)


def _get_tables():
    global _tables
    if _tables is None:
        p = preset()
        lsym, lextra = _len_symbol_table()
        lcode, dcode = np.asarray(canonical_codes(p["litlen"]), np.uint64), np.asarray(canonical_codes(p["dist"]), np.uint64)
        _tables = dict(ll_len=np.asarray(p["litlen"], np.uint64), d_len=np.asarray(p["dist"], np.uint64), ll_code=lcode, d_code=dcode,
                       lsym=lsym, lextra=lextra.astype(np.uint64), len_extra_bits=np.asarray(LEN_EXTRA, np.uint64),
                       dist_extra_bits=np.asarray(DIST_EXTRA, np.uint64), header=np.frombuffer(p["header"], np.uint8),
                       header_bits=p["header_bits"])
    return _tables


def deflate_preset(block):
    """the block as one deflate block (BFINAL = 1, BTYPE = 10) under the preset table"""
    t = _get_tables()
    a = np.frombuffer(bytes(block), np.uint8)
    pos, length, dist = tokens(block)
    lit = dist == 0
    val, nb = np.zeros(len(pos) + 1, np.uint64), np.zeros(len(pos) + 1, np.uint64)
    b = a[pos[lit]]
    val[:-1][lit], nb[:-1][lit] = t["ll_code"][b], t["ll_len"][b]
    m = ~lit
    ls = 257 + t["lsym"][length[m]]
    ds, dx = _dist_symbol(dist[m])
    v, k = t["ll_code"][ls].copy(), t["ll_len"][ls].copy()
    for part, bits in ((t["lextra"][length[m]], t["len_extra_bits"][ls - 257]), (t["d_code"][ds], t["d_len"][ds]),
                       (dx.astype(np.uint64), t["dist_extra_bits"][ds])):
        v |= part << k
        k = k + bits
    val[:-1][m], nb[:-1][m] = v, k
    val[-1], nb[-1] = t["ll_code"][256], t["ll_len"][256]  # end of block
    nbi = nb.astype(np.int64)
    off = t["header_bits"] + np.cumsum(nbi) - nbi
    total = int(t["header_bits"] + nbi.sum())
    bits = np.zeros((total + 7) // 8 * 8, np.uint8)
    bits[:t["header_bits"]] = np.unpackbits(t["header"], bitorder="little")[:t["header_bits"]]
    which = np.repeat(np.arange(len(val)), nbi)
    j = np.arange(t["header_bits"], total) - np.repeat(off, nbi)
    bits[t["header_bits"]:total] = (val[which] >> j.astype(np.uint64)) & np.uint64(1)
    return np.packbits(bits, bitorder="little").tobytes()


def deflate_stored(block):
    return b"\x01" + struct.pack("<HH", len(block), len(block) ^ 0xFFFF) + bytes(block)


def member(block, stats=None):
    """one BGZF member of a block of 1..PAYLOAD bytes"""
    block = bytes(block)
    if not 0 < len(block) <= PAYLOAD:
        raise ValueError("a block holds 1..PAYLOAD bytes")
    body = deflate_preset(block)
    stored = len(body) >= len(block) + 5
    if stored:
        body = deflate_stored(block)
    if stats is not None:
        stats["blocks"] = stats.get("blocks", 0) + 1
        stats["stored_blocks"] = stats.get("stored_blocks", 0) + int(stored)
    size = 18 + len(body) + 8
    return (b"\x1f\x8b\x08\x04\0\0\0\0\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", size - 1) + body +
            struct.pack("<II", zlib.crc32(block) & 0xFFFFFFFF, len(block)))


def compress(data, stats=None):
    """`data` as a BGZF stream; stats (a dict) receives blocks and stored_blocks"""
    data = bytes(data)
    if stats is not None:
        stats.setdefault("blocks", 0)
        stats.setdefault("stored_blocks", 0)
    return b"".join(member(data[at:at + PAYLOAD], stats) for at in range(0, len(data), PAYLOAD)) + EOF


def members(stream):
    """the members of a BGZF stream as (offset, size) pairs, hopping by BSIZE"""
    out, at = [], 0
    while at < len(stream):
        if stream[at:at + 4] != b"\x1f\x8b\x08\x04" or stream[at + 12:at + 16] != b"BC\x02\x00":
            raise ValueError("no BGZF member at byte %d" % at)
        size = struct.unpack_from("<H", stream, at + 16)[0] + 1
        out.append((at, size))
        at += size
    if at != len(stream):
        raise ValueError("the last member reaches beyond the stream")
    return out
