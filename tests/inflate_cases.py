"""The inputs of the BGZF reader's tests (tests/test_inflate_reference.py, test_gpu_inflate.py): name -> (raw deflate body, the ISIZE
and the CRC-32 its trailer claims).  Everything is made from seeds, by zlib or by the small bit writer below; nothing is read from a
file.  `reference` is the rule every decoder of the project is held to: zlib's inflate of exactly the body, then length and CRC."""
import functools
import struct
import zlib

import numpy as np

import bgzf_cases

TEXT = 65280   # the most text bgzip puts into a block


def reference(body, isize, crc):
    """the member's text, or None where it is refused: zlib raises, leaves input unused (what Z_FINISH on the exact body reports),
    or the length or the CRC-32 is not the trailer's"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(bytes(body)) + d.flush()
        zlib.decompress(bytes(body), -15)
    except zlib.error:
        return None
    if not d.eof or d.unused_data or len(out) != isize or zlib.crc32(out) != crc:
        return None
    return out


def claim(body, text):
    return bytes(body), len(text), zlib.crc32(text)


def _deflate(data, level=-1, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=()):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out, at = b"", 0
    for f in flush_at:
        out += c.compress(data[at:f]) + c.flush(zlib.Z_FULL_FLUSH)
        at = f
    return out + c.compress(data[at:]) + c.flush()


@functools.lru_cache(maxsize=None)
def zlib_cases():
    text = bgzf_cases._text(TEXT)
    rng = np.random.default_rng(17)
    c = {}
    for level in (1, 6, 9):
        c["text_level%d" % level] = claim(_deflate(text, level), text)
    c["fixed"] = claim(_deflate(text[:3000], 6, zlib.Z_FIXED), text[:3000])
    c["stored"] = claim(_deflate(text[:3000], 0), text[:3000])
    rnd = rng.integers(0, 256, TEXT).astype(np.uint8).tobytes()
    c["random_two_stored"] = claim(_deflate(rnd), rnd)
    rle = b"a" * 700 + b"bc" * 400 + text[:20000]
    c["rle"] = claim(_deflate(rle, 6, zlib.Z_RLE), rle)
    nine = text[:9000]
    c["full_flush"] = claim(_deflate(nine, 6, flush_at=(1000, 1000, 4000)), nine)
    fib = [1, 2]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    sym = np.repeat(np.arange(24, dtype=np.uint8) + 65, fib)
    rng.shuffle(sym)
    huff = sym.tobytes()[:TEXT]
    c["huffman_only"] = claim(_deflate(huff, 6, zlib.Z_HUFFMAN_ONLY), huff)
    c["empty"] = claim(_deflate(b""), b"")
    c["one_byte"] = claim(_deflate(b"x"), b"x")
    return c


def members_of(stream):
    """[(body, isize, crc)] of a BGZF stream"""
    out, pos = [], 0
    while pos < len(stream):
        xlen = struct.unpack_from("<H", stream, pos + 10)[0]
        clen = struct.unpack_from("<H", stream, pos + 16)[0] + 1
        crc, isize = struct.unpack_from("<II", stream, pos + clen - 8)
        out.append((stream[pos + 12 + xlen:pos + clen - 8], isize, crc))
        pos += clen
    return out


@functools.lru_cache(maxsize=None)
def library_cases():
    """every member of the writer's twin over tests/bgzf_cases.py"""
    c = {}
    for name in sorted(bgzf_cases.cases()):
        for k, m in enumerate(members_of(bgzf_cases.expected(name)[0])):
            c["lib_%s_%d" % (name, k)] = m
    return c


# ---- a bit writer for what zlib never emits ------------------------------------------------------------------------------------
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DL = [5] * 32
FLAT_LL = [8] * 226 + [9] * 60     # a complete code over all 286 symbols
FLAT_DL = [4] * 2 + [5] * 28       # ... over all 30
FLAT_CL = [4] * 16 + [0, 0, 0]     # ... over the lengths 0..15, no repeat codes


class Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, bits):      # LSB first
        self.acc |= (value & ((1 << bits) - 1)) << self.n
        self.n += bits

    def code(self, code, bits):      # a Huffman code: its first bit first
        for k in range(bits - 1, -1, -1):
            self.put((code >> k) & 1, 1)

    def align(self):
        self.n = (self.n + 7) // 8 * 8

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def canonical(lengths):
    """symbol -> (code, bits) by RFC 1951 3.2.2; an over-subscribed set still gets numbers (the decoder must refuse it first)"""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lengths):
        if l:
            out[s] = (nxt[l] & ((1 << l) - 1), l)
            nxt[l] += 1
    return out


def _tokens(w, ll, dl, tokens):
    lc, dc = canonical(ll), canonical(dl)
    for t in tokens:
        if t[0] == "lit":
            w.code(*lc[t[1]])
        elif t[0] == "eob":
            w.code(*lc[256])
        elif t[0] == "sym":          # a raw literal/length symbol
            w.code(*lc[t[1]])
        elif t[0] == "bits":         # raw bits
            w.put(t[1], t[2])
        elif t[0] == "match":
            _, length, dist = t[:3]
            s = max(k for k in range(29) if LEN_BASE[k] <= length) if length < 258 else 28
            w.code(*lc[257 + s])
            w.put(length - LEN_BASE[s], LEN_EXTRA[s])
            if len(t) > 3:           # ("match", length, None, distance symbol, extra value, extra bits)
                w.code(*dc[t[3]])
                w.put(t[4], t[5])
            else:
                d = max(k for k in range(30) if DIST_BASE[k] <= dist)
                w.code(*dc[d])
                w.put(dist - DIST_BASE[d], DIST_EXTRA[d])


def fixed_block(w, final, tokens):
    w.put(final, 1)
    w.put(1, 2)
    _tokens(w, FIXED_LL, FIXED_DL, tokens)


def dynamic_block(w, final, tokens, ll=FLAT_LL, dl=FLAT_DL, cl=FLAT_CL, cl_seq=None):
    """ll / dl: the HLIT / HDIST code lengths as sent (their count is what the header says); cl: the 19 lengths of the code-length
    code; cl_seq: [(code-length symbol, extra value)] instead of one symbol per length"""
    w.put(final, 1)
    w.put(2, 2)
    w.put(len(ll) - 257, 5)
    w.put(len(dl) - 1, 5)
    w.put(19 - 4, 4)
    for s in CL_ORDER:
        w.put(cl[s], 3)
    cc = canonical(cl)
    for s, extra in (cl_seq if cl_seq is not None else [(l, 0) for l in list(ll) + list(dl)]):
        w.code(*cc[s])
        w.put(extra, {16: 2, 17: 3, 18: 7}.get(s, 0))
    _tokens(w, ll, dl, tokens)


def stored_block(w, final, data, nlen=None):
    w.put(final, 1)
    w.put(0, 2)
    w.align()
    w.put(len(data), 16)
    w.put((~len(data) & 0xffff) if nlen is None else nlen, 16)
    for b in data:
        w.put(b, 8)


def _lits(data):
    return [("lit", b) for b in data]


def _grow(n):
    """tokens for n >= 1 bytes of 'q': one literal, matches at distance 1, literals for a rest below 3"""
    t, left = [("lit", 113)], n - 1
    while left >= 3:
        m = min(left, 258)
        t.append(("match", m, 1))
        left -= m
    return t + [("lit", 113)] * left


def _dyn(tokens, **kw):
    w = Bits()
    dynamic_block(w, 1, tokens, **kw)
    return w.bytes()


def _fix(tokens):
    w = Bits()
    fixed_block(w, 1, tokens)
    return w.bytes()


@functools.lru_cache(maxsize=None)
def hand_cases():
    """name -> (body, isize, crc, accepted); `accepted` is what the case is meant to be and tests check it against `reference`"""
    c = {}

    def ok(name, body, text=None):   # (text None: whatever zlib makes of it)
        made = zlib.decompress(body, -15)
        assert text is None or made == text, name
        c[name] = claim(body, made) + (True,)

    def bad(name, body, text=b""):
        c[name] = claim(body, text) + (False,)

    # a code-length code of 7 bits: the lengths used are 0, 1, 2 (codes of 1, 2, 3 bits), the 7-bit codes stay unused
    ll3 = [0] * 257
    ll3[97], ll3[98], ll3[256] = 1, 2, 2
    cl7 = [1, 2, 3, 4, 5, 6, 7, 7] + [0] * 11
    ok("cl_code_7_bits", _dyn(_lits(b"abba") + [("eob",)], ll=ll3, dl=[0], cl=cl7), b"abba")
    # ... and a length sent with a 7-bit code: 'a' 1 bit, 'b' .. : lengths 1, 2, 3, 7 x 32 complete: 1/2 + 1/4 + 1/8 + 16/128
    ll7 = [0] * 257
    ll7[97], ll7[98], ll7[256] = 1, 2, 3
    for s in range(16):
        ll7[s] = 7
    cl7b = [1, 2, 3, 4, 0, 0, 0, 5, 6, 7, 7] + [0] * 8   # lengths 0, 1, 2, 3, 7 (5 bits), 8, 9, 10 unused
    ok("cl_code_7_bits_length_7", _dyn(_lits(b"ab\x03a") + [("eob",)], ll=ll7, dl=[0], cl=cl7b), b"ab\x03a")
    # a distance code of 15 bits: symbols 0..14 of 1..15 bits, symbol 15 of 15 bits
    dl15 = list(range(1, 16)) + [15]
    base = bytes(range(32, 127)) * 3
    ok("dist_code_15_bits", _dyn(_lits(base) + [("match", 40, 200), ("match", 7, 130), ("eob",)], dl=dl15))
    # distance 32768 = produced; distance = produced when small
    big = b"q" * 32768
    ok("distance_32768", _dyn(_grow(32768) + [("match", 10, 32768), ("lit", 65), ("match", 258, 32768), ("eob",)]),
       big + b"q" * 10 + b"A" + b"q" * 258)
    ok("distance_is_produced", _dyn(_lits(b"hello") + [("match", 12, 5), ("eob",)]), b"hello" + b"hellohellohe")
    bad("distance_before_first_byte", _dyn(_lits(b"hello") + [("match", 12, 6), ("eob",)]))
    bad("distance_32768_of_32767", _dyn(_grow(32767) + [("match", 10, 32768), ("eob",)]))
    # a member of exactly 65536 bytes; one more is beyond ISIZE
    ok("isize_65536", _dyn(_grow(65536) + [("eob",)]), b"q" * 65536)
    c["output_beyond_isize_literal"] = (_dyn(_grow(65536) + [("lit", 113), ("eob",)]), 65536, zlib.crc32(b"q" * 65536), False)
    c["output_beyond_isize_match"] = (_dyn(_grow(65530) + [("match", 7, 1), ("eob",)]), 65536, zlib.crc32(b"q" * 65536), False)
    c["output_short_of_isize"] = (_dyn(_grow(65535) + [("eob",)]), 65536, zlib.crc32(b"q" * 65536), False)
    # a single-code distance set (zlib accepts it), used; its other bit is no code; no distance code at all
    ok("single_distance_code", _dyn(_lits(b"x") + [("match", 30, 1), ("eob",)], dl=[1]), b"x" * 31)
    bad("single_distance_code_other_bit", _dyn(_lits(b"x") + [("sym", 257 + 20), ("bits", 0, 4), ("bits", 1, 1), ("eob",)], dl=[1]))
    ok("no_distance_code", _dyn(_lits(b"xyz") + [("eob",)], dl=[0]), b"xyz")
    bad("no_distance_code_used", _dyn(_lits(b"xyz") + [("sym", 257), ("bits", 0, 1), ("eob",)], dl=[0]))
    ll1 = [0] * 257
    ll1[256] = 1
    ok("single_litlen_code", _dyn([("eob",)], ll=ll1, dl=[0]), b"")
    bad("single_litlen_code_other_bit", _dyn([("bits", 1, 1)], ll=ll1, dl=[0]))
    # ---- refusals ----
    over, short = list(FLAT_LL), list(FLAT_LL)
    over[285], short[0] = 8, 9
    bad("litlen_over_subscribed", _dyn(_lits(b"ab") + [("eob",)], ll=over))
    bad("litlen_incomplete", _dyn(_lits(b"ab") + [("eob",)], ll=short))
    bad("dist_over_subscribed", _dyn(_lits(b"ab") + [("eob",)], dl=[1, 1, 1]))
    bad("dist_incomplete", _dyn(_lits(b"ab") + [("eob",)], dl=[2, 2, 2]))
    bad("cl_over_subscribed", _dyn(_lits(b"ab") + [("eob",)], cl=[4] * 16 + [4, 0, 0]))
    bad("cl_incomplete", _dyn(_lits(b"ab") + [("eob",)], cl=[4] * 15 + [5, 0, 0, 0]))
    no_eob = list(FLAT_LL)
    no_eob[256], no_eob[257] = 0, 8   # (still complete: 9 -> 8 takes the room of the code that left)
    bad("no_end_of_block_code", _dyn(_lits(b"ab"), ll=no_eob))
    bad("litlen_286", _fix(_lits(b"ab") + [("sym", 286), ("eob",)]))
    bad("litlen_287", _fix(_lits(b"ab") + [("sym", 287), ("eob",)]))
    bad("dist_30", _fix(_lits(b"abcd") + [("match", 3, None, 30, 0, 0), ("eob",)]))
    bad("dist_31", _fix(_lits(b"abcd") + [("match", 3, None, 31, 0, 0), ("eob",)]))
    bad("hlit_287", _dyn([("eob",)], ll=[8] * 224 + [9] * 63))
    bad("hlit_288", _dyn([("eob",)], ll=[8] * 224 + [9] * 64))
    bad("hdist_31", _dyn([("eob",)], dl=[4] + [5] * 30))
    bad("hdist_32", _dyn([("eob",)], dl=[5] * 32))
    rep = list(FLAT_CL)
    rep[15], rep[16] = 5, 5      # (the length 15 shares its room with the repeat code 16)
    bad("repeat_without_previous", _dyn([("eob",)], cl=rep, cl_seq=[(16, 0)] + [(l, 0) for l in (FLAT_LL + FLAT_DL)[3:]]))
    bad("repeat_beyond_the_lengths", _dyn([("eob",)], cl=rep, cl_seq=[(l, 0) for l in (FLAT_LL + FLAT_DL)[:-2]] + [(16, 3)]))
    w = Bits()
    stored_block(w, 1, b"stored", nlen=0x1234)
    bad("stored_len_nlen", w.bytes())
    w = Bits()
    stored_block(w, 1, b"stored")
    bad("stored_cut", w.bytes()[:-2])
    ok("stored_hand", w.bytes(), b"stored")
    w = Bits()
    w.put(1, 1)
    w.put(3, 2)
    bad("block_type_3", w.bytes() + b"\0\0\0")
    good = _dyn(_lits(b"some text, some text") + [("match", 9, 11), ("eob",)])
    text = zlib.decompress(good, -15)
    ok("hand_plain", good)
    c["input_ends_in_symbol"] = (good[:-3],) + claim(good, text)[1:] + (False,)
    c["input_ends_in_header"] = (good[:40],) + claim(good, text)[1:] + (False,)
    c["unused_input_byte"] = (good + b"\0",) + claim(good, text)[1:] + (False,)
    c["wrong_crc"] = (good, len(text), zlib.crc32(text) ^ 1, False)
    c["empty_body"] = (b"", 0, 0, False)
    # several blocks by hand: stored, fixed, dynamic, an empty stored one between
    w = Bits()
    stored_block(w, 0, b"one ")
    fixed_block(w, 0, _lits(b"two ") + [("match", 4, 8), ("eob",)])
    stored_block(w, 0, b"")
    dynamic_block(w, 1, _lits(b"three ") + [("match", 20, 3), ("eob",)])
    ok("blocks_of_every_type", w.bytes(), b"one two one three " + b"ee ee ee ee ee ee ee"[:20])
    return c


MUTATED = ("text_level6", "fixed", "stored", "rle", "full_flush")


@functools.lru_cache(maxsize=None)
def mutation_cases():
    """for each member of MUTATED, 200 seeded mutations: one byte of the body flipped, or the body cut at a random byte"""
    c = {}
    for i, name in enumerate(MUTATED):
        body, isize, crc = zlib_cases()[name]
        rng = np.random.default_rng(1000 + i)
        for k in range(200):
            at = int(rng.integers(0, len(body)))
            if rng.random() < 0.7:
                m = body[:at] + bytes([body[at] ^ int(rng.integers(1, 256))]) + body[at + 1:]
            else:
                m = body[:at]
            c["mut_%s_%03d" % (name, k)] = (m, isize, crc)
    return c


@functools.lru_cache(maxsize=None)
def all_cases():
    """name -> (body, isize, crc): every stream above"""
    c = dict(zlib_cases())
    c.update(library_cases())
    c.update({k: v[:3] for k, v in hand_cases().items()})
    c.update(mutation_cases())
    return c


def member(body, isize, crc):
    """the BGZF member around a body (the body of at most 65510 bytes)"""
    size = 18 + len(body) + 8
    assert size <= 65536
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", size - 1) + bytes(body) + struct.pack("<II", crc, isize))


def records(names):
    """the input file of tests/inflate_host_main.cpp for these cases"""
    c = all_cases()
    return b"".join(struct.pack("<III", len(c[n][0]), c[n][1], c[n][2]) + c[n][0] for n in names)
