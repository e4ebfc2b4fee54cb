// The BGZF reader's format (cellector_bgzf_decompress, option gz_device): a raw DEFLATE stream (RFC 1951) of one BGZF member decoded
// into at most 65536 bytes.  Written like bgzf_format.h: no allocation, no libc, the same code on the device (kernels_inflate.hip)
// and on the host (tests/inflate_host_main.cpp, FileBytes::read).  The device kernel is not inflate_member_host: its table build and
// its copies are spread over a wave.  What both use is here: the bit reader with its bound, the rule a set of code lengths is
// accepted by, the symbol decode step, the length and distance bases, the reading of a dynamic block's code lengths.
//
// Validity is zlib's (inflate with Z_FINISH on the exact body): see inf_code_rule and the INF_E_ kinds.
// Bounds: a byte of input is fetched only below the body's length (zeros behind it, and a decode that used such a bit is refused);
// a byte of output is written only below isize; a distance is checked against the bytes produced; every table index is clamped to
// its table; every trip of a decode loop consumes at least one bit or ends the loop.
#pragma once
#include <stdint.h>

#include "bgzf_format.h"

#define INF_MAX_OUT 65536u   // ISIZE of a BGZF member is at most this (bgzf_index)
#define INF_LFAST_BITS 10u   // primary table of the literal/length code
#define INF_DFAST_BITS 8u    // ... of the distance code
#define INF_NLEN 288u        // symbols of a fixed block's codes (286, 287 and 30, 31 decode and are then refused)
#define INF_NDIST 32u

// why a member is refused (0: it is not)
enum {
    INF_OK = 0,
    INF_E_BTYPE = 1,     // block type 3
    INF_E_STORED = 2,    // LEN != ~NLEN
    INF_E_COUNTS = 3,    // HLIT above 286 or HDIST above 30
    INF_E_CODE = 4,      // an over-subscribed or incomplete set of code lengths, or no end-of-block code
    INF_E_REPEAT = 5,    // a repeat with no previous length, or beyond HLIT + HDIST
    INF_E_SYMBOL = 6,    // bits that are no code; literal/length 286, 287; distance 30, 31
    INF_E_DISTANCE = 7,  // a distance reaching before the member's first byte
    INF_E_OUTPUT = 8,    // output beyond ISIZE
    INF_E_INPUT = 9,     // the body ends inside a symbol or a header
    INF_E_UNUSED = 10,   // whole bytes of the body left behind the final block
    INF_E_LENGTH = 11,   // fewer bytes than ISIZE
    INF_E_CRC = 12,      // CRC-32 differs from the trailer
};

// ---- the bit reader ------------------------------------------------------------------------------------------------------------
// buf holds cnt bits, LSB first; pos is the next byte to fetch.  Bytes at n and behind read as zero: the bits used so far are
// 8 pos - cnt, and inf_overrun says when they went beyond the body.
struct InfBits {
    uint64_t buf;
    uint32_t cnt, pos, n;
};
BGZF_HD void inf_bits_init(InfBits *b, uint32_t n) { b->buf = 0; b->cnt = 0; b->pos = 0; b->n = n; }
// at least 57 bits afterwards; byte_at(p) is asked only for p < n
template <class Fetch>
BGZF_HD void inf_fill(InfBits *b, Fetch byte_at)
{
    while (b->cnt <= 56u) {
        const uint64_t v = b->pos < b->n ? (uint64_t)(uint8_t)byte_at(b->pos) : 0ull;
        b->buf |= v << b->cnt;
        b->pos++;
        b->cnt += 8u;
    }
}
// the same in one step: bytes_at(p) is the 8 bytes from p on, little-endian, p < n, those at n and behind as zero
template <class Fetch8>
BGZF_HD void inf_fill8(InfBits *b, Fetch8 bytes_at)
{
    const uint32_t k = (64u - b->cnt) >> 3;  // whole bytes of room: 0..8
    if (k == 0u) return;
    uint64_t v = b->pos < b->n ? (uint64_t)bytes_at(b->pos) : 0ull;
    if (k < 8u) v &= (1ull << (8u * k)) - 1ull;
    b->buf |= b->cnt < 64u ? v << b->cnt : 0ull;
    b->pos += k;
    b->cnt += 8u * k;
}
BGZF_HD uint32_t inf_peek(const InfBits *b, uint32_t k) { return (uint32_t)b->buf & ((1u << k) - 1u); }  // k <= 16
BGZF_HD void inf_drop(InfBits *b, uint32_t k) { b->buf >>= k; b->cnt -= k; }                          // k <= cnt
BGZF_HD uint32_t inf_take(InfBits *b, uint32_t k) { const uint32_t v = inf_peek(b, k); inf_drop(b, k); return v; }
BGZF_HD uint64_t inf_used_bits(const InfBits *b) { return 8ull * b->pos - b->cnt; }
BGZF_HD bool inf_overrun(const InfBits *b) { return inf_used_bits(b) > 8ull * b->n; }

// ---- a code: count[l] codes of length l (l = 1..15), sym[] the symbols ordered by (length, symbol) -------------------------------
// The rule zlib accepts a set of lengths by (inftrees.c): never over-subscribed; incomplete only for a literal/length or distance
// set whose longest code has one bit (a single code), or with no code at all.  kind: 0 code lengths, 1 literal/length, 2 distance.
BGZF_HD int inf_code_rule(const uint16_t *count, int kind)
{
    int left = 1, max = 0;
    for (int l = 1; l <= 15; l++) {
        left = 2 * left - (int)count[l];
        if (left < 0) return INF_E_CODE;
        if (count[l]) max = l;
    }
    if (max == 0) return kind == 0 ? INF_E_CODE : INF_OK;  // (zlib reads on with a table of invalid codes: a code-length code of
                                                           // none leaves no end-of-block code and is refused a step later)
    if (left > 0 && (kind == 0 || max != 1)) return INF_E_CODE;
    return INF_OK;
}
// The symbol whose code the low bits of v (first bit lowest) spell, among the codes of at most max_len bits; -1: none.
BGZF_HD int inf_decode_walk(const uint16_t *count, const uint16_t *sym, uint32_t cap, uint32_t v, uint32_t max_len, uint32_t *len)
{
    int code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l <= max_len; l++) {
        code |= (int)((v >> (l - 1u)) & 1u);
        const int c = (int)count[l];
        if (code - c < first) {
            const uint32_t at = (uint32_t)(index + (code - first));
            *len = l;
            return (int)sym[at < cap ? at : cap - 1u];
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return -1;
}
// entry i of a primary table of `bits` bits: symbol | length << 9, 0 when i starts no code that short
BGZF_HD uint16_t inf_fast_entry(const uint16_t *count, const uint16_t *sym, uint32_t cap, uint32_t i, uint32_t bits)
{
    uint32_t len = 0;
    const int s = inf_decode_walk(count, sym, cap, i, bits, &len);
    return s < 0 ? (uint16_t)0 : (uint16_t)((uint32_t)s | (len << 9));
}
// one symbol off the reader (at least 15 bits in it); -1: the bits are no code
BGZF_HD int inf_symbol(InfBits *b, const uint16_t *fast, uint32_t fast_bits, const uint16_t *count, const uint16_t *sym, uint32_t cap)
{
    const uint32_t v = inf_peek(b, 15u);
    const uint32_t e = fast[v & ((1u << fast_bits) - 1u)];
    if (e) {
        inf_drop(b, e >> 9);
        return (int)(e & 511u);
    }
    uint32_t len = 0;
    const int s = inf_decode_walk(count, sym, cap, v, 15u, &len);
    if (s >= 0) inf_drop(b, len);
    return s;
}

// ---- lengths and distances (RFC 1951, 3.2.5) -----------------------------------------------------------------------------------
BGZF_HD uint32_t inf_len_base(uint32_t s /*257..285*/, uint32_t *extra_bits)
{
    const uint32_t k = s - 257u;
    if (k < 8u) { *extra_bits = 0; return 3u + k; }
    if (k == 28u) { *extra_bits = 0; return 258u; }
    const uint32_t x = (k - 4u) >> 2;
    *extra_bits = x;
    return 3u + ((4u + (k & 3u)) << x);
}
BGZF_HD uint32_t inf_dist_base(uint32_t s /*0..29*/, uint32_t *extra_bits)
{
    if (s < 4u) { *extra_bits = 0; return 1u + s; }
    const uint32_t x = (s - 2u) >> 1;
    *extra_bits = x;
    return 1u + ((2u + (s & 1u)) << x);
}
// the order the code-length code's lengths come in: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, five bits each
BGZF_HD uint32_t inf_cl_order(uint32_t k /*0..18*/)
{
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 |
                        11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (uint32_t)((k < 12u ? lo >> (5u * k) : hi >> (5u * (k - 12u))) & 31u);
}
// a fixed block's lengths: lens[0..288) literal/length, lens[288..320) distance
BGZF_HD uint8_t inf_fixed_length(uint32_t s) { return s < 144u ? 8 : s < 256u ? 9 : s < 280u ? 7 : s < 288u ? 8 : 5; }

// ---- the tables of one block ----------------------------------------------------------------------------------------------------
// (one per decoder: on the device one per wave in LDS, 4.3 KB)
struct InfTables {
    uint16_t lfast[1u << INF_LFAST_BITS];
    uint16_t dfast[1u << INF_DFAST_BITS];
    uint16_t lsym[INF_NLEN], dsym[INF_NDIST];
    uint16_t lcount[16], dcount[16];
    uint16_t ccount[16], csym[20];  // the code-length code
    uint8_t lens[INF_NLEN + INF_NDIST];
};

// count[] and sym[] of lens[0..n): serial (the device ranks the symbols with ballots instead).  offs: 16 words of scratch (the
// device has them in LDS: an array of its own, indexed by a length, would live in scratch memory).
BGZF_HD void inf_sort_symbols(const uint8_t *lens, uint32_t n, uint16_t *count, uint16_t *sym, uint32_t cap, uint16_t *offs)
{
    for (int l = 0; l < 16; l++) count[l] = 0;
    for (uint32_t s = 0; s < n; s++) count[lens[s] & 15u]++;
    count[0] = 0;
    offs[0] = offs[1] = 0;
    for (int l = 1; l < 15; l++) offs[l + 1] = (uint16_t)(offs[l] + count[l]);
    for (uint32_t s = 0; s < n; s++) {
        const uint32_t l = lens[s] & 15u;
        if (l) {
            const uint32_t at = offs[l]++;
            sym[at < cap ? at : cap - 1u] = (uint16_t)s;
        }
    }
}

// A dynamic block's header behind its three type bits: HLIT, HDIST, HCLEN, the code-length code, the HLIT + HDIST lengths into
// t->lens[0..*nlen + *ndist).  Serial on host and device (at most 316 short symbols).
// (fill(b): inf_fill or inf_fill8 with the caller's way to the input)
template <class Fill>
BGZF_HD int inf_read_lengths(InfBits *b, Fill fill, InfTables *t, uint32_t *nlen, uint32_t *ndist)
{
    fill(b);
    const uint32_t nl = inf_take(b, 5u) + 257u, nd = inf_take(b, 5u) + 1u, nc = inf_take(b, 4u) + 4u;
    if (nl > 286u || nd > 30u) return INF_E_COUNTS;
    uint8_t *cl = t->lens + INF_NLEN;  // (19 bytes of the distance part serve as the code-length code's lengths meanwhile)
    for (uint32_t k = 0; k < 19u; k++) cl[k] = 0;
    for (uint32_t k = 0; k < nc; k++) {
        if ((k & 15u) == 0u) fill(b);
        cl[inf_cl_order(k)] = (uint8_t)inf_take(b, 3u);
    }
    inf_sort_symbols(cl, 19u, t->ccount, t->csym, 20u, t->lcount);  // (lcount: free until the block's tables are built)
    const int e = inf_code_rule(t->ccount, 0);
    if (e) return e;
    uint32_t have = 0, prev = 0;
    while (have < nl + nd) {
        fill(b);
        if (inf_overrun(b)) return INF_E_INPUT;  // (every trip below takes at least one bit)
        uint32_t len = 0;
        const int s = inf_decode_walk(t->ccount, t->csym, 20u, inf_peek(b, 7u), 7u, &len);
        if (s < 0) return INF_E_SYMBOL;
        inf_drop(b, len);
        if (s < 16) {
            t->lens[have++] = (uint8_t)s;
            prev = (uint32_t)s;
            continue;
        }
        uint32_t rep, val = 0;
        if (s == 16) {
            if (have == 0u) return INF_E_REPEAT;
            val = prev;
            rep = 3u + inf_take(b, 2u);
        } else if (s == 17) {
            rep = 3u + inf_take(b, 3u);
        } else {
            rep = 11u + inf_take(b, 7u);
        }
        if (have + rep > nl + nd) return INF_E_REPEAT;
        for (uint32_t k = 0; k < rep; k++) t->lens[have++] = (uint8_t)val;
        prev = val;
    }
    if (inf_overrun(b)) return INF_E_INPUT;
    if (t->lens[256] == 0) return INF_E_CODE;
    *nlen = nl;
    *ndist = nd;
    return INF_OK;
}

// One token off the reader (at least 48 bits in it).  Returns 0: a literal in *a; 1: a match of length *a at distance *d;
// 2: end of block; below 0: minus the INF_E_ kind.
BGZF_HD int inf_token(InfBits *b, const InfTables *t, uint32_t *a, uint32_t *d)
{
    const int s = inf_symbol(b, t->lfast, INF_LFAST_BITS, t->lcount, t->lsym, INF_NLEN);
    if (s < 0) return -INF_E_SYMBOL;
    if (s < 256) { *a = (uint32_t)s; return 0; }
    if (s == 256) return 2;
    if (s > 285) return -INF_E_SYMBOL;
    uint32_t xb;
    const uint32_t base = inf_len_base((uint32_t)s, &xb);
    *a = base + inf_take(b, xb);
    const int ds = inf_symbol(b, t->dfast, INF_DFAST_BITS, t->dcount, t->dsym, INF_NDIST);
    if (ds < 0 || ds > 29) return -INF_E_SYMBOL;
    const uint32_t dbase = inf_dist_base((uint32_t)ds, &xb);
    *d = dbase + inf_take(b, xb);
    return 1;
}

// ---- CRC-32 of up to INF_MAX_OUT bytes -------------------------------------------------------------------------------------------
// BgzfTables' xp32 reaches 32 * 1023 + 31 bytes; a member's text is up to twice that.  The reader's operators stand beside it.
#define INF_CRC_CHUNKS 2049u  // xp32[k] = x^(8 * 32 k), k <= INF_MAX_OUT / 32
struct InfCrcTables {
    uint32_t crc[256];
    uint32_t xp32[INF_CRC_CHUNKS];
    uint32_t xp1[BGZF_CRC_CHUNK];
};
// the bytewise CRC-32 without a table (host fallback paths and the test program; short inputs)
BGZF_HD uint32_t inf_crc32_plain(const uint8_t *p, uint32_t n)
{
    uint32_t c = 0xFFFFFFFFu;
    for (uint32_t k = 0; k < n; k++) {
        c ^= p[k];
        for (int i = 0; i < 8; i++) c = (c >> 1) ^ ((c & 1u) ? BGZF_CRC_POLY : 0u);
    }
    return ~c;
}

// ---- host only ----------------------------------------------------------------------------------------------------------------
static inline void inf_crc_tables_build(InfCrcTables *t)
{
    for (uint32_t b = 0; b < 256; b++) {
        uint32_t c = b;
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1u) ? BGZF_CRC_POLY : 0u);
        t->crc[b] = c;
    }
    const uint32_t x8 = 0x80000000u >> 8;
    t->xp1[0] = 0x80000000u;
    for (uint32_t r = 1; r < BGZF_CRC_CHUNK; r++) t->xp1[r] = bgzf_crc_mul(t->xp1[r - 1], x8);
    const uint32_t x256 = bgzf_crc_mul(t->xp1[BGZF_CRC_CHUNK - 1], x8);
    t->xp32[0] = 0x80000000u;
    for (uint32_t k = 1; k < INF_CRC_CHUNKS; k++) t->xp32[k] = bgzf_crc_mul(t->xp32[k - 1], x256);
}

// the tables of lens[0..nlen) and lens[INF_NLEN..INF_NLEN + ndist), serial
static inline int inf_build_tables_host(InfTables *t, uint32_t nlen, uint32_t ndist)
{
    inf_sort_symbols(t->lens, nlen, t->lcount, t->lsym, INF_NLEN, t->ccount);
    inf_sort_symbols(t->lens + INF_NLEN, ndist, t->dcount, t->dsym, INF_NDIST, t->ccount);
    int e = inf_code_rule(t->lcount, 1);
    if (!e) e = inf_code_rule(t->dcount, 2);
    if (e) return e;
    for (uint32_t i = 0; i < (1u << INF_LFAST_BITS); i++) t->lfast[i] = inf_fast_entry(t->lcount, t->lsym, INF_NLEN, i, INF_LFAST_BITS);
    for (uint32_t i = 0; i < (1u << INF_DFAST_BITS); i++) t->dfast[i] = inf_fast_entry(t->dcount, t->dsym, INF_NDIST, i, INF_DFAST_BITS);
    return INF_OK;
}

// The serial reference: the raw DEFLATE stream in[0..n_in) into out[0..isize).  Returns the bytes produced; *err is INF_OK exactly
// when zlib's inflate(Z_FINISH) of those n_in bytes ends the stream with isize bytes (the CRC is the caller's: inf_crc32_plain).
static inline uint32_t inflate_member_host(const uint8_t *in, uint32_t n_in, uint8_t *out, uint32_t isize, int *err)
{
    InfTables t;
    InfBits b;
    inf_bits_init(&b, n_in);
    auto byte_at = [in](uint32_t p) { return in[p]; };
    uint32_t produced = 0;
    *err = INF_OK;
    for (bool last = false; !last && *err == INF_OK;) {
        inf_fill(&b, byte_at);
        last = inf_take(&b, 1u) != 0u;
        const uint32_t type = inf_take(&b, 2u);
        if (inf_overrun(&b)) { *err = INF_E_INPUT; break; }
        if (type == 3u) { *err = INF_E_BTYPE; break; }
        if (type == 0u) {
            inf_drop(&b, b.cnt & 7u);
            inf_fill(&b, byte_at);
            const uint32_t len = inf_take(&b, 16u), nlen = inf_take(&b, 16u);
            if (inf_overrun(&b)) { *err = INF_E_INPUT; break; }
            if (len != (nlen ^ 0xffffu)) { *err = INF_E_STORED; break; }
            const uint32_t at = (uint32_t)(inf_used_bits(&b) >> 3);  // (a whole byte: the reader was aligned)
            if (len > n_in - at) { *err = INF_E_INPUT; break; }
            if (len > isize - produced) { *err = INF_E_OUTPUT; break; }
            for (uint32_t k = 0; k < len; k++) out[produced + k] = in[at + k];
            produced += len;
            b.buf = 0; b.cnt = 0; b.pos = at + len;
            continue;
        }
        uint32_t nlen = INF_NLEN, ndist = INF_NDIST;
        if (type == 1u)
            for (uint32_t s = 0; s < INF_NLEN + INF_NDIST; s++) t.lens[s] = inf_fixed_length(s);
        else if ((*err = inf_read_lengths(&b, [byte_at](InfBits *r) { inf_fill(r, byte_at); }, &t, &nlen, &ndist)) != INF_OK)
            break;
        if (type == 2u)  // (the distance lengths follow the literal/length ones at once: to their own place, from the back)
            for (uint32_t k = ndist; k-- > 0u;) t.lens[INF_NLEN + k] = t.lens[nlen + k];
        if ((*err = inf_build_tables_host(&t, nlen, ndist)) != INF_OK) break;
        for (;;) {
            inf_fill(&b, byte_at);
            if (inf_overrun(&b)) { *err = INF_E_INPUT; break; }  // (a token takes at least one bit: the loop ends)
            uint32_t a = 0, d = 0;
            const int k = inf_token(&b, &t, &a, &d);
            if (k < 0) { *err = -k; break; }
            if (k == 2) break;
            if (k == 0) {
                if (produced >= isize) { *err = INF_E_OUTPUT; break; }
                out[produced++] = (uint8_t)a;
                continue;
            }
            if (d > produced) { *err = INF_E_DISTANCE; break; }
            if (a > isize - produced) { *err = INF_E_OUTPUT; break; }
            for (uint32_t j = 0; j < a; j++, produced++) out[produced] = out[produced - d];
        }
        if (*err == INF_OK && inf_overrun(&b)) *err = INF_E_INPUT;
    }
    if (*err == INF_OK && (inf_used_bits(&b) + 7u) / 8u != n_in) *err = INF_E_UNUSED;
    if (*err == INF_OK && produced != isize) *err = INF_E_LENGTH;
    return produced;
}
