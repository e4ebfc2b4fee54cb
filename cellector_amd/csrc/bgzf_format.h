// The BGZF writer's format (cellector_bgzf_compress, cellector_write_mtx_bgzf): what a token is, its bits under the preset Huffman
// table, the gzip member around a block, and the CRC-32 pieces.  The same code runs on the device (kernels_bgzf.hip) and on the host
// (tests/bgzf_host_main.cpp drives bgzf_encode_block_host on a CPU); cellector_amd/bgzf.py is the byte-identical numpy twin and
// states the format in words.  bgzf_preset.h holds the preset's code lengths and the table's bit string (tools/bgzf_preset.py).
#pragma once
#include <stdint.h>
#include <string.h>

#include "bgzf_preset.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BGZF_HD __host__ __device__ __forceinline__
#else
#define BGZF_HD inline
#endif

#define BGZF_PAYLOAD 32640u       // input bytes of a block (a multiple of 16)
#define BGZF_MAX_MATCH 258u
#define BGZF_MIN_MATCH 3u
#define BGZF_HEAD 18u             // member header
#define BGZF_TAIL 8u              // CRC-32, ISIZE
#define BGZF_MAX_MEMBER (BGZF_HEAD + 5u + BGZF_PAYLOAD + BGZF_TAIL)  // a stored block; a preset block is smaller
#define BGZF_EOF_BYTES 28u
#define BGZF_CRC_CHUNK 32u        // bytes of one CRC chunk; chunks are aligned to the block's END
#define BGZF_CRC_CHUNKS 1024u     // >= ceil(BGZF_PAYLOAD / BGZF_CRC_CHUNK)
#define BGZF_CRC_POLY 0xEDB88320u

static const uint8_t BGZF_EOF[BGZF_EOF_BYTES] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 'B', 'C', 0x02, 0,
                                                 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// Everything a block's encoder looks up, as words (the device keeps the first four arrays in LDS).
//   lit[b]    literal b:            reversed code | code length << 16
//   len[m]    match length m:       (reversed code | extra value << code length) | bits of both << 24      (m = 3..258)
//   dist[s]   distance symbol s:    reversed code | code length << 16
//   crc[b]    the byte table of the reflected CRC-32
//   xp32[k]   x^(8 * 32 k) mod P: a CRC state moved over k chunks of 32 bytes; xp1[r]: x^(8 r), r < 32
//   eob       the end-of-block symbol, as lit[]
struct BgzfTables {
    uint32_t lit[256];
    uint32_t len[260];
    uint32_t dist[32];
    uint32_t crc[256];
    uint32_t xp32[BGZF_CRC_CHUNKS];
    uint32_t xp1[BGZF_CRC_CHUNK];
    uint32_t header[BGZF_HEADER_WORDS + 1];
    uint32_t eob;
};
#define BGZF_LDS_TABLE_WORDS (256u + 260u + 32u + 256u)  // lit, len, dist, crc

// a * b mod P in the reflected representation (x^0 = 0x80000000)
BGZF_HD uint32_t bgzf_crc_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? BGZF_CRC_POLY : 0u);
    }
    return p;
}
// x^(8 n) mod P, n <= 32 * 1023 + 31: the operator that moves a CRC state over n bytes
BGZF_HD uint32_t bgzf_crc_shift(const uint32_t *xp32, const uint32_t *xp1, uint32_t n) { return bgzf_crc_mul(xp32[n >> 5], xp1[n & 31u]); }
// the raw (no init, no final xor) state after one more byte
BGZF_HD uint32_t bgzf_crc_byte(const uint32_t *crc, uint32_t state, uint8_t b) { return crc[(state ^ b) & 0xffu] ^ (state >> 8); }
// The CRC-32 of n bytes from X = the xor over the chunks k (k = 0: the LAST 32 bytes; the first chunk may be shorter) of
// mul(raw state of the chunk from 0, xp32[k]): the init value moved over all n bytes, the chunks, the final xor.
BGZF_HD uint32_t bgzf_crc_finish(const uint32_t *xp32, const uint32_t *xp1, uint32_t X, uint32_t n)
{
    return 0xFFFFFFFFu ^ bgzf_crc_mul(0xFFFFFFFFu, bgzf_crc_shift(xp32, xp1, n)) ^ X;
}

// distance 1..32768 -> its symbol, extra bits and extra value (RFC 1951, 3.2.5)
BGZF_HD uint32_t bgzf_dist_symbol(uint32_t d, uint32_t *extra_bits, uint32_t *extra)
{
    const uint32_t x = d - 1u;
    if (x < 4u) { *extra_bits = 0; *extra = 0; return x; }
    uint32_t h = 2;  // the highest set bit of x (x >= 4)
    while ((x >> (h + 1u)) != 0u) h++;
    *extra_bits = h - 1u;
    *extra = x & ((1u << (h - 1u)) - 1u);
    return 2u * h + ((x >> (h - 1u)) & 1u);
}

// the bits of a literal / of a match (len, d), LSB first, and how many (at most 15 / 48)
BGZF_HD uint64_t bgzf_literal_bits(const uint32_t *lit, uint8_t b, uint32_t *n_bits)
{
    const uint32_t e = lit[b];
    *n_bits = e >> 16;
    return e & 0xffffu;
}
BGZF_HD uint64_t bgzf_match_bits(const uint32_t *len_tab, const uint32_t *dist_tab, uint32_t len, uint32_t d, uint32_t *n_bits)
{
    const uint32_t l = len_tab[len];
    uint32_t xb, xv;
    const uint32_t ds = dist_tab[bgzf_dist_symbol(d, &xb, &xv)];
    uint32_t n = l >> 24;
    uint64_t v = l & 0xffffffu;
    v |= (uint64_t)(ds & 0xffffu) << n;
    n += ds >> 16;
    v |= (uint64_t)xv << n;
    *n_bits = n + xb;
    return v;
}

// the length of the match piece position p is in, for a run [s, e): pieces of 258 from s
BGZF_HD uint32_t bgzf_piece(uint32_t p, uint32_t s, uint32_t e, uint32_t *offset_in_piece)
{
    const uint32_t o = p - s, k = o / BGZF_MAX_MATCH, left = (e - s) - k * BGZF_MAX_MATCH;
    *offset_in_piece = o - k * BGZF_MAX_MATCH;
    return left < BGZF_MAX_MATCH ? left : BGZF_MAX_MATCH;
}

// framing: the 18 bytes in front of a member of `size` bytes in all, the 8 behind its deflate block
// (byte k of each piece as a function, so that the device can or it into its word image without a local array)
BGZF_HD uint8_t bgzf_head_byte(uint32_t k, uint32_t size)
{
    // 1f 8b 08 04 | MTIME 0 | XFL 0, OS ff | XLEN 6 | 'B' 'C' 02 00 | BSIZE
    const uint64_t lo = 0x00000000'04088b1full, hi = 0x0002'4342'0006'ff00ull;
    if (k < 8u) return (uint8_t)(lo >> (8u * k));
    if (k < 16u) return (uint8_t)(hi >> (8u * (k - 8u)));
    return (uint8_t)((size - 1u) >> (8u * (k - 16u)));
}
BGZF_HD uint8_t bgzf_tail_byte(uint32_t k, uint32_t crc, uint32_t isize) { return (uint8_t)((k < 4u ? crc : isize) >> (8u * (k & 3u))); }
BGZF_HD uint8_t bgzf_stored_head_byte(uint32_t k, uint32_t n)
{
    if (k == 0u) return 1;  // BFINAL = 1, BTYPE = 00
    return (uint8_t)((k < 3u ? n : ~n) >> (8u * ((k - 1u) & 1u)));
}
BGZF_HD void bgzf_put_head(uint8_t *p, uint32_t size)
{
    for (uint32_t k = 0; k < BGZF_HEAD; k++) p[k] = bgzf_head_byte(k, size);
}
BGZF_HD void bgzf_put_tail(uint8_t *p, uint32_t crc, uint32_t isize)
{
    for (uint32_t k = 0; k < BGZF_TAIL; k++) p[k] = bgzf_tail_byte(k, crc, isize);
}
BGZF_HD void bgzf_put_stored_head(uint8_t *p, uint32_t n)
{
    for (uint32_t k = 0; k < 5u; k++) p[k] = bgzf_stored_head_byte(k, n);
}
// deflate bytes of total_bits; a block is stored when they are not below n + 5
BGZF_HD bool bgzf_is_stored(uint64_t total_bits, uint32_t n) { return (total_bits + 7u) / 8u >= (uint64_t)n + 5u; }

// ---- host only ----------------------------------------------------------------------------------------------------------------
// canonical codes of the lengths (RFC 1951, 3.2.2), bits reversed: the order deflate packs them in
static inline void bgzf_canonical(const uint8_t *lengths, int n, uint32_t *rev_codes)
{
    uint32_t count[17] = {0}, next[17] = {0}, code = 0;
    for (int k = 0; k < n; k++) count[lengths[k]]++;
    count[0] = 0;
    for (int bits = 1; bits <= 16; bits++) {
        code = (code + count[bits - 1]) << 1;
        next[bits] = code;
    }
    for (int k = 0; k < n; k++) {
        uint32_t c = next[lengths[k]]++, r = 0;
        for (int b = 0; b < lengths[k]; b++) { r = (r << 1) | (c & 1u); c >>= 1; }
        rev_codes[k] = r;
    }
}

static inline void bgzf_tables_build(BgzfTables *t)
{
    static const uint16_t len_base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    static const uint8_t len_extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    memset(t, 0, sizeof *t);
    uint32_t ll[286], dd[30];
    bgzf_canonical(BGZF_LITLEN_LENGTHS, 286, ll);
    bgzf_canonical(BGZF_DIST_LENGTHS, 30, dd);
    for (int b = 0; b < 256; b++) t->lit[b] = ll[b] | ((uint32_t)BGZF_LITLEN_LENGTHS[b] << 16);
    t->eob = ll[256] | ((uint32_t)BGZF_LITLEN_LENGTHS[256] << 16);
    for (uint32_t m = BGZF_MIN_MATCH; m <= BGZF_MAX_MATCH; m++) {
        int s = 28;
        while (len_base[s] > m) s--;
        const uint32_t cl = BGZF_LITLEN_LENGTHS[257 + s];
        t->len[m] = (ll[257 + s] | ((m - len_base[s]) << cl)) | ((cl + len_extra[s]) << 24);
    }
    for (int s = 0; s < 30; s++) t->dist[s] = dd[s] | ((uint32_t)BGZF_DIST_LENGTHS[s] << 16);
    for (uint32_t b = 0; b < 256; b++) {
        uint32_t c = b;
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1u) ? BGZF_CRC_POLY : 0u);
        t->crc[b] = c;
    }
    uint32_t x8 = 0x80000000u >> 8;  // x^8
    t->xp1[0] = 0x80000000u;
    for (uint32_t r = 1; r < BGZF_CRC_CHUNK; r++) t->xp1[r] = bgzf_crc_mul(t->xp1[r - 1], x8);
    const uint32_t x256 = bgzf_crc_mul(t->xp1[BGZF_CRC_CHUNK - 1], x8);
    t->xp32[0] = 0x80000000u;
    for (uint32_t k = 1; k < BGZF_CRC_CHUNKS; k++) t->xp32[k] = bgzf_crc_mul(t->xp32[k - 1], x256);
    for (uint32_t k = 0; k < BGZF_HEADER_WORDS; k++) t->header[k] = BGZF_HEADER[k];
}

// `bits` (n_bits of them, LSB first) or-ed into the zeroed byte image at bit `at`
static inline void bgzf_or_bits(uint8_t *image, uint64_t at, uint64_t bits, uint32_t n_bits)
{
    for (uint32_t k = 0; k < n_bits; k++, at++)
        if ((bits >> k) & 1u) image[at >> 3] |= (uint8_t)(1u << (at & 7u));
}

// One block of 1..BGZF_PAYLOAD bytes as its BGZF member at out (room for BGZF_MAX_MEMBER + 8 bytes); returns the member's size.
// The serial restatement of bgzf.member: segments, d, eq, runs cut into pieces of 258, tails below 3 as literals, the preset's
// bits, the stored form when those are not smaller, the CRC from chunks as the device combines them.
static inline uint32_t bgzf_encode_block_host(const BgzfTables *t, const uint8_t *in, uint32_t n, uint8_t *out, bool *stored_out)
{
    // d and eq of every position
    uint16_t *d = new uint16_t[n];
    uint8_t *eq = new uint8_t[n];
    uint32_t seg = 0, prev = 0;  // first byte of the position's segment / of the one before
    bool has = false;
    for (uint32_t p = 0; p < n; p++) {
        d[p] = has ? (uint16_t)(seg - prev) : 0;
        eq[p] = has && in[p] == in[p - d[p]];
        if (in[p] == '\n') { prev = seg; seg = p + 1; has = true; }
    }
    // two passes over the tokens: the bits, then (unless stored) the image
    uint8_t *body = out + BGZF_HEAD;
    uint64_t total = 0;
    bool stored = false;
    for (int pass = 0; pass < 2 && !stored; pass++) {
        uint64_t at = BGZF_HEADER_BITS;
        if (pass == 1) {
            memset(body, 0, (size_t)((total + 7u) / 8u));
            for (uint32_t k = 0; k < BGZF_HEADER_BITS; k++)
                if ((t->header[k >> 5] >> (k & 31u)) & 1u) body[k >> 3] |= (uint8_t)(1u << (k & 7u));
        }
        for (uint32_t p = 0; p < n;) {
            uint32_t e = p + 1, nb;
            uint64_t v;
            if (eq[p])
                while (e < n && eq[e] && d[e] == d[p]) e++;  // the run [p, e)
            if (!eq[p]) {
                v = bgzf_literal_bits(t->lit, in[p], &nb);
                if (pass) bgzf_or_bits(body, at, v, nb);
                at += nb;
                p++;
                continue;
            }
            for (uint32_t q = p; q < e;) {
                uint32_t o;
                const uint32_t piece = bgzf_piece(q, p, e, &o);
                if (piece >= BGZF_MIN_MATCH) {
                    v = bgzf_match_bits(t->len, t->dist, piece, d[p], &nb);
                    if (pass) bgzf_or_bits(body, at, v, nb);
                    at += nb;
                    q += piece;
                } else {
                    v = bgzf_literal_bits(t->lit, in[q], &nb);
                    if (pass) bgzf_or_bits(body, at, v, nb);
                    at += nb;
                    q++;
                }
            }
            p = e;
        }
        if (pass) bgzf_or_bits(body, at, t->eob & 0xffffu, t->eob >> 16);
        at += t->eob >> 16;
        if (pass == 0) {
            total = at;
            stored = bgzf_is_stored(total, n);
        }
    }
    delete[] d;
    delete[] eq;
    uint32_t body_bytes = (uint32_t)((total + 7u) / 8u);
    if (stored) {
        bgzf_put_stored_head(body, n);
        memcpy(body + 5, in, n);
        body_bytes = n + 5u;
    }
    // the CRC as the device forms it: chunks of 32 bytes aligned to the end, each moved over what follows it
    uint32_t X = 0;
    for (uint32_t k = 0; k * BGZF_CRC_CHUNK < n; k++) {
        const uint32_t hi = n - k * BGZF_CRC_CHUNK, lo = hi >= BGZF_CRC_CHUNK ? hi - BGZF_CRC_CHUNK : 0;
        uint32_t s = 0;
        for (uint32_t p = lo; p < hi; p++) s = bgzf_crc_byte(t->crc, s, in[p]);
        X ^= bgzf_crc_mul(s, t->xp32[k]);
    }
    const uint32_t size = BGZF_HEAD + body_bytes + BGZF_TAIL;
    bgzf_put_head(out, size);
    bgzf_put_tail(body + body_bytes, bgzf_crc_finish(t->xp32, t->xp1, X, n), n);
    if (stored_out) *stored_out = stored;
    return size;
}
