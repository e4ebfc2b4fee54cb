// cellector_bgzf_compress / cellector_write_mtx_bgzf: text on the device as a BGZF stream (bgzf_format.h; cellector_amd/bgzf.py is the
// byte-identical twin and states the format).
//
// k_bz_block: one workgroup of 1024 threads per block of BGZF_PAYLOAD = 32640 bytes, thread t owns the positions [32 t, 32 t + 32).
//   load     the block's text into LDS with 16-byte loads; the word image of the member is zeroed
//   newlines every thread finds the newlines among its bytes; an exclusive scan of "the last two newlines" gives it the start of the
//            segment it opens in and of the one before: d = their difference
//   eq       eq[p] = text[p] == text[p - d], link[p] = eq[p] & eq[p + 1] & (d[p] == d[p + 1]), as two 32-bit masks per thread; a run
//            starts behind the last unlinked position before p (forward max-scan) and ends at the first one from p on (backward
//            min-scan)
//   bits     a walk over the thread's positions adds up the bits of the tokens that start there; an exclusive scan places them; the
//            block's total decides preset or stored
//   emit     the same walk ors every token's bits (at most three words) into the image with LDS atomics: or commutes, so the bytes
//            do not depend on the order of the lanes.  A stored block copies its text behind the 5-byte stored header instead.
//   crc      every thread takes the CRC state of one 32-byte chunk, chunks aligned to the block's end, moves it over the bytes behind
//            it (a multiplication mod P by a tabulated power of x), and the block xors them
//   out      header, trailer; the image goes to the block's slot (BZ_SLOT bytes each) in 16-byte stores, its size to sizes[block]
// k_bz_compact: after dev_exclusive_scan_u64 over the sizes, one workgroup per block moves its slot to its place in the stream with
//   aligned 16-byte stores (the slot read as aligned words and funnel-shifted); head and tail units shared with a neighbour bytewise.
// LDS: 32 KiB of text + 31.9 KiB of image + 3.1 KiB of tables (literal, length, distance, CRC) + scan scratch = 68.9 KB: two
// workgroups per CU.  The bytes depend neither on the grid nor on how the caller windows the text: a block is a function of its
// 32640 bytes alone.
#include "ctx.h"
#include "bgzf_format.h"

#define BZ_THREADS 1024
#define BZ_PER 32                                  // positions of a thread
#define BZ_WAVES (BZ_THREADS / 64)
#define BZ_TEXT_BYTES (BZ_THREADS * BZ_PER)        // 32768 >= BGZF_PAYLOAD
#define BZ_SLOT ((BGZF_MAX_MEMBER + 15u) / 16u * 16u)  // 32672: a member's image and its slot
#define BZ_COMPACT_THREADS 256
#define BZ_CHUNK_BLOCKS 2048ull                    // blocks per launch of cellector_bgzf_compress: 64 MB of text

static_assert(BGZF_PAYLOAD % 16u == 0 && BGZF_PAYLOAD <= BZ_TEXT_BYTES, "a block's text is whole 16-byte units in LDS");
static_assert(BGZF_CRC_CHUNK == BZ_PER && BGZF_CRC_CHUNKS >= BZ_THREADS, "one CRC chunk per thread");

// Exclusive scan over the block's threads under op(earlier, later); REV: over the threads behind.  wt: [BZ_WAVES] in LDS.
template <bool REV, typename Op>
__device__ __forceinline__ uint32_t bz_scan(uint32_t v, uint32_t ident, Op op, uint32_t *wt)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = REV ? __shfl_down(inc, off, 64) : __shfl_up(inc, off, 64);
        if (REV ? lane + off < 64 : lane >= off) inc = REV ? op(inc, o) : op(o, inc);
    }
    __syncthreads();  // (wt may still be read from the scan before)
    if (lane == (REV ? 0 : 63)) wt[w] = inc;
    __syncthreads();
    uint32_t ex = REV ? __shfl_down(inc, 1, 64) : __shfl_up(inc, 1, 64);
    if (lane == (REV ? 63 : 0)) ex = ident;
    uint32_t rest = ident;  // the waves before (behind) this one
    if (REV) {
        for (int j = BZ_WAVES - 1; j > w; j--) rest = op(wt[j], rest);
        return op(ex, rest);
    }
    for (int j = 0; j < w; j++) rest = op(rest, wt[j]);
    return op(rest, ex);
}

// the last two newlines before a position as (last + 1) | (the one before + 1) << 16, 0 = none
__device__ __forceinline__ uint32_t bz_last_two(uint32_t earlier, uint32_t later)
{
    if ((later & 0xffffu) == 0u) return earlier;
    if ((later >> 16) == 0u) return (later & 0xffffu) | (earlier << 16);
    return later;
}

// v (n_bits <= 48 of them, LSB first) or-ed into the zeroed word image at bit `at`
__device__ __forceinline__ void bz_or(uint32_t *image, uint32_t at, uint64_t v)
{
    const uint32_t wi = at >> 5, sh = at & 31u;
    const uint64_t lo = v << sh;
    const uint32_t p0 = (uint32_t)lo, p1 = (uint32_t)(lo >> 32), p2 = sh ? (uint32_t)(v >> (64u - sh)) : 0u;
    if (p0) atomicOr(&image[wi], p0);
    if (p1) atomicOr(&image[wi + 1], p1);
    if (p2) atomicOr(&image[wi + 2], p2);
}
__device__ __forceinline__ void bz_or_byte(uint32_t *image, uint32_t byte_at, uint8_t b)
{
    if (b) atomicOr(&image[byte_at >> 2], (uint32_t)b << (8u * (byte_at & 3u)));
}

// The thread's positions [c, c + 32) below n, in order: the tokens that start there.  EMIT = false adds up their bits; EMIT = true
// ors them into the image from bit `at` on.  Returns the bits.  (a, b): the segment starts at c, as bz_last_two leaves them; s_in /
// e_in: the run start / end the scans give for what the thread's own masks do not decide.
template <bool EMIT>
__device__ __forceinline__ uint32_t bz_walk(const uint32_t *text32, uint32_t c, uint32_t n, uint32_t nl, uint32_t eq, uint32_t brk,
                                            uint32_t a, uint32_t b, uint32_t s_in, uint32_t e_in, const uint32_t *lit,
                                            const uint32_t *len_tab, const uint32_t *dist_tab, uint32_t *image, uint32_t at)
{
    uint32_t s = s_in, bits = 0;
    for (uint32_t j = 0; j < BZ_PER / 4 && c + 4u * j < n; j++) {
        const uint32_t word = text32[(c >> 2) + j];
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) {
            const uint32_t k = 4u * j + i, p = c + k;
            if (p < n) {
                bool in_match = false;
                uint32_t piece = 0, o = 0;
                if ((eq >> k) & 1u) {
                    const uint32_t m = brk >> k, e = m ? p + (uint32_t)__ffs((int)m) : e_in;
                    piece = bgzf_piece(p, s, e, &o);
                    in_match = piece >= BGZF_MIN_MATCH;
                }
                if (!in_match || o == 0u) {
                    uint32_t nb;
                    const uint64_t v = in_match ? bgzf_match_bits(len_tab, dist_tab, piece, a - b, &nb)
                                                : bgzf_literal_bits(lit, (uint8_t)(word >> (8u * i)), &nb);
                    if (EMIT) bz_or(image, at + bits, v);
                    bits += nb;
                }
            }
            if ((brk >> k) & 1u) s = p + 1u;
            if ((nl >> k) & 1u) { b = a; a = p + 1u; }
        }
    }
    return bits;
}

// (8 waves per SIMD asked for: two workgroups per CU, as the LDS allows.  Without it the kernel takes 106 SGPRs, seven waves per
// SIMD, one workgroup per CU, and 1.35 times as long.)
__global__ __launch_bounds__(BZ_THREADS, 8) void k_bz_block(const uint8_t *__restrict__ text /*16-byte aligned*/, uint64_t n_text,
                                                         const BgzfTables *__restrict__ tab, uint8_t *__restrict__ slots,
                                                         uint64_t *__restrict__ sizes, unsigned long long *__restrict__ n_stored)
{
    __shared__ __attribute__((aligned(16))) uint32_t text32[BZ_TEXT_BYTES / 4];
    __shared__ __attribute__((aligned(16))) uint32_t image[BZ_SLOT / 4];
    __shared__ uint32_t lds_tab[BGZF_LDS_TABLE_WORDS];
    __shared__ uint32_t wt[BZ_WAVES];
    const uint8_t *text8 = reinterpret_cast<const uint8_t *>(text32);
    const uint32_t *lit = lds_tab, *len_tab = lds_tab + 256, *dist_tab = lds_tab + 516, *crc_tab = lds_tab + 548;
    const uint32_t t = threadIdx.x, c = t * BZ_PER;
    const uint64_t first = (uint64_t)blockIdx.x * BGZF_PAYLOAD;
    const uint32_t n = (uint32_t)(n_text - first < BGZF_PAYLOAD ? n_text - first : BGZF_PAYLOAD);  // 1..BGZF_PAYLOAD
    const uint8_t *src = text + first;

    // ---- load: text (zeros behind n), a zeroed image, the tables
    for (uint32_t u = t; u < BZ_TEXT_BYTES / 16; u += BZ_THREADS) {
        uint4 v = make_uint4(0, 0, 0, 0);
        const uint32_t b0 = u * 16u;
        if (b0 + 16u <= n) {
            v = *reinterpret_cast<const uint4 *>(src + b0);
        } else if (b0 < n) {
            uint32_t w[4] = {0, 0, 0, 0};
            for (uint32_t k = b0; k < n; k++) w[(k - b0) >> 2] |= (uint32_t)src[k] << (8u * (k & 3u));
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        reinterpret_cast<uint4 *>(text32)[u] = v;
    }
    for (uint32_t u = t; u < BZ_SLOT / 16; u += BZ_THREADS) reinterpret_cast<uint4 *>(image)[u] = make_uint4(0, 0, 0, 0);
    for (uint32_t k = t; k < BGZF_LDS_TABLE_WORDS; k += BZ_THREADS) lds_tab[k] = reinterpret_cast<const uint32_t *>(tab)[k];  // lit, len, dist, crc: the head of BgzfTables
    __syncthreads();

    // ---- newlines: the thread's mask, the two segment starts it opens with
    uint32_t nl = 0;
    for (uint32_t j = 0; j < BZ_PER / 4; j++) {
        const uint32_t word = text32[(c >> 2) + j];
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) nl |= (uint32_t)(((word >> (8u * i)) & 0xffu) == 10u) << (4u * j + i);
    }
    uint32_t mine = 0;
    if (nl) {
        const uint32_t hi = 31u - (uint32_t)__clz((int)nl), rest = nl & ~(1u << hi);
        mine = (c + hi + 1u) | (rest ? (c + 32u - (uint32_t)__clz((int)rest)) << 16 : 0u);
    }
    const uint32_t seg = bz_scan<false>(mine, 0u, bz_last_two, wt);
    const uint32_t a0 = seg & 0xffffu, b0 = seg >> 16;

    // ---- eq and link of the thread's positions
    uint32_t eq = 0, link = 0;
    {
        uint32_t a = a0, b = b0, d_before = 0;
        bool eq_before = false;
        for (uint32_t k = 0; k <= BZ_PER; k++) {
            const uint32_t p = c + k;
            bool e = false;
            const uint32_t d = a - b;
            if (p < n && a != 0u) e = text8[p] == text8[p - d];
            if (k > 0 && eq_before && e && d == d_before) link |= 1u << (k - 1u);
            if (k < BZ_PER) {
                eq |= (uint32_t)e << k;
                if ((nl >> k) & 1u) { b = a; a = p + 1u; }
            }
            eq_before = e;
            d_before = d;
        }
    }
    const uint32_t brk = ~link;  // a run ends behind these positions
    const uint32_t s_in = bz_scan<false>(brk ? c + 32u - (uint32_t)__clz((int)brk) : 0u, 0u,
                                         [](uint32_t x, uint32_t y) { return x > y ? x : y; }, wt);
    const uint32_t e_in = bz_scan<true>(brk ? c + (uint32_t)__ffs((int)brk) : 0xffffffffu, 0xffffffffu,
                                        [](uint32_t x, uint32_t y) { return x < y ? x : y; }, wt);

    // ---- bits: the tokens' sizes, their places, preset or stored
    const uint32_t my_bits = bz_walk<false>(text32, c, n, nl, eq, brk, a0, b0, s_in, e_in, lit, len_tab, dist_tab, image, 0u);
    const uint32_t bits_before = bz_scan<false>(my_bits, 0u, [](uint32_t x, uint32_t y) { return x + y; }, wt);
    uint32_t token_bits = 0;  // (wt holds the waves' sums)
#pragma unroll
    for (int j = 0; j < BZ_WAVES; j++) token_bits += wt[j];
    const uint32_t eob = tab->eob, total_bits = BGZF_HEADER_BITS + token_bits + (eob >> 16);
    const bool stored = bgzf_is_stored(total_bits, n);
    const uint32_t body = stored ? n + 5u : (total_bits + 7u) / 8u, size = BGZF_HEAD + body + BGZF_TAIL;

    // ---- crc: the chunk [n - 32 (t + 1), n - 32 t), moved over the 32 t bytes behind it
    uint32_t X = 0;
    if (t * BGZF_CRC_CHUNK < n) {
        const uint32_t hi = n - t * BGZF_CRC_CHUNK, lo = hi >= BGZF_CRC_CHUNK ? hi - BGZF_CRC_CHUNK : 0u;
        uint32_t state = 0;
        for (uint32_t p = lo; p < hi; p++) state = bgzf_crc_byte(crc_tab, state, text8[p]);
        X = bgzf_crc_mul(state, tab->xp32[t]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) X ^= __shfl_xor(X, off, 64);
    __syncthreads();  // (the sums in wt have been read)
    if ((t & 63u) == 0u) wt[t >> 6] = X;

    // ---- emit
    if (stored) {
        uint8_t *image8 = reinterpret_cast<uint8_t *>(image);
        for (uint32_t k = 0; k < BZ_PER && c + k < n; k++) image8[BGZF_HEAD + 5u + c + k] = text8[c + k];
    } else {
        const uint32_t at0 = BGZF_HEAD * 8u + BGZF_HEADER_BITS;
        if (t < BGZF_HEADER_WORDS) bz_or(image, BGZF_HEAD * 8u + 32u * t, tab->header[t]);
        bz_walk<true>(text32, c, n, nl, eq, brk, a0, b0, s_in, e_in, lit, len_tab, dist_tab, image, at0 + bits_before);
        if (t == 0) bz_or(image, at0 + token_bits, eob & 0xffffu);
    }
    __syncthreads();
    if (t < 64u) {  // header, stored header, trailer: bytes or-ed into words that the body shares
        X = 0;
#pragma unroll
        for (int j = 0; j < BZ_WAVES; j++) X ^= wt[j];
        const uint32_t crc = bgzf_crc_finish(tab->xp32, tab->xp1, X, n);
        if (t < BGZF_HEAD) bz_or_byte(image, t, bgzf_head_byte(t, size));
        else if (t < BGZF_HEAD + BGZF_TAIL) bz_or_byte(image, BGZF_HEAD + body + (t - BGZF_HEAD), bgzf_tail_byte(t - BGZF_HEAD, crc, n));
        else if (stored && t < BGZF_HEAD + BGZF_TAIL + 5u)
            bz_or_byte(image, BGZF_HEAD + (t - BGZF_HEAD - BGZF_TAIL), bgzf_stored_head_byte(t - BGZF_HEAD - BGZF_TAIL, n));
    }
    __syncthreads();

    // ---- out: whole 16-byte units of the slot (the image is zero behind the member)
    uint4 *dst = reinterpret_cast<uint4 *>(slots + (uint64_t)blockIdx.x * BZ_SLOT);
    for (uint32_t u = t; u < (size + 15u) / 16u; u += BZ_THREADS) dst[u] = reinterpret_cast<const uint4 *>(image)[u];
    if (t == 0) {
        sizes[blockIdx.x] = size;
        if (stored) atomicAdd(n_stored, 1ull);
    }
}

// slot b's first (off[b + 1] - off[b]) bytes -> out[off[b] ..): out is 16-byte aligned, unit u of it is written by one thread
__global__ __launch_bounds__(BZ_COMPACT_THREADS) void k_bz_compact(const uint8_t *__restrict__ slots, const uint64_t *__restrict__ off,
                                                                   uint8_t *__restrict__ out)
{
    const uint64_t o0 = off[blockIdx.x], o1 = off[blockIdx.x + 1];
    const uint8_t *src = slots + (uint64_t)blockIdx.x * BZ_SLOT;
    const uint32_t *src32 = reinterpret_cast<const uint32_t *>(src);
    for (uint64_t u = (o0 >> 4) + threadIdx.x; u * 16u < o1; u += BZ_COMPACT_THREADS) {
        const uint64_t b0 = u * 16u;
        if (b0 >= o0 && b0 + 16u <= o1) {
            const uint32_t s0 = (uint32_t)(b0 - o0), q = s0 >> 2, sh = 8u * (s0 & 3u);
            uint32_t w[5];
#pragma unroll
            for (int k = 0; k < 4; k++) w[k] = src32[q + k];
            w[4] = sh ? src32[q + 4] : 0u;  // (inside the slot: s0 + 20 <= the member's size + 4 <= BZ_SLOT)
            uint4 v;
            v.x = sh ? (w[0] >> sh) | (w[1] << (32u - sh)) : w[0];
            v.y = sh ? (w[1] >> sh) | (w[2] << (32u - sh)) : w[1];
            v.z = sh ? (w[2] >> sh) | (w[3] << (32u - sh)) : w[2];
            v.w = sh ? (w[3] >> sh) | (w[4] << (32u - sh)) : w[3];
            *reinterpret_cast<uint4 *>(out + b0) = v;
        } else {
            const uint64_t lo = b0 < o0 ? o0 : b0, hi = b0 + 16u < o1 ? b0 + 16u : o1;
            for (uint64_t p = lo; p < hi; p++) out[p] = src[p - o0];
        }
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------
BzScratch::~BzScratch()
{
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
}

uint64_t bz_blocks(uint64_t text_bytes) { return (text_bytes + BGZF_PAYLOAD - 1) / BGZF_PAYLOAD; }
uint64_t bz_out_capacity(uint64_t blocks) { return blocks * BZ_SLOT + 16; }

cellector_status bz_scratch(cellector_ctx *c, BzScratch *s, uint64_t cap_blocks)
{
    s->cap_blocks = cap_blocks;
    CHK(dev_alloc(c, &s->tables, sizeof(BgzfTables)));
    CHK(dev_alloc(c, &s->slots, bz_out_capacity(cap_blocks)));
    CHK(dev_alloc(c, &s->sizes, cap_blocks + 1));
    CHK(dev_alloc(c, &s->stored, 1));
    BgzfTables *t = new BgzfTables;
    bgzf_tables_build(t);
    const hipError_t e = hipMemcpyAsync(s->tables, t, sizeof *t, hipMemcpyHostToDevice, c->stream);
    const hipError_t e2 = hipStreamSynchronize(c->stream);
    delete t;
    HIPCHK(c, e);
    HIPCHK(c, e2);
    if (getenv("CELLECTOR_TIMING")) {
        for (hipEvent_t &ev : s->ev) HIPCHK(c, hipEventCreate(&ev));
        s->timed = true;
    }
    return CELLECTOR_OK;
}

// The n bytes of device text (16-byte aligned, at most s->cap_blocks blocks) as BGZF members, no EOF member: their bytes, blocks and
// stored blocks; with `out` (device, 16-byte aligned, bz_out_capacity(blocks) bytes) also the members, one behind the other.  The
// compaction is queued, not awaited.
cellector_status bz_compress(cellector_ctx *c, BzScratch *s, const uint8_t *text, uint64_t n, uint8_t *out, uint64_t *bytes,
                             uint64_t *blocks, uint64_t *stored)
{
    *bytes = *blocks = *stored = 0;
    if (n == 0) return CELLECTOR_OK;
    const uint64_t nb = bz_blocks(n);
    if (nb > s->cap_blocks) return ctx_fail(c, CELLECTOR_EINVAL, "bgzf: %llu blocks for a scratch of %llu", (unsigned long long)nb, (unsigned long long)s->cap_blocks);
    HIPCHK(c, hipMemsetAsync(s->stored, 0, 8, c->stream));
    HIPCHK(c, hipMemsetAsync(s->sizes + nb, 0, 8, c->stream));
    if (s->timed) HIPCHK(c, hipEventRecord(s->ev[0], c->stream));
    hipLaunchKernelGGL(k_bz_block, dim3((unsigned)nb), dim3(BZ_THREADS), 0, c->stream, text, n, (const BgzfTables *)(const void *)s->tables.get(),
                       s->slots.get(), s->sizes.get(), s->stored.get());
    HIPCHK(c, hipGetLastError());
    if (s->timed) HIPCHK(c, hipEventRecord(s->ev[1], c->stream));
    unsigned long long st = 0;
    HIPCHK(c, hipMemcpyAsync(&st, s->stored, 8, hipMemcpyDeviceToHost, c->stream));
    CHK(dev_exclusive_scan_u64(c, s->sizes, nb + 1, bytes));  // (synchronises: st has arrived)
    *blocks = nb;
    *stored = st;
    float ms = 0;
    if (s->timed && hipEventElapsedTime(&ms, s->ev[0], s->ev[1]) == hipSuccess) s->ms_block += ms;
    if (out) {
        if (s->timed) HIPCHK(c, hipEventRecord(s->ev[2], c->stream));
        hipLaunchKernelGGL(k_bz_compact, dim3((unsigned)nb), dim3(BZ_COMPACT_THREADS), 0, c->stream, (const uint8_t *)s->slots.get(),
                           (const uint64_t *)s->sizes.get(), out);
        HIPCHK(c, hipGetLastError());
        if (s->timed) {
            HIPCHK(c, hipEventRecord(s->ev[3], c->stream));
            HIPCHK(c, hipEventSynchronize(s->ev[3]));
            if (hipEventElapsedTime(&ms, s->ev[2], s->ev[3]) == hipSuccess) s->ms_compact += ms;
        }
    }
    return CELLECTOR_OK;
}

// cellector_bgzf_compress behind its checks: host bytes in chunks of BZ_CHUNK_BLOCKS blocks through the device
cellector_status bgzf_compress_host(cellector_ctx *c, const uint8_t *in, uint64_t n, uint8_t *out, uint64_t capacity, uint64_t *n_out,
                                    uint64_t *n_blocks)
{
    const uint64_t chunk = BZ_CHUNK_BLOCKS * BGZF_PAYLOAD, n_chunks = (n + chunk - 1) / chunk;
    const uint64_t cap_blocks = bz_blocks(n < chunk ? n : chunk);
    BzScratch s;
    DevBuf<uint8_t> text, packed;
    if (n) {
        CHK(bz_scratch(c, &s, cap_blocks));
        CHK(dev_alloc(c, &text, cap_blocks * BGZF_PAYLOAD));
        if (out) CHK(dev_alloc(c, &packed, bz_out_capacity(cap_blocks)));
    }
    auto run = [&](uint64_t k, uint8_t *dev_out, uint64_t *bytes, uint64_t *blocks) -> cellector_status {
        const uint64_t at = k * chunk, m = n - at < chunk ? n - at : chunk;
        uint64_t stored;
        HIPCHK(c, hipMemcpyAsync(text, in + at, m, hipMemcpyHostToDevice, c->stream));
        return bz_compress(c, &s, text, m, dev_out, bytes, blocks, &stored);
    };
    // the sizes: of a single chunk they come with its one compression, of several from a pass of their own
    uint64_t total = BGZF_EOF_BYTES, blocks = 0, b1 = 0, k1 = 0;
    if (n_chunks == 1) {
        CHK(run(0, out ? packed.get() : nullptr, &b1, &k1));
        total += b1;
        blocks = k1;
    } else {
        for (uint64_t k = 0; k < n_chunks; k++) {
            uint64_t b, kb;
            CHK(run(k, nullptr, &b, &kb));
            total += b;
            blocks += kb;
        }
    }
    *n_out = total;
    *n_blocks = blocks;
    if (!out) return CELLECTOR_OK;
    if (capacity < total)
        return ctx_fail(c, CELLECTOR_EINVAL, "bgzf_compress: capacity %llu is below the %llu bytes of the stream", (unsigned long long)capacity,
                        (unsigned long long)total);
    uint64_t done = 0;
    if (n_chunks == 1) {
        CHK(d2h(c, out, packed, b1));
        done = b1;
    } else {
        for (uint64_t k = 0; k < n_chunks; k++) {
            uint64_t b, kb;
            CHK(run(k, packed, &b, &kb));
            CHK(d2h(c, out + done, packed, b));
            done += b;
        }
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    memcpy(out + done, BGZF_EOF, BGZF_EOF_BYTES);
    return CELLECTOR_OK;
}
