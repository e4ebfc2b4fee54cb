// cellector_bgzf_decompress / option gz_device: the members of a BGZF stream inflated on the device (inflate_format.h holds the format
// and the pieces this kernel shares with the serial host decoder).
//
// k_bgzf_inflate: one wave per member, INF_WAVES waves per workgroup.  A wave works in rounds:
//   ring     all lanes bring the member's next input bytes into a 1 KB ring in LDS (byte i lives at i mod 1024; only bytes below the
//            body's length are ever fetched), so that the serial lane reads LDS, not HBM
//   decode   lane 0 runs the symbol loop on a 64-bit bit buffer (inf_fill / inf_token) and puts up to 64 tokens (a literal, or a
//            length with its distance) into a token ring in LDS; it returns when the ring is full, when it has used 512 bytes of
//            input, or at an event: a block header read (the wave builds the tables), a stored block (the wave copies it), the
//            end of the stream, a refusal.  It checks every token against the bytes produced and against ISIZE before it emits it.
//   expand   a wave scan of the token lengths gives every token its place; the literals are stored first, then the matches in token
//            order, each by all lanes with src[j mod distance] (right for overlapping matches: the source is complete before)
//   tables   lane 0 has left the code lengths in LDS (inf_read_lengths) or the block is a fixed one; the wave ranks the symbols by
//            (length, symbol) with ballots, checks the counts by inf_code_rule, and fills the primary tables entry by entry with
//            inf_fast_entry
//   crc      after the last block: every lane takes the raw CRC state of one span of the text (spans of a multiple of 32 bytes,
//            aligned to the member's END), moves it over the bytes behind it by a tabulated power of x, the wave xors them
// LDS: 4944 B per wave (tables 3656 B, input ring 1032 B, tokens 256 B) + the CRC byte table 1 KB per workgroup: 20 800 B for 4 waves.
// Bounds: see inflate_format.h; every index into LDS is masked or clamped, every global store is below the member's isize, every
// global load of text is below the bytes produced, the member's ranges are checked against both buffers before anything else.
// The status word (64 bits, as the tokeniser's bad[]): the smallest (member << 8 | INF_E_ kind) over the launches since it was set to
// ~0, which it stays when no member was refused; member = first_index + the member's place in the launch.
#include "ctx.h"
#include "inflate_format.h"
#include "mtx_bytes.h"

#define INF_WAVES 4
#define INF_THREADS (64 * INF_WAVES)
#define INF_RING 1024u   // bytes of the input ring (a power of two)
#define INF_RUN 512u     // input bytes after which lane 0 hands back: a step behind that uses at most 286 (a dynamic header)
#define INF_BATCH 64u    // tokens of a round
#define INF_CHUNK_MEMBERS 2048ull  // members per launch of cellector_bgzf_decompress: at most 128 MB of text

static_assert(INF_RUN + 286u + 8u + 48u <= INF_RING, "the ring holds what a run of lane 0 may read");

struct InfWave {
    InfTables t;
    __attribute__((aligned(8))) uint8_t ring[INF_RING + 8];  // (the first 8 bytes once more behind the end: an 8-byte read never wraps)
    uint32_t tok[INF_BATCH];
};

enum { INF_EV_BATCH = 0, INF_EV_FIXED, INF_EV_DYNAMIC, INF_EV_STORED, INF_EV_DONE, INF_EV_ERROR };

// what a wave's lanes wrote to LDS is read by its other lanes: the LDS instructions of one wave execute in order, the compiler
// must keep them so
__device__ __forceinline__ void inf_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// count[] and sym[] of lens[0..n), n <= 64 CHUNKS, by the wave: the rank of a symbol among those of its length is the number before
// it, counted with ballots.  offs: 16 words of scratch in LDS.
template <int CHUNKS>
__device__ __forceinline__ void inf_rank_wave(const uint8_t *lens, uint32_t n, uint16_t *count, uint16_t *sym, uint32_t cap, uint16_t *offs,
                                              uint32_t lane)
{
    uint32_t cnt[16], l[CHUNKS], r[CHUNKS];
#pragma unroll
    for (int k = 0; k < 16; k++) cnt[k] = 0;
    const uint64_t below = (1ull << lane) - 1ull;
#pragma unroll
    for (int c = 0; c < CHUNKS; c++) {
        const uint32_t s = 64u * c + lane;
        l[c] = s < n ? (lens[s] & 15u) : 0u;
        r[c] = 0;
#pragma unroll
        for (int k = 1; k < 16; k++) {
            const uint64_t m = __ballot(l[c] == (uint32_t)k);
            if (l[c] == (uint32_t)k) r[c] = cnt[k] + (uint32_t)__popcll(m & below);
            cnt[k] += (uint32_t)__popcll(m);
        }
    }
    uint32_t mine = 0, before = 0, run = 0;  // lane k < 16: count[k], and the symbols of shorter codes
#pragma unroll
    for (int k = 1; k < 16; k++) {
        if (lane == (uint32_t)k) { mine = cnt[k]; before = run; }
        run += cnt[k];
    }
    if (lane < 16u) { count[lane] = (uint16_t)mine; offs[lane] = (uint16_t)before; }
    inf_wave_sync();
#pragma unroll
    for (int c = 0; c < CHUNKS; c++)
        if (l[c]) {
            const uint32_t at = offs[l[c]] + r[c];
            sym[at < cap ? at : cap - 1u] = (uint16_t)(64u * c + lane);
        }
    inf_wave_sync();
}

// the tables of t->lens[0..nlen) and t->lens[INF_NLEN..INF_NLEN + ndist) (zeros behind both); INF_OK or why the lengths are refused
__device__ __forceinline__ int inf_build_wave(InfTables *t, uint32_t nlen, uint32_t ndist, uint32_t lane)
{
    inf_rank_wave<5>(t->lens, nlen, t->lcount, t->lsym, INF_NLEN, t->ccount, lane);
    inf_rank_wave<1>(t->lens + INF_NLEN, ndist, t->dcount, t->dsym, INF_NDIST, t->ccount, lane);
    int e = inf_code_rule(t->lcount, 1);
    if (!e) e = inf_code_rule(t->dcount, 2);
    if (e) return e;
    for (uint32_t i = lane; i < (1u << INF_LFAST_BITS); i += 64u) t->lfast[i] = inf_fast_entry(t->lcount, t->lsym, INF_NLEN, i, INF_LFAST_BITS);
    for (uint32_t i = lane; i < (1u << INF_DFAST_BITS); i += 64u) t->dfast[i] = inf_fast_entry(t->dcount, t->dsym, INF_NDIST, i, INF_DFAST_BITS);
    inf_wave_sync();
    return INF_OK;
}

__global__ __launch_bounds__(INF_THREADS) void k_bgzf_inflate(const uint8_t *__restrict__ in, uint64_t n_in, const InfMember *__restrict__ members,
                                                              uint32_t n_members, uint8_t *out_base /*read back: not restrict*/, uint64_t out_cap,
                                                              const InfCrcTables *__restrict__ crc_tab, uint64_t first_index,
                                                              unsigned long long *__restrict__ status)
{
    __shared__ InfWave waves[INF_WAVES];
    __shared__ uint32_t crc_lds[256];
    for (uint32_t k = threadIdx.x; k < 256u; k += INF_THREADS) crc_lds[k] = crc_tab->crc[k];
    __syncthreads();  // (the only workgroup barrier: behind it the waves go their own ways)
    const uint32_t lane = threadIdx.x & 63u, index = blockIdx.x * INF_WAVES + (threadIdx.x >> 6);
    if (index >= n_members) return;
    InfWave *w = &waves[threadIdx.x >> 6];
    const InfMember m = members[index];
    const uint32_t n = m.in_len, isize = m.isize;
    int err = INF_OK;
    // the member's ranges lie inside the two buffers, or nothing of it is touched
    if (m.in_off > n_in || n > n_in - m.in_off) err = INF_E_INPUT;
    else if (isize > INF_MAX_OUT || m.out_off > out_cap || isize > out_cap - m.out_off) err = INF_E_OUTPUT;
    const uint8_t *src = in + m.in_off;
    uint8_t *out = out_base + m.out_off;
    const uint8_t *ring = w->ring;
    auto fill = [ring](InfBits *r) {  // (8 bytes of the ring in one read; what lies at n and behind is masked by inf_fill8's caller rule)
        inf_fill8(r, [ring, r](uint32_t p) {
            uint64_t v;
            __builtin_memcpy(&v, ring + (p & (INF_RING - 1u)), 8);
            const uint32_t valid = r->n - p;  // (p < n)
            return valid < 8u ? v & ((1ull << (8u * valid)) - 1ull) : v;
        });
    };

    // lane 0's own state
    InfBits b;
    inf_bits_init(&b, n);
    bool last = false, in_block = false;
    uint32_t emitted = 0;  // bytes of text up to the last token lane 0 emitted
    // the wave's
    uint32_t produced = 0, loaded = 0;  // text stored; input bytes [.., loaded) are or were in the ring
    uint32_t clean = 0;                 // text below this was stored before the last fence

    while (err == INF_OK) {
        // ---- ring: the bytes [pos, pos + INF_RING) below n
        const uint32_t pos = (uint32_t)__shfl((int)b.pos, 0, 64);
        if (loaded < pos) loaded = pos;
        const uint32_t upto = n - pos < INF_RING ? n : pos + INF_RING;  // (pos <= n + 8; n - pos wraps to a large number behind n)
        const uint32_t end = pos > n ? loaded : upto;
        for (uint32_t i = loaded + lane; i < end; i += 64u) {
            const uint32_t at = i & (INF_RING - 1u);
            const uint8_t v = src[i];
            w->ring[at] = v;
            if (at < 8u) w->ring[INF_RING + at] = v;
        }
        if (end > loaded) loaded = end;
        inf_wave_sync();

        // ---- decode: lane 0
        uint32_t ev = INF_EV_BATCH, ev_a = 0, ev_b = 0, ntok = 0;
        if (lane == 0u) {
            const uint32_t start = b.pos;
            while (ntok < INF_BATCH && b.pos - start <= INF_RUN) {
                fill(&b);
                if (inf_overrun(&b)) { ev = INF_EV_ERROR; ev_a = INF_E_INPUT; break; }  // (every trip below takes at least a bit)
                if (in_block) {
                    uint32_t a = 0, d = 0;
                    const int k = inf_token(&b, &w->t, &a, &d);
                    if (k < 0) { ev = INF_EV_ERROR; ev_a = (uint32_t)-k; break; }
                    if (k == 2) { in_block = false; continue; }
                    if (k == 0) {
                        if (emitted >= isize) { ev = INF_EV_ERROR; ev_a = INF_E_OUTPUT; break; }
                        w->tok[ntok++ & (INF_BATCH - 1u)] = a & 255u;
                        emitted++;
                        continue;
                    }
                    if (d > emitted) { ev = INF_EV_ERROR; ev_a = INF_E_DISTANCE; break; }
                    if (a > isize - emitted) { ev = INF_EV_ERROR; ev_a = INF_E_OUTPUT; break; }
                    w->tok[ntok++ & (INF_BATCH - 1u)] = 0x80000000u | ((d - 1u) << 9) | a;
                    emitted += a;
                    continue;
                }
                if (last) {  // behind the final block
                    ev = INF_EV_DONE;
                    if ((inf_used_bits(&b) + 7u) / 8u != n) { ev = INF_EV_ERROR; ev_a = INF_E_UNUSED; }
                    else if (emitted != isize) { ev = INF_EV_ERROR; ev_a = INF_E_LENGTH; }
                    break;
                }
                last = inf_take(&b, 1u) != 0u;
                const uint32_t type = inf_take(&b, 2u);
                if (inf_overrun(&b)) { ev = INF_EV_ERROR; ev_a = INF_E_INPUT; break; }
                if (type == 3u) { ev = INF_EV_ERROR; ev_a = INF_E_BTYPE; break; }
                if (type == 0u) {
                    inf_drop(&b, b.cnt & 7u);
                    fill(&b);
                    const uint32_t len = inf_take(&b, 16u), nlen = inf_take(&b, 16u);
                    ev = INF_EV_ERROR;
                    if (inf_overrun(&b)) { ev_a = INF_E_INPUT; break; }
                    if (len != (nlen ^ 0xffffu)) { ev_a = INF_E_STORED; break; }
                    const uint32_t at = (uint32_t)(inf_used_bits(&b) >> 3);  // (<= n: no overrun)
                    if (len > n - at) { ev_a = INF_E_INPUT; break; }
                    if (len > isize - emitted) { ev_a = INF_E_OUTPUT; break; }
                    ev = INF_EV_STORED; ev_a = at; ev_b = len;
                    emitted += len;
                    b.buf = 0; b.cnt = 0; b.pos = at + len;
                    break;
                }
                in_block = true;
                if (type == 1u) { ev = INF_EV_FIXED; break; }
                uint32_t nl = 0, nd = 0;
                const int e = inf_read_lengths(&b, fill, &w->t, &nl, &nd);
                if (e) { ev = INF_EV_ERROR; ev_a = (uint32_t)e; break; }
                ev = INF_EV_DYNAMIC; ev_a = nl; ev_b = nd;
                break;
            }
        }
        inf_wave_sync();
        ev = (uint32_t)__shfl((int)ev, 0, 64);
        ev_a = (uint32_t)__shfl((int)ev_a, 0, 64);
        ev_b = (uint32_t)__shfl((int)ev_b, 0, 64);
        ntok = (uint32_t)__shfl((int)ntok, 0, 64);
        if (ev == INF_EV_ERROR) { err = (int)ev_a; break; }

        // ---- expand the tokens
        if (ntok) {
            const uint32_t tk = lane < ntok ? w->tok[lane] : 0u;
            const bool is_match = (tk >> 31) != 0u;
            const uint32_t ln = lane < ntok ? (is_match ? (tk & 511u) : 1u) : 0u;
            uint32_t inc = ln;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t o = (uint32_t)__shfl_up((int)inc, off, 64);
                if (lane >= (uint32_t)off) inc += o;
            }
            const uint32_t at = produced + inc - ln, total = (uint32_t)__shfl((int)inc, 63, 64);
            if (lane < ntok && !is_match && at < isize) out[at] = (uint8_t)tk;
            uint64_t mm = __ballot(is_match);
            while (mm) {
                const int k = __ffsll((unsigned long long)mm) - 1;
                mm &= mm - 1ull;
                const uint32_t t = (uint32_t)__shfl((int)tk, k, 64), len = t & 511u, d = ((t >> 9) & 32767u) + 1u;
                const uint32_t dst = (uint32_t)__shfl((int)at, k, 64);
                if (d > dst || dst > isize || len > isize - dst) continue;  // (lane 0 has checked both: never taken)
                if (dst - d + (len < d ? len : d) > clean) {
                    // The source bytes may have been stored a moment ago by OTHER lanes of this wave (the literals above, the match
                    // before).  What makes the loads see them is the hardware's order: one wave's vector memory instructions go
                    // through this CU's L1 in the order they were issued (the model LLVM compiles for when a workgroup's waves
                    // share a CU), the L1 is write-through and the loads read it, and no other wave touches the member's text.  On
                    // gfx950 this fence therefore emits no instruction; what it does is keep the COMPILER from moving the loads
                    // above the stores or from keeping text in registers across them.
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
                    clean = dst;  // (everything below dst: earlier tokens of this round, the rounds before)
                }
                const uint8_t *from = out + (dst - d);
                for (uint32_t j = lane; j < len; j += 64u) out[dst + j] = from[j % d];
            }
            produced += total;
        }

        // ---- the event
        if (ev == INF_EV_DONE) break;
        if (ev == INF_EV_STORED) {  // ev_a: where its bytes start in the body, ev_b: how many (checked by lane 0 against n and isize)
            if (ev_a <= n && ev_b <= n - ev_a && produced <= isize && ev_b <= isize - produced)
                for (uint32_t j = lane; j < ev_b; j += 64u) out[produced + j] = src[ev_a + j];
            produced += ev_b;
        } else if (ev == INF_EV_FIXED || ev == INF_EV_DYNAMIC) {
            uint32_t nlen = INF_NLEN, ndist = INF_NDIST;
            if (ev == INF_EV_FIXED) {
                for (uint32_t s = lane; s < INF_NLEN + INF_NDIST; s += 64u) w->t.lens[s] = inf_fixed_length(s);
            } else {  // the distance lengths follow the literal/length ones at once: to their own place, zeros behind both
                nlen = ev_a <= 286u ? ev_a : 286u;
                ndist = ev_b <= 30u ? ev_b : 30u;
                const uint8_t dl = lane < ndist ? w->t.lens[nlen + lane] : (uint8_t)0;
                inf_wave_sync();
                for (uint32_t s = nlen + lane; s < INF_NLEN; s += 64u) w->t.lens[s] = 0;
                if (lane < INF_NDIST) w->t.lens[INF_NLEN + lane] = dl;
            }
            inf_wave_sync();
            err = inf_build_wave(&w->t, nlen, ndist, lane);
        }
    }

    // ---- crc: spans of S bytes (a multiple of 32) aligned to the end, lane t the span that ends S t bytes before it
    if (err == INF_OK) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // (the text is read back by other lanes than stored it: as for the matches above)
        const uint32_t S = ((isize + 63u) / 64u + BGZF_CRC_CHUNK - 1u) / BGZF_CRC_CHUNK * BGZF_CRC_CHUNK;
        uint32_t X = 0;
        if (lane * S < isize) {
            const uint32_t hi = isize - lane * S, lo = hi >= S ? hi - S : 0u;
            uint32_t state = 0;
            for (uint32_t p = lo; p < hi; p++) state = bgzf_crc_byte(crc_lds, state, out[p]);
            X = bgzf_crc_mul(state, crc_tab->xp32[(lane * S / BGZF_CRC_CHUNK) < INF_CRC_CHUNKS ? lane * S / BGZF_CRC_CHUNK : 0u]);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) X ^= (uint32_t)__shfl_xor((int)X, off, 64);
        if (bgzf_crc_finish(crc_tab->xp32, crc_tab->xp1, X, isize) != m.crc) err = INF_E_CRC;
    }
    if (err != INF_OK && lane == 0u) atomicMin(status, (unsigned long long)((first_index + index) << 8) | (unsigned long long)err);
}

// ---- host side --------------------------------------------------------------------------------------------------------------
InfScratch::~InfScratch()
{
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
    if (h_status) (void)hipHostFree(h_status);
}

uint64_t inf_chunk_members()
{
    const char *e = getenv("CELLECTOR_INFLATE_CHUNK");  // (tests: several launches on a small stream)
    const uint64_t v = e ? strtoull(e, nullptr, 10) : 0;
    return v >= 1 && v <= INF_CHUNK_MEMBERS ? v : INF_CHUNK_MEMBERS;
}

cellector_status inf_scratch(cellector_ctx *c, InfScratch *s, uint64_t cap_members)
{
    s->cap_members = cap_members;
    CHK(dev_alloc(c, &s->tables, sizeof(InfCrcTables)));
    CHK(dev_alloc(c, &s->members, cap_members));
    CHK(dev_alloc(c, &s->status, 1));
    HIPCHK(c, hipHostMalloc((void **)&s->h_status, sizeof(unsigned long long), hipHostMallocDefault));
    *s->h_status = ~0ull;
    HIPCHK(c, hipMemsetAsync(s->status, 0xff, sizeof(unsigned long long), c->stream));  // (in place when this returns: synchronised below)
    InfCrcTables *t = new InfCrcTables;
    inf_crc_tables_build(t);
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

// The members blocks[k0..k1) of the stream whose bytes [in_first, in_first + n_in) are at dev_in, inflated to dev_out + (their
// out offset - out_first), all on `st`; the status word is copied to s->h_status behind the kernel (read it after synchronising
// st: ~0 = all accepted, else member << 8 | kind, the smallest since the word was last reset; reset: before this launch).
// `host` is where the member table is put together (cap_members entries; it must stay as it is until st has passed the launch).
cellector_status inf_launch(cellector_ctx *c, InfScratch *s, hipStream_t st, const std::vector<BgzfBlock> &blocks, uint64_t k0, uint64_t k1,
                            InfMember *host, const uint8_t *file, const uint8_t *dev_in, uint64_t in_first, uint64_t n_in, uint8_t *dev_out,
                            uint64_t out_first, uint64_t out_cap, bool reset)
{
    const uint64_t nm = k1 - k0;
    if (nm == 0) return CELLECTOR_OK;
    if (nm > s->cap_members) return ctx_fail(c, CELLECTOR_EINVAL, "inflate: %llu members for a scratch of %llu", (unsigned long long)nm, (unsigned long long)s->cap_members);
    for (uint64_t k = k0; k < k1; k++) {
        const BgzfBlock &b = blocks[k];
        const uint8_t *tr = file + b.off + b.clen - 8;
        InfMember &m = host[k - k0];
        m.in_off = b.off + 12 + b.xlen - in_first;
        m.in_len = (uint32_t)(b.clen - 12 - b.xlen - 8);
        m.isize = b.isize;
        m.out_off = b.out - out_first;
        m.crc = tr[0] | ((uint32_t)tr[1] << 8) | ((uint32_t)tr[2] << 16) | ((uint32_t)tr[3] << 24);
        m.pad = 0;
    }
    HIPCHK(c, hipMemcpyAsync(s->members, host, nm * sizeof(InfMember), hipMemcpyHostToDevice, st));
    if (reset) HIPCHK(c, hipMemsetAsync(s->status, 0xff, sizeof(unsigned long long), st));
    if (s->timed) HIPCHK(c, hipEventRecord(s->ev[0], st));
    hipLaunchKernelGGL(k_bgzf_inflate, dim3((unsigned)((nm + INF_WAVES - 1) / INF_WAVES)), dim3(INF_THREADS), 0, st, dev_in, n_in,
                       (const InfMember *)s->members.get(), (uint32_t)nm, dev_out, out_cap, (const InfCrcTables *)(const void *)s->tables.get(),
                       (uint64_t)k0, s->status.get());
    HIPCHK(c, hipGetLastError());
    if (s->timed) HIPCHK(c, hipEventRecord(s->ev[1], st));
    HIPCHK(c, hipMemcpyAsync(s->h_status, s->status, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    s->n_members += nm;
    s->bytes_in += n_in;
    s->bytes_out += out_cap;
    return CELLECTOR_OK;
}
// after the stream was synchronised: the launch's kernel time joins the sum
void inf_launch_timed(InfScratch *s)
{
    float ms = 0;
    if (s->timed && hipEventElapsedTime(&ms, s->ev[0], s->ev[1]) == hipSuccess) s->ms_kernel += ms;
}

static const char *inf_kind(unsigned k)
{
    static const char *const names[] = {"",
                                        "block type 3",
                                        "stored LEN is not ~NLEN",
                                        "too many length or distance symbols",
                                        "an over-subscribed or incomplete set of code lengths",
                                        "a repeat with no length before it or beyond the lengths",
                                        "bits that are no code",
                                        "a distance before the member's first byte",
                                        "output beyond ISIZE",
                                        "the body ends inside a symbol",
                                        "unused bytes behind the final block",
                                        "fewer bytes than ISIZE",
                                        "the CRC-32 is not the trailer's"};
    return k < sizeof names / sizeof *names ? names[k] : "?";
}
cellector_status inf_refused(const cellector_ctx *c, const char *what, unsigned long long status)
{
    return ctx_fail(c, CELLECTOR_EIO, "%s: member %llu is refused: %s", what, status >> 8, inf_kind((unsigned)(status & 0xffu)));
}

// cellector_bgzf_decompress behind its checks: the stream through the device in chunks of inf_chunk_members() members
cellector_status bgzf_decompress_host(cellector_ctx *c, const uint8_t *in, uint64_t n, uint8_t *out, uint64_t capacity, uint64_t *n_out,
                                      uint64_t *n_blocks)
{
    std::vector<BgzfBlock> blocks;
    size_t total = 0;
    try {
        if (n == 0 || !bgzf_index(in, (size_t)n, &blocks, &total))
            return ctx_fail(c, CELLECTOR_EPARSE, "bgzf_decompress: the %llu bytes are no BGZF stream (gzip members with a 'BC' size field, whole, at most 64 KB of text each)",
                            (unsigned long long)n);
    } catch (const std::exception &) {
        return ctx_fail(c, CELLECTOR_ENOMEM, "bgzf_decompress: out of host memory for the index");
    }
    *n_out = total;
    *n_blocks = blocks.size();
    if (!out) return CELLECTOR_OK;
    if (capacity < total)
        return ctx_fail(c, CELLECTOR_EINVAL, "bgzf_decompress: capacity %llu is below the %llu bytes of the text", (unsigned long long)capacity,
                        (unsigned long long)total);
    const uint64_t chunk = inf_chunk_members(), nb = blocks.size();
    uint64_t max_in = 0, max_out = 0;
    for (uint64_t k0 = 0; k0 < nb; k0 += chunk) {
        const uint64_t k1 = k0 + chunk < nb ? k0 + chunk : nb;
        max_in = std::max<uint64_t>(max_in, blocks[k1 - 1].off + blocks[k1 - 1].clen - blocks[k0].off);
        max_out = std::max<uint64_t>(max_out, blocks[k1 - 1].out + blocks[k1 - 1].isize - blocks[k0].out);
    }
    InfScratch s;
    DevBuf<uint8_t> d_in, d_out;
    CHK(inf_scratch(c, &s, chunk < nb ? chunk : nb));
    CHK(dev_alloc(c, &d_in, max_in));
    CHK(dev_alloc(c, &d_out, max_out));
    std::vector<InfMember> table(s.cap_members);
    for (uint64_t k0 = 0; k0 < nb; k0 += chunk) {
        const uint64_t k1 = k0 + chunk < nb ? k0 + chunk : nb;
        const uint64_t in_first = blocks[k0].off, n_in = blocks[k1 - 1].off + blocks[k1 - 1].clen - in_first;
        const uint64_t out_first = blocks[k0].out, n_text = blocks[k1 - 1].out + blocks[k1 - 1].isize - out_first;
        HIPCHK(c, hipMemcpyAsync(d_in, in + in_first, n_in, hipMemcpyHostToDevice, c->stream));
        CHK(inf_launch(c, &s, c->stream, blocks, k0, k1, table.data(), in, d_in, in_first, n_in, d_out, out_first, n_text, true));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        inf_launch_timed(&s);
        if (*s.h_status != ~0ull) return inf_refused(c, "bgzf_decompress", *s.h_status);
        CHK(d2h(c, out + out_first, d_out, n_text));
    }
    if (s.timed)
        fprintf(stderr, "[cellector] bgzf_decompress: %llu members, %llu -> %llu bytes, inflate kernel %.3f ms\n", (unsigned long long)nb,
                (unsigned long long)n, (unsigned long long)total, s.ms_kernel);
    return CELLECTOR_OK;
}
