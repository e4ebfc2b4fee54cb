// Engine v2, the once-per-ingest half: tiled_build turns the by-cell CSR / by-locus CSC into everything CtxTiled holds (ctx.h): the
// SELL-64-1024 tiles, the overflow CSR / CSC and their static lists, the compact CSC and the per-iteration workspaces.  The kernels
// an iteration runs are in kernels_tiled.hip.
#include "tiled.h"

// ---------------------------------------------------------------------------------------------------------
// build: tiles + overflow CSR from the by-cell CSR; compact CSC + overflow CSC + per-locus code histogram
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t row_lower_bound(const uint64_t *__restrict__ ent, uint64_t lo, uint64_t hi, uint32_t locus)
{
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (ENT_IDX(ent[mid]) < locus) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// One 1024-thread block per tile, thread = cell of the block.  The cells are ordered by their number of regular entries
// in this chunk (stable counting sort: deterministic layout), every 64 of them form a slice of 64 cell ids and 64 rows of K
// entries, K = the slice's longest cell (at least 1), in the format of K's parity (tiled.h).  FILL = false: tile size; FILL =
// true: write slices + header.
// which entries a tile set takes, and their 16-bit form inside chunk j
template <class G>
__device__ __forceinline__ bool geo_take(uint64_t e)
{
    const uint32_t n = ENT_ALT(e) + ENT_REF(e);
    return n - G::NLO <= G::NHI - G::NLO;
}
template <class G>
__device__ __forceinline__ uint16_t geo_encode(uint64_t e, uint32_t j)
{
    const uint32_t r = ENT_REF(e), n = ENT_ALT(e) + r;
    const uint32_t code = G::NLO == 1 ? ent_code(e) : t2_code(n, r);
    return tile_entry<G>(ENT_IDX(e) - j * G::BLU, code);
}
template <bool FILL, class G = geo_reg>
__global__ __launch_bounds__(T_BC) void k_tile_build(uint64_t nloc, uint32_t nj, uint64_t tile0,
                                                     const uint64_t *__restrict__ csr_ptr,
                                                     const uint64_t *__restrict__ csr_ent,
                                                     uint64_t *__restrict__ tile_elems /*count pass: out; fill: tile_ptr*/,
                                                     uint16_t *__restrict__ tiles, uint16_t *__restrict__ thdr,
                                                     const uint32_t *__restrict__ toff /*[row][nj + 1] or null*/)
{
    __shared__ uint32_t s_cnt[T_BC / 64][TB_BINS];  // cells per (source wave, bin)
    __shared__ uint32_t s_base[TB_BINS];            // first rank of a bin
    __shared__ uint32_t s_kmax[T_BC / 64];          // longest cell of a slice
    __shared__ uint32_t s_sbase[T_BC / 64 + 1];     // first entry of a slice inside the tile
    const uint64_t t = tile0 + blockIdx.x;
    const uint32_t b = (uint32_t)(t / nj), j = (uint32_t)(t % nj);
    const uint32_t cl = threadIdx.x, lane = cl & 63, wv = cl >> 6;
    const uint64_t row = (uint64_t)b * T_BC + cl;
    for (uint32_t i = cl; i < (T_BC / 64) * TB_BINS; i += T_BC) (&s_cnt[0][0])[i] = 0;
    if (cl < T_BC / 64) s_kmax[cl] = 0;
    uint64_t lo = 0, hi = 0;
    uint32_t len = 0;
    if (row < nloc) {
        const uint64_t beg = csr_ptr[row], end = csr_ptr[row + 1];
        if (toff) {  // where the row's entries of every chunk start (k_range_offsets): two reads instead of two searches
            lo = beg + toff[row * (nj + 1) + j];
            hi = beg + toff[row * (nj + 1) + j + 1];
        } else {
            lo = row_lower_bound(csr_ent, beg, end, j * G::BLU);
            hi = row_lower_bound(csr_ent, lo, end, (j + 1u) * G::BLU);
        }
        for (uint64_t i = lo; i < hi; i++) len += geo_take<G>(csr_ent[i]) ? 1u : 0u;
    }
    __syncthreads();
    // stable counting sort by bin = min(len, TB_BINS-1): rank inside (wave, bin) from ballots
    const uint32_t bin = min(len, (uint32_t)TB_BINS - 1u);
    uint32_t within = 0;
    {
        unsigned long long todo = ~0ull;  // lanes whose bin has not been handled yet
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            const uint32_t v = (uint32_t)__shfl((int)bin, src, 64);
            const unsigned long long m = __ballot(bin == v);
            if (bin == v) within = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if ((int)lane == src) s_cnt[wv][v] = (uint32_t)__popcll(m);
            todo &= ~m;
        }
    }
    __syncthreads();
    if (cl < TB_BINS) {  // exclusive prefix over bins of the bin totals
        uint32_t tot = 0;
        for (int w = 0; w < T_BC / 64; w++) tot += s_cnt[w][cl];
        uint32_t inc = tot;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t o = __shfl_up(inc, off, 64);
            if ((int)cl >= off) inc += o;
        }
        s_base[cl] = inc - tot;
    }
    __syncthreads();
    uint32_t rank = s_base[bin] + within;
    for (uint32_t w = 0; w < wv; w++) rank += s_cnt[w][bin];
    const uint32_t dw = rank >> 6, dl = rank & 63;  // destination slice and lane
    atomicMax(&s_kmax[dw], len);
    __syncthreads();
    if (cl == 0) {
        uint32_t acc = 0;
        for (int w = 0; w < T_BC / 64; w++) {
            s_sbase[w] = acc;
            acc += 64u * (slice_k(s_kmax[w]) + 1u);
        }
        s_sbase[T_BC / 64] = acc;
    }
    __syncthreads();
    if (!FILL) {
        if (cl == 0) tile_elems[t] = (uint64_t)s_sbase[T_BC / 64];  // a multiple of 64 u16
        return;
    }
    const uint64_t tbase = tile_elems[t];
    uint16_t *hp = thdr + t * T_HDR;
    if (cl < T_BC / 64) {
        uint32_t *hd = reinterpret_cast<uint32_t *>(hp) + 4 * cl;
        const uint64_t first = tbase + s_sbase[cl];
        hd[0] = (uint32_t)first;
        hd[1] = (uint32_t)(first >> 32);
        hd[2] = slice_k(s_kmax[cl]);  // K: padded entries per cell of the slice
        hd[3] = s_kmax[cl] == 0u;  // no row of the slice has an entry (the nearly empty tier-2 tiles of a deep matrix: most slices)
    }
    const uint32_t K = slice_k(s_kmax[dw]);
    uint16_t *sl = tiles + tbase + s_sbase[dw], *dst = sl + slice_row_at(K, dl);  // this cell's slice and its row's entries
    sl[slice_cell_at(K, dl)] = (uint16_t)cl;
    uint32_t k = 0;
    for (uint64_t i = lo; i < hi; i++) {
        const uint64_t e = csr_ent[i];
        if (geo_take<G>(e)) dst[k++] = geo_encode<G>(e, j);
    }
    for (; k < K; k++) dst[k] = tile_entry_null<G>();  // padding: the chunk's all-zero slot
}

// Bank-aware order of the entries inside the rows of one slice (option "bank_order"; a wave per slice, lane = row, the slice's rows
// in LDS).  The tile kernel's lookup step k reads, for the 32 lanes of a half-wave, the log-pmf and the expected term of the lane's
// entry (tab_pmf / tab_exp of the geometry, tiled.h): two 8-byte LDS reads per lane, served at one cycle per DISTINCT address on the
// busiest of the 32 bank pairs.  In file order the banks are random — 3.3 cycles per step and half-wave instead of 1 — and those conflicts
// are 42 % of the kernel's time (SQ_LDS_BANK_CONFLICT).  A row's sum does not care about the order of its entries beyond rounding,
// so the builder picks it: step by step, every lane whose entry of this step is still open proposes the cheapest of its remaining
// entries given the bank loads of the lanes already placed in the step; of the proposers that share a bank pair the lowest lane is
// placed, the others propose again; after four rounds whoever is left takes its proposal.  Simulated (tools/probe/bank_sim.py):
// 3.3 -> 2.4 cycles per step, the same as placing the lanes one after the other (locus-major, 18 doubles per locus; with the
// code-major image 3.06 -> 2.17).  Deterministic; the order inside a row then depends
// on the 31 rows that share its half-wave, i.e. on the shard's cell set: per-cell sums of differently sharded runs differ in the
// last bits (as they already do between different chunk-group counts).
#define TBO_ROUNDS 4
__device__ __forceinline__ void tbo_banks(uint32_t e, uint32_t *a, uint32_t *b)
{
    // (the tile kernel's own address function; code-major: both are the slot's bank pair, slot mod 32)
    *a = tile_entry_pmf<geo_reg>(e) & 31u;
    *b = tile_entry_exp<geo_reg>(e) & 31u;
}
// Which lane of its slice a row takes (any permutation of a slice's 64 rows is a valid layout).  The tile kernel adds a row's
// sums to its cell's accumulator in LDS with one 16-byte read and one 16-byte write per lane: address = cell * 16, served in
// groups of 16 lanes (read: {0-3,12-15,20-27}, {4-11,16-19,28-31}, and the same + 32) resp. 8 contiguous lanes (write), one cycle
// per distinct address on a bank quad = cell mod 16.  Rows in count order carry arbitrary cells — 2.7 addresses on the busiest
// quad of a read group.  Here the slice's rows are ranked by (cell mod 16, lane) and dealt round-robin to the four read groups,
// the second and fourth group shifted by half a group so that two rows of one class never share a write group either: classes of
// up to four rows (the average) become conflict-free.  Returns the row count that now belongs to this lane.
__device__ uint32_t tile_lane_assign(uint16_t *slice /*64 x (Kw + 1) u16, either format*/, uint32_t Kw, uint32_t lane, uint32_t cnt, uint32_t *scr)
{
#define TLA_SYNC() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
    const uint32_t cls = (uint32_t)slice[slice_cell_at(Kw, lane)] & 15u;
    const unsigned long long lt = (1ull << lane) - 1ull;
    uint32_t t = 0;
#pragma unroll
    for (uint32_t c = 0; c < 16u; c++) {
        const unsigned long long m = __ballot(cls == c);
        if (c < cls) t += (uint32_t)__popcll(m);
        else if (c == cls) t += (uint32_t)__popcll(m & lt);
    }
    const uint32_t g = t & 3u, pp = ((t >> 2) + ((g & 1u) ? 8u : 0u)) & 15u;
    // lane number pp of read group g & 1 (G0 = 0-3, 12-15, 20-27; G1 = 4-11, 16-19, 28-31), upper half for g >= 2
    const uint32_t l0 = pp < 4u ? pp : (pp < 8u ? pp + 8u : pp + 12u);          // G0: 0..3 | 12..15 | 20..27
    const uint32_t l1 = pp < 8u ? pp + 4u : (pp < 12u ? pp + 8u : pp + 16u);    // G1: 4..11 | 16..19 | 28..31
    const uint32_t dst = ((g & 1u) ? l1 : l0) + ((g & 2u) ? 32u : 0u);
    scr[dst] = lane;
    scr[64 + dst] = cnt;
    TLA_SYNC();
    const uint32_t src = scr[lane], cnt_new = scr[64 + lane];
    for (uint32_t k = 0; k <= Kw; k++) {  // column by column (the cell ids, then entry k - 1): all of a column's reads before its writes
        const uint16_t v = slice[k ? slice_row_at(Kw, src) + k - 1u : slice_cell_at(Kw, src)];
        TLA_SYNC();
        slice[k ? slice_row_at(Kw, lane) + k - 1u : slice_cell_at(Kw, lane)] = v;
        TLA_SYNC();
    }
    return cnt_new;
#undef TLA_SYNC
}

#define TBO_WIN 4  // candidates per lane and round: its next four remaining entries (the whole rest is no better: 2.46 vs 2.50 cycles)
__device__ void tile_bank_order(uint16_t *row /*this lane's K entries*/, uint32_t K, uint32_t cnt /*real entries: the first cnt*/,
                                uint32_t lane, uint32_t *scr /*[256]: this wave's bank loads and claims*/)
{
    const uint32_t h = lane >> 5;
    uint32_t *ld_a = scr + h * 64, *ld_b = ld_a + 32, *win_a = scr + 128 + h * 64, *win_b = win_a + 32;
    // (one wave: its LDS operations complete in program order; the asm statements only keep the compiler from moving them)
#define TBO_SYNC() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
    if (K <= 1u) return;  // (wave-uniform) nothing to choose
    for (uint32_t k = 0; k + 1u < K; k++) {
        if (__ballot(k + 1u < cnt) == 0ull) break;  // no lane has two entries left to choose from
        scr[lane] = 0u; scr[64 + lane] = 0u;  // the step's loads
        // this lane's candidates: its next TBO_WIN remaining entries, and their bank pairs
        uint32_t e[TBO_WIN], ca[TBO_WIN], cb[TBO_WIN];
#pragma unroll
        for (uint32_t u = 0; u < (uint32_t)TBO_WIN; u++) {
            e[u] = k + u < cnt ? (uint32_t)row[k + u] : 0xffffffffu;
            tbo_banks(e[u], &ca[u], &cb[u]);
        }
        bool open = k < cnt;  // (a row out of real entries keeps its padding entry: one shared address)
        TBO_SYNC();
        for (uint32_t rd = 0; rd < (uint32_t)TBO_ROUNDS; rd++) {
            if (__ballot(open) == 0ull) break;
            scr[128 + lane] = ~0u; scr[192 + lane] = ~0u;  // the round's claims
            uint32_t cost[TBO_WIN];
#pragma unroll
            for (uint32_t u = 0; u < (uint32_t)TBO_WIN; u++) cost[u] = ld_a[ca[u]] + ld_b[cb[u]];
            uint32_t best = 0, bc = cost[0];
#pragma unroll
            for (uint32_t u = 1; u < (uint32_t)TBO_WIN; u++)
                if (e[u] != 0xffffffffu && cost[u] < bc) { bc = cost[u]; best = u; }
            uint32_t ba = ca[0], bb = cb[0];
#pragma unroll
            for (uint32_t u = 1; u < (uint32_t)TBO_WIN; u++)
                if (best == u) { ba = ca[u]; bb = cb[u]; }
            TBO_SYNC();
            if (open) {
                atomicMin(&win_a[ba], lane);
                atomicMin(&win_b[bb], lane);
            }
            TBO_SYNC();
            if (open && (rd == (uint32_t)TBO_ROUNDS - 1u || (win_a[ba] == lane && win_b[bb] == lane))) {
                if (best) {  // swap the chosen entry into position k
                    uint32_t eb = e[0];
#pragma unroll
                    for (uint32_t u = 1; u < (uint32_t)TBO_WIN; u++)
                        if (best == u) eb = e[u];
                    row[k] = (uint16_t)eb;
                    row[k + best] = (uint16_t)e[0];
                }
                atomicAdd(&ld_a[ba], 1u);
                atomicAdd(&ld_b[bb], 1u);
                open = false;
            }
            TBO_SYNC();
        }
    }
#undef TBO_SYNC
}

// The same tiles, built the way the memory system likes (used whenever the per-(cell, chunk) offsets table exists):
//   * a PERSISTENT workgroup takes whole cell blocks and walks a block's tiles chunk by chunk: a thread's reads of its row move
//     forward through one cache line after the other (a grid of one workgroup per tile spread the chunks of a block over the
//     XCDs, and every tile fetched its 1024 row segments afresh: 2.5x the bytes);
//   * it reads the 2-byte compact by-cell entries (c4r: locus mod 4096 | code << 12, code 15 = not a table entry) instead of the
//     8-byte packed ones — the chunk is narrower than 4096 loci, so the slot inside it follows from the low 12 bits;
//   * the slices are assembled in LDS and leave as whole 16-byte stores (rows written two bytes at a time straight to global
//     memory cost 65x their bytes in partial-line traffic: 0.35 TB for 5.3 GB of tiles at 10^6 cells x 200k loci).
// Same layout, bit for bit, as k_tile_build.
template <bool FILL, bool ORDER = false>
__global__ __launch_bounds__(T_BC, 8) void k_tile_build2(uint64_t nloc, uint32_t nb, uint32_t nj, const uint64_t *__restrict__ csr_ptr,
                                                      const uint16_t *__restrict__ c4r, const uint32_t *__restrict__ toff /*[row][nj + 1]*/,
                                                      uint64_t *__restrict__ tile_elems /*count pass: out; fill: tile_ptr*/,
                                                      uint16_t *__restrict__ tiles, uint16_t *__restrict__ thdr)
{
    static_assert(T_BLU < LR_LOCI, "a chunk's loci are told apart by their low 12 bits");
    __shared__ uint32_t s_cnt[T_BC / 64][TB_BINS];
    __shared__ uint32_t s_base[TB_BINS];
    __shared__ uint32_t s_kmax[T_BC / 64];
    __shared__ uint32_t s_sbase[T_BC / 64 + 1];
    __shared__ __attribute__((aligned(16))) uint16_t s_tile[FILL ? TB_STAGE : 8];
    __shared__ uint32_t s_scr[ORDER ? (T_BC / 64) * 256 : 1];  // bank-aware order: a wave's loads and claims
    __shared__ uint16_t s_rcnt[ORDER ? T_BC : 1];              // ... real entries of every row of the tile, by (slice, lane)
    const uint32_t cl = threadIdx.x, lane = cl & 63, wv = cl >> 6;
    for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
        const uint64_t row = (uint64_t)b * T_BC + cl;
        const bool have = row < nloc;
        const uint64_t beg = have ? csr_ptr[row] : 0;
        const uint32_t *orow = toff + (have ? row : 0) * ((uint64_t)nj + 1);
        uint32_t o_lo = have ? orow[0] : 0u, o_hi = have ? orow[1] : 0u;
        for (uint32_t j = 0; j < nj; j++) {
            const uint64_t t = (uint64_t)b * nj + j;
            for (uint32_t i = cl; i < (T_BC / 64) * TB_BINS; i += T_BC) (&s_cnt[0][0])[i] = 0;
            if (cl < T_BC / 64) s_kmax[cl] = 0;
            const uint32_t o_next = have ? orow[min(j + 2u, nj)] : 0u;  // (the next chunk's end, requested a step ahead)
            const uint64_t lo = beg + o_lo, hi = beg + o_hi;
            // the segment's first TB_SEG entries with independent loads (one memory latency instead of one per entry); longer
            // segments finish in loops
            constexpr uint32_t TB_SEG = 16;
            uint32_t seg[TB_SEG];
            if (FILL) {
#pragma unroll
                for (uint32_t u = 0; u < TB_SEG; u++) seg[u] = lo + u < hi ? (uint32_t)c4r[lo + u] : 0xffffu;  // (all ones: code 15)
            }
            // The sort key and the row length are the segment's length INCLUDING its few overflow entries (0.8 %): the size pass then
            // reads the offsets table only, and a row that holds one gets a padding entry in its place — sums unchanged to the bit
            // (a row's entries stay in locus order, a padding entry adds an exact zero), 0.3 % more tile bytes.
            const uint32_t len = o_hi - o_lo;
            __syncthreads();
            // stable counting sort by bin = min(len, TB_BINS-1): rank inside (wave, bin) from ballots
            const uint32_t bin = min(len, (uint32_t)TB_BINS - 1u);
            uint32_t within = 0;
            {
                unsigned long long todo = ~0ull;
                while (todo) {
                    const int src = __ffsll((long long)todo) - 1;
                    const uint32_t v = (uint32_t)__shfl((int)bin, src, 64);
                    const unsigned long long m = __ballot(bin == v);
                    if (bin == v) within = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                    if ((int)lane == src) s_cnt[wv][v] = (uint32_t)__popcll(m);
                    todo &= ~m;
                }
            }
            __syncthreads();
            if (cl < TB_BINS) {
                uint32_t tot = 0;
                for (int w = 0; w < T_BC / 64; w++) tot += s_cnt[w][cl];
                uint32_t inc = tot;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const uint32_t o = __shfl_up(inc, off, 64);
                    if ((int)cl >= off) inc += o;
                }
                s_base[cl] = inc - tot;
            }
            __syncthreads();
            uint32_t rank = s_base[bin] + within;
            for (uint32_t w = 0; w < wv; w++) rank += s_cnt[w][bin];
            const uint32_t dw = rank >> 6, dl = rank & 63;
            atomicMax(&s_kmax[dw], len);
            __syncthreads();
            if (cl == 0) {
                uint32_t acc = 0;
                for (int w = 0; w < T_BC / 64; w++) {
                    s_sbase[w] = acc;
                    acc += 64u * (slice_k(s_kmax[w]) + 1u);
                }
                s_sbase[T_BC / 64] = acc;
            }
            __syncthreads();
            const uint32_t total = s_sbase[T_BC / 64];  // a multiple of 64 u16
            if (!FILL) {
                if (cl == 0) tile_elems[t] = (uint64_t)total;
            } else {
                const uint64_t tbase = tile_elems[t];
                if (cl < T_BC / 64) {
                    uint32_t *hd = reinterpret_cast<uint32_t *>(thdr + t * T_HDR) + 4 * cl;
                    const uint64_t first = tbase + s_sbase[cl];
                    hd[0] = (uint32_t)first;
                    hd[1] = (uint32_t)(first >> 32);
                    hd[2] = slice_k(s_kmax[cl]);
                    hd[3] = s_kmax[cl] == 0u;
                }
                const uint32_t K = slice_k(s_kmax[dw]);
                const bool staged = total <= (uint32_t)TB_STAGE;  // (uniform)
                uint16_t *sl = (staged ? s_tile : tiles + tbase) + s_sbase[dw], *dst = sl + slice_row_at(K, dl);
                sl[slice_cell_at(K, dl)] = (uint16_t)cl;
                uint32_t k = 0;
                const uint32_t cbase = (j * (uint32_t)T_BLU) & (LR_LOCI - 1u);
#define TB_PUT(E)                                                                                                       \
                do {                                                                                                   \
                    const uint32_t e__ = (E), code__ = e__ >> 12;                                                      \
                    if (code__ < (uint32_t)T_NCODE)                                                                    \
                        dst[k++] = tile_entry<geo_reg>(((e__ & (LR_LOCI - 1u)) - cbase) & (LR_LOCI - 1u), code__);     \
                } while (0)
#pragma unroll
                for (uint32_t u = 0; u < TB_SEG; u++) TB_PUT(seg[u]);
                for (uint64_t i = lo + TB_SEG; i < hi; i++) TB_PUT((uint32_t)c4r[i]);
#undef TB_PUT
                if (ORDER) s_rcnt[rank] = (uint16_t)k;
                for (; k < K; k++) dst[k] = T_NULL;
                if (staged) {
                    __syncthreads();
                    if (ORDER) {  // wave wv = slice wv, lane = row
                        const uint32_t Kw = slice_k(s_kmax[wv]);
                        const uint32_t rc = tile_lane_assign(s_tile + s_sbase[wv], Kw, lane, s_rcnt[wv * 64 + lane], s_scr + wv * 256);
                        tile_bank_order(s_tile + s_sbase[wv] + slice_row_at(Kw, lane), Kw, rc, lane, s_scr + wv * 256);
                        __syncthreads();
                    }
                    uint4 *out = reinterpret_cast<uint4 *>(tiles + tbase);  // (tile starts and sizes are multiples of 64 u16)
                    const uint4 *in = reinterpret_cast<const uint4 *>(s_tile);
                    for (uint32_t i = cl; i < total / 8u; i += T_BC) out[i] = in[i];
                }
            }
            __syncthreads();  // (the sort's arrays and the staged tile are reused by the next chunk)
            o_lo = o_hi;
            o_hi = o_next;
        }
    }
}

// wave per row/column: count entries that are NOT regular (FILL = false) or copy them in order (FILL = true);
// REST > 0: only those outside the totals 5..REST as well (8: tier 2, i.e. totals 0 and above 8 remain)
template <bool FILL, int REST = 0>
__global__ __launch_bounds__(256) void k_ovf_build(uint64_t n_rows, const uint64_t *__restrict__ ptr,
                                                   const uint64_t *__restrict__ ent, uint64_t *__restrict__ optr,
                                                   uint64_t *__restrict__ oent)
{
    const int lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * 4;
    for (uint64_t row = wave0; row < n_rows; row += nwaves) {
        const uint64_t beg = ptr[row], end = ptr[row + 1];
        uint64_t base = FILL ? optr[row] : 0, cnt = 0;
        for (uint64_t i0 = beg; i0 < end; i0 += 64) {
            const uint64_t i = i0 + lane;
            const uint64_t e = i < end ? ent[i] : 0;
            const bool ov = i < end && !ent_regular(e) && !(REST && ENT_ALT(e) + ENT_REF(e) - T2_NMIN <= (uint32_t)REST - T2_NMIN);
            const unsigned long long m = __ballot(ov);
            if (FILL && ov) oent[base + __popcll(m & ((1ull << lane) - 1ull))] = e;
            base += __popcll(m);
            cnt += __popcll(m);
        }
        if (!FILL && lane == 0) optr[row] = cnt;
    }
}

// wave per locus column: regular entries -> compact u32 (cell | code<<28) in order; per-code histogram
template <bool FILL, int EB>
__global__ __launch_bounds__(256) void k_c4_build(uint64_t L, const uint64_t *__restrict__ csc_ptr,
                                                  const uint64_t *__restrict__ csc_ent, uint64_t *__restrict__ c4_ptr,
                                                  uint32_t *__restrict__ c4_ent, uint32_t *__restrict__ hist_all)
{
    const int lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * 4;
    for (uint64_t l = wave0; l < L; l += nwaves) {
        const uint64_t beg = csc_ptr[l], end = csc_ptr[l + 1];
        uint64_t base = FILL ? c4_ptr[l] : 0, cnt = 0;
        uint32_t myhist = 0;
        for (uint64_t i0 = beg; i0 < end; i0 += 64) {
            const uint64_t i = i0 + lane;
            const uint64_t e = i < end ? csc_ent[i] : 0;
            const bool reg = i < end && ent_regular(e);
            const uint32_t code = reg ? ent_code(e) : 0xffu;
            const unsigned long long m = __ballot(reg);
            if (FILL) {
                if (reg) c4_write1<EB>(c4_ent, base + __popcll(m & ((1ull << lane) - 1ull)), ENT_IDX(e), code);
            } else {
#pragma unroll
                for (int k = 0; k < T_NCODE; k++) {
                    const unsigned long long mk = __ballot(code == (uint32_t)k);
                    if (lane == k) myhist += (uint32_t)__popcll(mk);
                }
            }
            base += __popcll(m);
            cnt += __popcll(m);
        }
        if (!FILL) {
            if (lane == 0) c4_ptr[l] = (cnt + 3) & ~3ull;  // whole 16-byte vectors
            if (lane < T_NCODE) hist_all[l * T_NCODE + lane] = myhist;
        } else if ((uint64_t)lane < ((4 - (cnt & 3)) & 3)) {
            c4_write1<EB>(c4_ent, c4_ptr[l] + cnt + lane, EB == 32 ? 0x0fffffffu : 0xfffffu, 15u);  // padding: code 15 = no entry
        }
    }
}

// compact by-cell entries for k_minority_ranges: locus | code << 28 (code 15: an overflow entry, not counted there) —
// half the bytes of the packed CSR entry, and that kernel runs at the memory rate
__global__ __launch_bounds__(256) void k_cell_compact(uint64_t nnz, const uint64_t *__restrict__ csr_ent, uint16_t *__restrict__ c4r)
{
    static_assert(LR_LOCI == 4096, "12 bits of locus inside its range + 4 bits of code");
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nnz) return;
    const uint64_t e = csr_ent[i];
    c4r[i] = (uint16_t)((ENT_IDX(e) % LR_LOCI) | ((ent_regular(e) ? ent_code(e) : 15u) << 12));
}

// roff[cell][r] = number of the row's entries with locus < r * LR_LOCI, r = 0..R (row sorted by locus).  Wave per row.
__global__ __launch_bounds__(256) void k_range_offsets(uint64_t n_rows, uint32_t R, uint32_t width,
                                                       const uint64_t *__restrict__ csr_ptr,
                                                       const uint64_t *__restrict__ csr_ent, uint32_t *__restrict__ roff)
{
    const int lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * 4;
    for (uint64_t row = wave0; row < n_rows; row += nwaves) {
        const uint64_t beg = csr_ptr[row], end = csr_ptr[row + 1];
        uint32_t *o = roff + row * (R + 1);
        // position i (0..len): ranges above that of entry i-1 up to that of entry i start at i (entry -1: range -1,
        // entry len: range R)
        for (uint64_t i0 = beg; i0 <= end; i0 += 64) {
            const uint64_t i = i0 + lane;
            if (i > end) continue;
            const int r_prev = i > beg ? (int)(ENT_IDX(csr_ent[i - 1]) / width) : -1;
            const int r_here = i < end ? (int)(ENT_IDX(csr_ent[i]) / width) : (int)R;
            for (int r = r_prev + 1; r <= r_here; r++) o[r] = (uint32_t)(i - beg);
        }
    }
}

// The most entries any cell has at ONE locus (1 unless the file repeats a (locus, cell) pair): rows are sorted by locus, so
// the entries of a pair are a run; the lane at a run's first entry measures it.  Wave per row; out: one u32, zeroed.
__global__ __launch_bounds__(256) void k_max_pair_entries(uint64_t n_rows, const uint64_t *__restrict__ csr_ptr,
                                                          const uint64_t *__restrict__ csr_ent, uint32_t *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * 4;
    uint32_t best = 1;
    for (uint64_t row = wave0; row < n_rows; row += nwaves) {
        const uint64_t beg = csr_ptr[row], end = csr_ptr[row + 1];
        for (uint64_t i = beg + 1 + lane; i < end; i += 64) {
            const uint64_t l = ENT_IDX(csr_ent[i]);
            if (ENT_IDX(csr_ent[i - 1]) != l) continue;               // not repeated (nearly always)
            if (i - 1 > beg && ENT_IDX(csr_ent[i - 2]) == l) continue;  // inside a run: its second entry measures it
            uint32_t run = 2;
            for (uint64_t k = i + 1; k < end && ENT_IDX(csr_ent[k]) == l; k++) run++;
            best = max(best, run);
        }
    }
    if (best > 1) atomicMax(out, best);
}

// locus of every overflow entry (by-locus order): wave per locus
__global__ __launch_bounds__(256) void k_ovf_locus_ids(uint64_t L, const uint64_t *__restrict__ ovc_ptr, uint32_t *__restrict__ ovc_locus)
{
    const int lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * 4;
    for (uint64_t l = wave0; l < L; l += nwaves)
        for (uint64_t i = ovc_ptr[l] + lane; i < ovc_ptr[l + 1]; i += 64) ovc_locus[i] = (uint32_t)l;
}

// nmask[l]: bit (n - 4) set iff an overflow entry of locus l has alt+ref == n, 4 <= n <= OV_NE (static)
__global__ __launch_bounds__(256) void k_ovf_nmask(uint64_t L, const uint64_t *__restrict__ ovc_ptr,
                                                   const uint64_t *__restrict__ ovc_ent, uint32_t *__restrict__ nmask)
{
    const int lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * 4;
    for (uint64_t l = wave0; l < L; l += nwaves) {
        uint32_t m = 0;
        for (uint64_t i = ovc_ptr[l] + lane; i < ovc_ptr[l + 1]; i += 64) {
            const uint64_t en = ovc_ent[i];
            const uint32_t n = ENT_ALT(en) + ENT_REF(en);
            if (n >= 4u && n <= (uint32_t)OV_NE) m |= 1u << (n - 4u);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m |= (uint32_t)__shfl_xor((int)m, off, 64);
        if (lane == 0) nmask[l] = m;
    }
}

// the two lists, from the static pair histogram: a thread per locus.  COUNT: pairs / sectors of the locus; FILL: at the offsets
template <bool FILL>
__global__ __launch_bounds__(256) void k_t2_lists(uint64_t L, const uint32_t *__restrict__ hist_all2, uint64_t *__restrict__ np,
                                                  uint64_t *__restrict__ ns, uint32_t *__restrict__ plist, uint32_t *__restrict__ slist,
                                                  uint32_t *__restrict__ pmask /*FILL: bit c2 = the pair occurs at the locus*/)
{
    const uint64_t l = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= L) return;
    uint64_t kp = FILL ? np[l] : 0, ks = FILL ? ns[l] : 0;
    uint32_t secs = 0, pm = 0;
    for (uint32_t c2 = 0; c2 < (uint32_t)T2_NCODE; c2++) {
        if (hist_all2[l * T2_CSTRIDE + c2] == 0u) continue;
        const uint32_t n = 5u + (c2 >= 6u) + (c2 >= 13u) + (c2 >= 21u), r = c2 - t2_code(n, 0u);
        secs |= 1u << (t2_pos(n, r) >> 3);
        pm |= 1u << c2;
        if (FILL) plist[kp] = (uint32_t)(l << 5) | c2;
        kp++;
    }
    for (uint32_t sec = 0; sec < 6u; sec++) {
        if (!((secs >> sec) & 1u)) continue;
        if (FILL) slist[ks] = (uint32_t)(l << 3) | sec;
        ks++;
    }
    if (!FILL) { np[l] = kp; ns[l] = ks; }
    else pmask[l] = pm;
}

// static: how often every tier-2 pair occurs at every locus (all cells of the shard); a thread per overflow entry (by-locus order)
__global__ __launch_bounds__(256) void k_t2_hist(uint64_t n_ovf, const uint32_t *__restrict__ ovc_locus, const uint64_t *__restrict__ ovc_ent,
                                                 uint32_t *__restrict__ hist_all2)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_ovf) return;
    const uint64_t en = ovc_ent[i];
    const uint32_t r = ENT_REF(en), n = ENT_ALT(en) + r;
    if (t2_total(n)) atomicAdd(&hist_all2[(uint64_t)ovc_locus[i] * T2_CSTRIDE + t2_code(n, r)], 1u);
}

// 64-row ELLPACK copy of the overflow CSR.  COUNT: slots of group g = 64 x its longest row; FILL: lane = row & 63 writes
// its entries at ell_ptr[g] + k * 64 + lane and pads.  One wave per group.
template <bool FILL>
__global__ __launch_bounds__(256) void k_ovf_ell_build(uint64_t n_rows, const uint64_t *__restrict__ ovf_ptr,
                                                       const uint64_t *__restrict__ ovf_ent, uint64_t *__restrict__ ell_ptr,
                                                       uint64_t *__restrict__ ell)
{
    const int lane = threadIdx.x & 63;
    const uint64_t grp = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const uint64_t n_grp = (n_rows + 63) >> 6;
    if (grp >= n_grp) return;
    const uint64_t row = grp * 64 + lane;
    uint64_t beg = 0, len = 0;
    if (row < n_rows) { beg = ovf_ptr[row]; len = ovf_ptr[row + 1] - beg; }
    uint64_t kmax = len;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) kmax = max(kmax, (uint64_t)__shfl_xor((long long)kmax, off, 64));
    if (!FILL) {
        if (lane == 0) ell_ptr[grp] = kmax * 64;
        return;
    }
    const uint64_t base = ell_ptr[grp] + lane;
    for (uint64_t k = 0; k < kmax; k++) ell[base + k * 64] = k < len ? ovf_ent[beg + k] : OVF_PAD;
}

// The overflow entries the fast kernel leaves out, as two small lists in row order (static): tier 0 = totals 9..OV_NE (longer
// products; expected term still tabulated), tier 1 = totals above OV_NE (generic paths).  COUNT: entries per row and tier;
// FILL: (row, entry) pairs at the row's offset.  A thread per row.
template <bool FILL>
__global__ __launch_bounds__(256) void k_ovf_tier_lists(uint64_t n_rows, const uint64_t *__restrict__ ovf_ptr,
                                                        const uint64_t *__restrict__ ovf_ent,
                                                        uint64_t *__restrict__ cnt0 /*count: out; fill: offsets*/,
                                                        uint64_t *__restrict__ cnt1, uint32_t *__restrict__ row0,
                                                        uint64_t *__restrict__ ent0, uint32_t *__restrict__ row1,
                                                        uint64_t *__restrict__ ent1)
{
    const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n_rows) return;
    uint64_t k0 = FILL ? cnt0[row] : 0, k1 = FILL ? cnt1[row] : 0;
    for (uint64_t i = ovf_ptr[row], end = ovf_ptr[row + 1]; i < end; i++) {
        const uint64_t en = ovf_ent[i];
        const int t = ovf_tier(en);
        if (t == 0) {
            if (FILL) { row0[k0] = (uint32_t)row; ent0[k0] = en; }
            k0++;
        } else if (t == 1) {
            if (FILL) { row1[k1] = (uint32_t)row; ent1[k1] = en; }
            k1++;
        }
    }
    if (!FILL) { cnt0[row] = k0; cnt1[row] = k1; }
}

// ===========================================================================================================
// Chunk groups of a tile pass (see tiled_build): the count with the shortest modelled makespan of the persistent workgroups,
// rounded so that every group has the same number of chunks (the last one maybe fewer).
static void tile_groups_for(const cellector_ctx *c, uint32_t nb, uint32_t nj, uint32_t *groups_out, uint32_t *cpg_out)
{
    const uint64_t cols = (nb + T_SB_MAX - 1) / T_SB_MAX;
    uint64_t groups = 1;
    double best = 1e300;
    for (uint64_t g = 1; g <= T_GROUPS_MAX && g <= (uint64_t)nj; g++) {
        uint64_t per = (uint64_t)c->n_cu / g;
        if (per < 1) per = 1;
        if (per > cols) per = cols;
        const uint64_t rounds = (cols + per - 1) / per, chunks = ((uint64_t)nj + g - 1) / g;
        const double cost = (double)(rounds * (chunks + 3)) * (1.0 + 0.03 * (g > T_GROUPS ? (double)(g - T_GROUPS) / T_GROUPS : 0.0));
        if (cost < best) { best = cost; groups = g; }
    }
    if (c->tile_groups_opt > 0) groups = (uint64_t)c->tile_groups_opt;  // (A/B runs)
    if (groups > nj) groups = nj;
    *cpg_out = (nj + (uint32_t)groups - 1) / (uint32_t)groups;
    *groups_out = (nj + *cpg_out - 1) / *cpg_out;
}

// the per-tile builder (one workgroup per tile, two searches per row) over nt tiles of the CSR (ptr, ent)
template <bool FILL, class G>
static void launch_tile_build(cellector_ctx *c, uint64_t nt, uint32_t nj, const uint64_t *ptr, const uint64_t *ent, uint64_t *tile_ptr,
                              uint16_t *tiles, uint16_t *thdr)
{
    const uint64_t maxg = 1ull << 30;
    for (uint64_t t0 = 0; t0 < nt; t0 += maxg)
        hipLaunchKernelGGL((k_tile_build<FILL, G>), dim3((unsigned)std::min(nt - t0, maxg)), dim3(T_BC), 0, c->stream, c->nloc, nj, t0, ptr, ent,
                           tile_ptr, tiles, thdr, (const uint32_t *)nullptr);
}

// ---- the kept values of the EM pass' tier-2 lookups (option t2_cache; kernels_tiled.hip, k_t2_cell<.., CACHE>) ----
// One (log-pmf, expected term) per slot of ovf_ell, zero until a pass stores it (padding slots and entries outside tier 2 stay
// zero: they add 0.0), and the (alpha, beta) bits every locus' values were written under: all-ones, which no live locus
// (finite, positive) and no masked one (alpha = -1) has, so every locus starts dirty.  Only where k_t2_cell runs.
cellector_status t2_cache_alloc(cellector_ctx *c)
{
    if (!c->t2 || c->ovf_deep || !c->L || !c->nloc) return CELLECTOR_OK;
    const uint64_t L = c->L, words = (L + 63) / 64 * 2;
    CHK(dev_alloc(c, &c->t2_val, c->ovf_ell_slots));
    CHK(dev_alloc(c, &c->ab_t2, L));
    CHK(dev_alloc(c, &c->ab_last, L));
    CHK(dev_alloc(c, &c->t2_dirty, words));
    HIPCHK(c, hipMemsetAsync(c->t2_val, 0, c->ovf_ell_slots * sizeof(double2), c->stream));
    HIPCHK(c, hipMemsetAsync(c->ab_t2, 0xff, L * sizeof(double2), c->stream));
    HIPCHK(c, hipMemsetAsync(c->ab_last, 0xff, L * sizeof(double2), c->stream));
    HIPCHK(c, hipMemsetAsync(c->t2_dirty, 0xff, words * sizeof(uint32_t), c->stream));
    c->t2_val_exp = true;  // (nothing kept yet)
    return CELLECTOR_OK;
}

// ---- tier-2 tiles (deep coverage): a second tile set over the overflow CSR's entries with totals 5..G::NHI ----
// Built with the per-tile builder (the overflow rows are short); the rows keep
// their file order.  A tile holds all 1024 rows of its block, most of them with one padding entry: 4 bytes per row (K = 1).
template <class G>
static cellector_status t2_tiles_build(cellector_ctx *c)
{
    const uint64_t nloc = c->nloc, L = c->L;
    c->t2_nj = (uint32_t)((L + G::BLU - 1) / G::BLU);
    if (c->t2_nj == 0) c->t2_nj = 1;
    tile_groups_for(c, c->t_nb, c->t2_nj, &c->t2_groups, &c->t2_cpg);
    const uint64_t nt = (uint64_t)c->t_nb * c->t2_nj;
    uint64_t elems = 0;
    CHK(dev_alloc(c, &c->tile2_ptr, nt + 1));
    HIPCHK(c, hipMemsetAsync(c->tile2_ptr + nt, 0, 8, c->stream));
    CHK(count_scan_fill(c, nt, {{c->tile2_ptr, &elems}}, [&](auto FILL) {
        launch_tile_build<FILL.value, G>(c, nt, c->t2_nj, c->ovf_ptr, c->ovf_ent, c->tile2_ptr, c->tiles2, c->thdr2);
    }, [&] {
        CHK(dev_alloc(c, &c->tiles2, elems + 64));  // tail pad: the 16-byte load of the last row runs past its end
        return dev_alloc(c, &c->thdr2, nt * T_HDR);
    }));
    const uint64_t tab_elems = (uint64_t)c->t2_nj * G::LROW * G::BL + 4 * T_THREADS;  // tail pad: the partial last table load
    CHK(dev_alloc(c, &c->tab2c, tab_elems));
    HIPCHK(c, hipMemsetAsync(c->tab2c, 0, tab_elems * sizeof(double), c->stream));  // (zero slots and the slots beyond L stay zero)
    CHK(dev_alloc(c, &c->part2, 3ull * 2 * c->t2_groups * c->t_npad));
    CHK(dev_alloc(c, &c->tile_work2, T_GROUPS_MAX));
    // what the tiles leave to the per-entry kernel (totals 0 and above G::NHI), as a by-cell CSR of its own: walking the whole
    // overflow CSR and skipping the tiles' entries kept that kernel's waves as long as before (a wave waits for its slowest lane)
    CHK(dev_alloc(c, &c->ovr_ptr, nloc + 1));
    HIPCHK(c, hipMemsetAsync(c->ovr_ptr + nloc, 0, 8, c->stream));
    return count_scan_fill(c, nloc, {{c->ovr_ptr, &c->ovr_n}}, [&](auto FILL) {
        hipLaunchKernelGGL((k_ovf_build<FILL.value, (int)G::NHI>), dim3(gcap(nloc, 4)), dim3(256), 0, c->stream, nloc, c->ovf_ptr, c->ovf_ent,
                           c->ovr_ptr, c->ovr_ent);
    }, [&] { return dev_alloc(c, &c->ovr_ent, c->ovr_n); });
}

cellector_status tiled_build(cellector_ctx *c)
{
    const uint64_t nloc = c->nloc, L = c->L;
    if (nloc >= (1ull << 28)) return ctx_fail(c, CELLECTOR_EINVAL, "tiled engine: more than 2^28 cells per shard");
    if (L >= (1ull << 28)) return ctx_fail(c, CELLECTOR_EINVAL, "tiled engine: more than 2^28 loci");
    c->t_nb = (uint32_t)((nloc + T_BC - 1) / T_BC);
    c->t_nj = (uint32_t)((L + T_BLU - 1) / T_BLU);
    if (c->t_nb == 0) c->t_nb = 1;
    if (c->t_nj == 0) c->t_nj = 1;
    // Chunk groups.  The tile kernel runs one persistent workgroup per CU, each bound to a group of locus chunks and fetching
    // columns of T_SB_MAX cell blocks from the group's counter; a cell gets one partial sum per group.  Every workgroup of a
    // group walks the group's chunks once per column it fetches, so the kernel takes about rounds(g) x (chunks(g) + 3)
    // chunk-steps with rounds = ceil(columns / workgroups per group) — a column costs its chunks plus a fixed part
    // (accumulators cleared and written out as partial sums), put at three chunk-steps.  Any count from 1 up is taken, the one
    // with the shortest makespan wins (ties: fewer groups), charging 3 % per 8 groups beyond 8 for the additional partial
    // sums (16 bytes more per cell and pass written by the tile kernel and read by the finalize).  Measured (ms per EM
    // iteration): 10^6 cells x 200k loci (245 columns, 313 chunks): 1 group 2.33, 2: 2.34, 4: 2.36, 7: 2.43, 8: 2.44, 32:
    // 2.59 — with one group every workgroup does one column over all chunks: no ragged last round, no partial sums to add
    // up; 200k cells x 100k loci (49 columns, 157 chunks): 5 groups 0.394 (245 workgroups, one round), 8: 0.430 (two rounds,
    // the second half empty), 2: 0.48, 1: 0.73 (49 CUs busy).  Groups used to be multiples of 8 so that a group's workgroups
    // shared an XCD's L2 for the table reads (workgroup i runs on XCD i mod 8): the figures above show no such need — the
    // workgroups of a group walk the chunks in step, a table chunk is fetched once per XCD either way.
    tile_groups_for(c, c->t_nb, c->t_nj, &c->t_groups, &c->t_cpg);
    c->t_npad = (uint64_t)c->t_nb * T_BC;
    const uint64_t nt = (uint64_t)c->t_nb * c->t_nj;

    // ---- tiles
    CHK(dev_alloc(c, &c->tile_ptr, nt + 1));
    HIPCHK(c, hipMemsetAsync(c->tile_ptr + nt, 0, 8, c->stream));
    // every (cell, chunk) pair's first entry, once per row: the two builder passes searched each row per tile (two binary
    // searches of ~11 scattered probes per cell and tile: 1.4 TB through the L2 at 1M x 200k, 0.2 s)
    DevBuf<uint32_t> toff;  // (stays empty when there is no room for the table: the builder searches)
    if (nloc && dev_alloc(c, &toff, nloc * ((uint64_t)c->t_nj + 1)) == CELLECTOR_OK)
        hipLaunchKernelGGL(k_range_offsets, dim3(gcap(nloc, 4)), dim3(256), 0, c->stream, nloc, c->t_nj, (uint32_t)T_BLU, c->csr_ptr,
                           c->csr_ent, toff);
    // the compact by-cell entries (also the minority-driven locus pass' input): with the offsets table the builder reads these
    CHK(dev_alloc(c, &c->c4r, c->nnz));
    if (c->nnz)
        hipLaunchKernelGGL(k_cell_compact, dim3(gcap(c->nnz, 256, 0x7fffffffu)), dim3(256), 0, c->stream, c->nnz, c->csr_ent, c->c4r);
    const unsigned bgrid = (unsigned)std::min<uint64_t>(c->t_nb, (uint64_t)c->n_cu * 8);  // (one block per CU at a time: LDS)
    auto build2 = [&](auto FILL, auto ORDER) {
        hipLaunchKernelGGL((k_tile_build2<FILL.value, ORDER.value>), dim3(bgrid), dim3(T_BC), 0, c->stream, nloc, c->t_nb, c->t_nj, c->csr_ptr,
                           c->c4r, toff, c->tile_ptr, c->tiles, c->thdr);
    };
    CHK(count_scan_fill(c, nt, {{c->tile_ptr, &c->t_elems}}, [&](auto FILL) {
        if (!toff) launch_tile_build<FILL.value, geo_reg>(c, nt, c->t_nj, c->csr_ptr, c->csr_ent, c->tile_ptr, c->tiles, c->thdr);
        else if constexpr (FILL.value) with_bool(c->bank_order, [&](auto ORDER) { build2(FILL, ORDER); });
        else build2(FILL, std::false_type());  // (the sizes do not depend on the order inside a row)
    }, [&] {
        CHK(dev_alloc(c, &c->tiles, c->t_elems + 64));  // tail pad: the 16-byte load of the last row runs past its end
        return dev_alloc(c, &c->thdr, nt * T_HDR);
    }));
    if (toff) {
        HIPCHK(c, hipStreamSynchronize(c->stream));  // (the block goes back to the allocation cache: no kernel may still read it)
        toff.reset();
    }

    // ---- overflow CSR
    CHK(dev_alloc(c, &c->ovf_ptr, nloc + 1));
    HIPCHK(c, hipMemsetAsync(c->ovf_ptr + nloc, 0, 8, c->stream));
    CHK(count_scan_fill(c, nloc, {{c->ovf_ptr, &c->ovf_n}}, [&](auto FILL) {
        if (nloc)
            hipLaunchKernelGGL(k_ovf_build<FILL.value>, dim3(gcap(nloc, 4)), dim3(256), 0, c->stream, nloc, c->csr_ptr, c->csr_ent, c->ovf_ptr,
                               c->ovf_ent);
    }, [&] { return dev_alloc(c, &c->ovf_ent, c->ovf_n); }));

    // ---- compact CSC + histogram, overflow CSC
    uint64_t n4 = 0, novc = 0;
    CHK(dev_alloc(c, &c->c4_ptr, L + 1));
    CHK(dev_alloc(c, &c->ovc_ptr, L + 1));
    CHK(dev_alloc(c, &c->hist_all, L * T_NCODE));
    HIPCHK(c, hipMemsetAsync(c->c4_ptr + L, 0, 8, c->stream));
    HIPCHK(c, hipMemsetAsync(c->ovc_ptr + L, 0, 8, c->stream));
    CHK(count_scan_fill(c, L, {{c->c4_ptr, &n4}, {c->ovc_ptr, &novc}}, [&](auto FILL) {
        if (!L) return;
        // (the count pass has one form; the entry width is chosen below, from the counts)
        with_bool(FILL.value && c->c4_bits == 24, [&](auto NARROW) {
            if constexpr (FILL.value || !NARROW.value)
                hipLaunchKernelGGL((k_c4_build<FILL.value, NARROW.value ? 24 : 32>), dim3(gcap(L, 4)), dim3(256), 0, c->stream, L, c->csc_ptr,
                                   c->csc_ent, c->c4_ptr, c->c4_ent, c->hist_all);
        });
        hipLaunchKernelGGL(k_ovf_build<FILL.value>, dim3(gcap(L, 4)), dim3(256), 0, c->stream, L, c->csc_ptr, c->csc_ent, c->ovc_ptr, c->ovc_ent);
    }, [&] {
        if (novc != c->ovf_n || n4 < c->nnz - novc)
            return ctx_fail(c, CELLECTOR_EDEVICE, "internal: tiled build entry counts inconsistent (%llu + %llu vs %llu, ovf %llu)",
                            (unsigned long long)n4, (unsigned long long)novc, (unsigned long long)c->nnz,
                            (unsigned long long)c->ovf_n);
        c->c4_bits = (nloc <= (1ull << 20) && c->c4_bits_opt != 32) ? 24 : 32;
        CHK(dev_alloc(c, &c->c4_ent, c->c4_bits == 32 ? n4 : (n4 * 3 + 3) / 4 + 4));
        return dev_alloc(c, &c->ovc_ent, novc);
    }));

    // ---- overflow entries: which paths they take
    if (c->ovf_n >= (1ull << 32)) return ctx_fail(c, CELLECTOR_EINVAL, "tiled engine: more than 2^32 overflow entries per shard");
    // deep coverage: more than 3 % of the entries outside the tables (0.8 % with vartrix-like totals 1 + Geometric(0.7),
    // 13 % with 1 + Geometric(0.4)) — the side-stream arrangement built for "a few entries per row" no longer hides them
    c->ovf_deep = c->ovf_deep_opt >= 0 ? c->ovf_deep_opt != 0 : (c->ovf_n * 100 > c->nnz * 3);
    // tier 2 (k_t2_tables): on by default.  A deep matrix takes it on the LOCUS side only (counts instead of 1300 per-entry
    // evaluations per locus: locus pass 1.6 -> 1.0 ms at 10^6 cells x 200k loci deep); its cell side stays with the arithmetic
    // kernel — 2.3e8 lookups of a line each out of a 77 MB table cost more than evaluating the entries (measured: 9.8 vs 6.1 ms).
    c->t2 = c->ovf_n != 0 && L != 0 && L < (1ull << 27) /* the pair list's keys */ && (c->t2_opt >= 0 ? c->t2_opt != 0 : true);
    // tier-2 tiles: the cell side of the totals 5..8 (or 5..6) of a deep matrix walks tiles of its own (t2_tiles_build)
    c->t2_tiles = 0;
    if (c->ovf_deep && c->ovf_deep_wide && c->ovf_n && nloc && L) c->t2_tiles = c->t2_tiles_opt < 0 ? 8 : c->t2_tiles_opt;
    if (c->t2_tiles == 8) CHK(t2_tiles_build<geo_t2<8>>(c));
    else if (c->t2_tiles == 6) CHK(t2_tiles_build<geo_t2<6>>(c));
    CHK(dev_alloc(c, &c->ovf_sum, 3 * 2 * nloc));
    CHK(dev_alloc(c, &c->ovf_tab, L * OV_ROW));
    CHK(dev_alloc(c, &c->ovc_locus, c->ovf_n));
    if (L && c->ovf_n)
        hipLaunchKernelGGL(k_ovf_locus_ids, dim3(gcap(L, 4)), dim3(256), 0, c->stream, L, c->ovc_ptr, c->ovc_locus);
    if (!(c->t2 && !c->ovf_deep)) {  // (the per-entry paths of a shard without tier 2, and the deep forms)
        CHK(dev_alloc(c, &c->ovf_lp, c->ovf_n));
        CHK(dev_alloc(c, &c->ovf_etab, L * OV_REC));
    }
    CHK(dev_alloc(c, &c->ovf_nmask, L));
    c->ovx_n = 0;
    if (c->t2) {
        // tier 2: static pair histogram, per-iteration counters and table; the by-locus CSC of the entries outside it
        CHK(dev_alloc(c, &c->hist_all2, L * T2_CSTRIDE));
        CHK(dev_alloc(c, &c->cnt2, L * T2_CSTRIDE));
        CHK(dev_alloc(c, &c->tab2, L * T2_ROW));
        HIPCHK(c, hipMemsetAsync(c->hist_all2, 0, L * T2_CSTRIDE * sizeof(uint32_t), c->stream));
        HIPCHK(c, hipMemsetAsync(c->cnt2, 0, L * T2_CSTRIDE * sizeof(uint32_t), c->stream));
        hipLaunchKernelGGL(k_t2_hist, dim3(gcap(c->ovf_n, 256, 0x7fffffffu)), dim3(256), 0, c->stream, c->ovf_n, c->ovc_locus, c->ovc_ent,
                           c->hist_all2);
        {
            DevBuf<uint64_t> np, ns;
            uint64_t tot_p = 0, tot_s = 0;
            CHK(dev_alloc(c, &np, L + 1));
            CHK(dev_alloc(c, &ns, L + 1));
            HIPCHK(c, hipMemsetAsync(np + L, 0, 8, c->stream));
            HIPCHK(c, hipMemsetAsync(ns + L, 0, 8, c->stream));
            CHK(count_scan_fill(c, L, {{np, &tot_p}, {ns, &tot_s}}, [&](auto FILL) {
                hipLaunchKernelGGL(k_t2_lists<FILL.value>, dim3(gcap(L, 256)), dim3(256), 0, c->stream, L, c->hist_all2, np, ns, c->t2_plist,
                                   c->t2_slist, c->t2_pmask);
            }, [&] {
                CHK(dev_alloc(c, &c->t2_plist, tot_p));
                CHK(dev_alloc(c, &c->t2_slist, tot_s));
                return dev_alloc(c, &c->t2_pmask, L);
            }));
            if (hipStreamSynchronize(c->stream) != hipSuccess) return ctx_fail(c, CELLECTOR_EDEVICE, "tier-2 list build failed");
            c->t2_np = (uint32_t)tot_p; c->t2_ns = (uint32_t)tot_s;
        }
        CHK(dev_alloc(c, &c->ovx_ptr, L + 1));
        HIPCHK(c, hipMemsetAsync(c->ovx_ptr + L, 0, 8, c->stream));
        CHK(count_scan_fill(c, L, {{c->ovx_ptr, &c->ovx_n}}, [&](auto FILL) {
            hipLaunchKernelGGL((k_ovf_build<FILL.value, 8>), dim3(gcap(L, 4)), dim3(256), 0, c->stream, L, c->ovc_ptr, c->ovc_ent, c->ovx_ptr,
                               c->ovx_ent);
        }, [&] {
            CHK(dev_alloc(c, &c->ovx_ent, c->ovx_n));
            CHK(dev_alloc(c, &c->ovx_locus, c->ovx_n));
            return dev_alloc(c, &c->ovx_lp, c->ovx_n);
        }));
        if (c->ovx_n)
            hipLaunchKernelGGL(k_ovf_locus_ids, dim3(gcap(L, 4)), dim3(256), 0, c->stream, L, c->ovx_ptr, c->ovx_locus);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->ovc_locus.reset();  // (only the histogram needed it)
    }
    {
        const uint64_t n_grp = (nloc + 63) / 64;
        uint64_t slots = 0;
        CHK(dev_alloc(c, &c->ovf_ell_ptr, n_grp + 1));
        HIPCHK(c, hipMemsetAsync(c->ovf_ell_ptr + n_grp, 0, 8, c->stream));
        CHK(count_scan_fill(c, n_grp, {{c->ovf_ell_ptr, &slots}}, [&](auto FILL) {
            if (nloc)
                hipLaunchKernelGGL(k_ovf_ell_build<FILL.value>, dim3(gcap(n_grp * 64, 256, 0x7fffffffu)), dim3(256), 0, c->stream, nloc,
                                   c->ovf_ptr, c->ovf_ent, c->ovf_ell_ptr, c->ovf_ell);
        }, [&] { return dev_alloc(c, &c->ovf_ell, slots); }));
        c->ovf_ell_slots = slots;
        // (a rebuild dropped the kept lookup values with the copy they follow; a ctx that has them switched off gets them with
        //  its first caching pass, should the option change)
        c->t2_val.reset(); c->ab_t2.reset(); c->ab_last.reset(); c->t2_dirty.reset();
        if (t2_cache_on(c)) CHK(t2_cache_alloc(c));
    }
    // the tier lists of the entries the fast cell-side kernel leaves out
    c->ovf_n_tier[0] = c->ovf_n_tier[1] = 0;
    if (nloc && c->ovf_n) {
        DevBuf<uint64_t> cnt0, cnt1;
        CHK(dev_alloc(c, &cnt0, nloc + 1));
        CHK(dev_alloc(c, &cnt1, nloc + 1));
        HIPCHK(c, hipMemsetAsync(cnt0 + nloc, 0, 8, c->stream));
        HIPCHK(c, hipMemsetAsync(cnt1 + nloc, 0, 8, c->stream));
        CHK(count_scan_fill(c, nloc, {{cnt0, &c->ovf_n_tier[0]}, {cnt1, &c->ovf_n_tier[1]}}, [&](auto FILL) {
            hipLaunchKernelGGL(k_ovf_tier_lists<FILL.value>, dim3(gcap(nloc, 256, 0x7fffffffu)), dim3(256), 0, c->stream, nloc, c->ovf_ptr,
                               c->ovf_ent, cnt0, cnt1, c->ovf_tier_row[0], c->ovf_tier_ent[0], c->ovf_tier_row[1], c->ovf_tier_ent[1]);
        }, [&] {
            for (int t = 0; t < 2; t++) {
                CHK(dev_alloc(c, &c->ovf_tier_row[t], c->ovf_n_tier[t]));
                CHK(dev_alloc(c, &c->ovf_tier_ent[t], c->ovf_n_tier[t]));
            }
            return CELLECTOR_OK;
        }));
        if (hipStreamSynchronize(c->stream) != hipSuccess) return ctx_fail(c, CELLECTOR_EDEVICE, "tier list build failed");
        cnt0.reset(); cnt1.reset();
        CHK(dev_alloc(c, &c->ovf_tier_val, 2 * c->ovf_n_tier[1]));  // (log-pmf, expected term) of the tier-1 entries, per pass
    }
    // which totals the per-entry tables (k_ovf_tables, k_ovf_tables_e) must cover at every locus: those of the entries that
    // take these paths
    if (L && c->ovf_n) {
        if (c->t2 && !c->ovf_deep)  // (a deep matrix' cell side evaluates every overflow entry: its tables cover all totals)
            hipLaunchKernelGGL(k_ovf_nmask, dim3(gcap(L, 4)), dim3(256), 0, c->stream, L, c->ovx_ptr, c->ovx_ent, c->ovf_nmask);
        else
            hipLaunchKernelGGL(k_ovf_nmask, dim3(gcap(L, 4)), dim3(256), 0, c->stream, L, c->ovc_ptr, c->ovc_ent, c->ovf_nmask);
    }
    HIPCHK(c, hipGetLastError());

    // ---- per-iteration workspaces
    // tables: three log-pmf-only sets (posterior passes; set 0 also serves an EM pass without the expected column),
    // then one set of (log-pmf, expected) pairs; tail pad for the unconditional partial last table load
    const uint64_t tab_elems = (uint64_t)c->t_nj * TAB_ELEMS;
    CHK(dev_alloc(c, &c->tab, 4 * tab_elems + 4 * T_THREADS));
    c->tab_em = c->tab;
    c->tab_em_stride = 1;
    CHK(dev_alloc(c, &c->part, 3ull * 2 * c->t_groups * c->t_npad));
    CHK(dev_alloc(c, &c->ab3, 3 * L));
    CHK(dev_alloc(c, &c->masked_cnt, nloc));
    CHK(dev_alloc(c, &c->flag_bits, (nloc + 31) / 32 + 1));
    CHK(dev_alloc(c, &c->tile_work, 3 * T_GROUPS_MAX));
    CHK(dev_alloc(c, &c->minlist, nloc));
    CHK(dev_alloc(c, &c->chg, nloc));
    CHK(dev_alloc(c, &c->tally, L * 16));
    {
        // subsets of the exclusion set: enough (range, subset) workgroups to fill the chip once
        const uint32_t R = (uint32_t)((L + LR_LOCI - 1) / LR_LOCI);
        uint32_t sub = R ? (uint32_t)c->n_cu / R : 1;  // one workgroup per CU (LDS): at most one round of them
        if (sub < 1) sub = 1;
        if (sub > LR_SUB_MAX) sub = LR_SUB_MAX;
        c->lr_sub = sub;
        CHK(dev_alloc(c, &c->hist_min, (uint64_t)sub * L * 16));
        CHK(dev_alloc(c, &c->roff, nloc * (R + 1)));
        // what a subset may hold (locus_by_minority): its u16 counters take 65535 / (most entries of a cell at one locus)
        DevBuf<uint32_t> pair_max;
        CHK(dev_alloc(c, &pair_max, 1));
        HIPCHK(c, hipMemsetAsync(pair_max, 0, sizeof(uint32_t), c->stream));
        if (nloc) {
            hipLaunchKernelGGL(k_range_offsets, dim3(gcap(nloc, 4)), dim3(256), 0, c->stream, nloc, R, (uint32_t)LR_LOCI, c->csr_ptr, c->csr_ent,
                               c->roff);
            hipLaunchKernelGGL(k_max_pair_entries, dim3(gcap(nloc, 4, 1u << 16)), dim3(256), 0, c->stream, nloc, c->csr_ptr, c->csr_ent,
                               pair_max.get());
        }
        HIPCHK(c, hipGetLastError());
        uint32_t h_pair_max = 0;
        HIPCHK(c, hipMemcpyAsync(&h_pair_max, pair_max, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->lr_cap = std::min<uint32_t>(32767u, 65535u / std::max<uint32_t>(1u, h_pair_max));
        // the transposed offsets of the excluded cells, sized for the largest exclusion set the automatic choice hands to the
        // minority-driven form (allocated here, not in the first iteration's locus pass: that cost the first iteration a
        // stream synchronisation and two allocations — and a run has few iterations)
        if (nloc && (c->locus_mode != 1 || c->tally_delta)) {
            c->mroff_cap = ((nloc * LM_NUM / LM_DEN + LT_CELLS) + 63) & ~63ull;
            CHK(dev_alloc(c, &c->mroff, (uint64_t)(R + 1) * c->mroff_cap));
            CHK(dev_alloc(c, &c->mbeg, c->mroff_cap));
        }
    }
    HIPCHK(c, hipMemsetAsync(c->masked_cnt, 0, (nloc ? nloc : 1) * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(c->flag_bits, 0, ((nloc + 31) / 32 + 1) * 4, c->stream));
    if (L) HIPCHK(c, hipMemsetAsync(c->tally, 0, L * 16 * sizeof(uint32_t), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->tiled_ready = true;
    // before the first iteration the exclusion set is empty (cellector_ingest_finish): the zeroed counts (tally, cnt2) are its
    // counts.  (A build after engine-1 iterations is followed by the engine option's invalidation.)
    c->tally_valid = c->iteration == 0;
    return CELLECTOR_OK;
}
