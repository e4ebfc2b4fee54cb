// cellector_restage: a new staged COO from the one the ctx holds — an arbitrary cell subset, renumbered, and per-read
// downsampling — without going back to the files.  Replaces what the reference does on files: rewriting barcodes.tsv and both
// matrices for another load_barcodes (load_data.rs), and combiner's select_cells / barcode mask (combiner/src/main.rs:246-280)
// with its per-read thinning (main.rs:83-88, :102-107).
//
//   ranks   an exclusive scan of keep[] gives every kept cell its new index (ascending old index); the inverse, composed with
//           the origin the ctx holds, is the new cellector_cell_origin
//   count   one number per tile of RESTAGE_TILE entries: how many of them belong to kept cells (keep[] is a byte per cell: it
//           stays in L2)
//   scan    dev_exclusive_scan_u64 over the tile counts only
//   write   recomputes the predicate from the rank table and places the survivors in order: ballot + popcount below the lane
//           inside a wave, the waves' totals through LDS, the tile's offset from the scan; thins the two counts on the way
//
// The draw (restage.py is the numpy twin): for the entry at position i of the arrays the call reads, allele a
// (0 = ref, 1 = alt) and read r = 0..count-1
//   x = mix64(mix64((seed * GOLD) ^ ((i + 1) * GOLD)) + (2 r + a + 1) * GOLD),   removed iff (x >> 11) < T,
//   T = (uint64_t)(downsample_rate * 2^53).
// Keyed by position before the compaction: it does not depend on keep, the grid or the engine.
#include "ctx.h"
#include "mix64.h"

#define RESTAGE_TILE 4096
#define RS_BLOCK 256
#define RS_WAVES (RS_BLOCK / 64)
#define RS_WAVE_SPAN (RESTAGE_TILE / RS_WAVES)  // consecutive entries one wave places
#define RS_ROUNDS (RS_WAVE_SPAN / 64)
#define RS_DROPPED 0xffffffffu

static_assert(RESTAGE_TILE % (RS_WAVES * 64) == 0, "a wave takes whole rounds of 64 entries");

// reads of one count that survive
__device__ __forceinline__ uint32_t rs_thin(uint64_t h, uint32_t count, uint32_t allele, uint64_t T)
{
    uint32_t kept = 0;
    for (uint32_t r = 0; r < count; r++) {
        const uint64_t x = mix64(h + (uint64_t)(2u * r + allele + 1u) * GOLD);
        kept += (x >> 11) < T ? 0u : 1u;
    }
    return kept;
}
__device__ __forceinline__ uint64_t rs_entry_hash(uint64_t seed_gold, uint64_t i) { return mix64(seed_gold ^ ((i + 1) * GOLD)); }

// ---- cell ranks -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RS_BLOCK) void k_rs_keep_flags(uint64_t tc, const uint8_t *__restrict__ keep_in, uint8_t *__restrict__ keep01,
                                                            uint64_t *__restrict__ scan /*[tc + 1]*/)
{
    const uint64_t i = (uint64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
    if (i > tc) return;
    const uint8_t k = (i < tc && keep_in[i]) ? 1 : 0;
    scan[i] = k;
    if (i < tc) keep01[i] = k;
}
__global__ __launch_bounds__(RS_BLOCK) void k_rs_ranks(uint64_t tc, const uint8_t *__restrict__ keep01, const uint64_t *__restrict__ scan,
                                                       const uint32_t *__restrict__ old_origin /*null: identity*/,
                                                       uint32_t *__restrict__ rank, uint32_t *__restrict__ origin)
{
    const uint64_t i = (uint64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
    if (i >= tc) return;
    if (!keep01[i]) {
        rank[i] = RS_DROPPED;
        return;
    }
    const uint64_t r = scan[i];  // (< the number of kept cells: the size of origin)
    rank[i] = (uint32_t)r;
    origin[r] = old_origin ? old_origin[i] : (uint32_t)i;
}

cellector_status restage_cell_ranks(cellector_ctx *c, const uint8_t *host_keep, uint64_t tc, uint64_t n_keep, const uint32_t *old_origin,
                                    DevBuf<uint8_t> *keep01, DevBuf<uint32_t> *rank, DevBuf<uint32_t> *origin)
{
    DevBuf<uint8_t> raw;
    DevBuf<uint64_t> scan;
    CHK(dev_alloc(c, &raw, tc)); CHK(dev_alloc(c, keep01, tc)); CHK(dev_alloc(c, &scan, tc + 1));
    CHK(dev_alloc(c, rank, tc)); CHK(dev_alloc(c, origin, n_keep));
    HIPCHK(c, hipMemcpyAsync(raw, host_keep, tc, hipMemcpyHostToDevice, c->stream));
    const unsigned g = (unsigned)((tc + 1 + RS_BLOCK - 1) / RS_BLOCK);
    hipLaunchKernelGGL(k_rs_keep_flags, dim3(g), dim3(RS_BLOCK), 0, c->stream, tc, raw.get(), keep01->get(), scan.get());
    HIPCHK(c, hipGetLastError());
    uint64_t kept = 0;
    CHK(dev_exclusive_scan_u64(c, scan, tc + 1, &kept));
    if (kept != n_keep) return ctx_fail(c, CELLECTOR_EDEVICE, "restage: the device counts %llu kept cells, the host %llu",
                                        (unsigned long long)kept, (unsigned long long)n_keep);
    hipLaunchKernelGGL(k_rs_ranks, dim3(g), dim3(RS_BLOCK), 0, c->stream, tc, keep01->get(), scan.get(), old_origin, rank->get(),
                       origin->get());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (raw and scan go with this scope; the host array is the caller's)
    return CELLECTOR_OK;
}

// ---- count pass: kept entries per tile ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(RS_BLOCK) void k_rs_count(uint64_t n, uint64_t tc, const uint32_t *__restrict__ cell,
                                                       const uint8_t *__restrict__ keep01, uint64_t *__restrict__ tile_cnt)
{
    __shared__ uint32_t ws[RS_WAVES];
    const uint64_t base = (uint64_t)blockIdx.x * RESTAGE_TILE;
    uint32_t cnt = 0;
#pragma unroll 4
    for (int k = 0; k < RESTAGE_TILE / RS_BLOCK; k++) {
        const uint64_t i = base + (uint64_t)k * RS_BLOCK + threadIdx.x;
        if (i < n) {
            const uint32_t c0 = cell[i];
            if (c0 < tc) cnt += keep01[c0];
        }
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) cnt += __shfl_down(cnt, off, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < RS_WAVES; w++) t += ws[w];
        tile_cnt[blockIdx.x] = t;
    }
}

// ---- write pass -----------------------------------------------------------------------------------------------------------------
// Wave w of a block owns the entries [tile + w * RS_WAVE_SPAN, + RS_WAVE_SPAN) in rounds of 64: the survivors of a round go behind
// those of the rounds, waves and tiles before it, a lane's own behind those of the lower lanes (64-lane ballot masks).
template <bool THIN>
__global__ __launch_bounds__(RS_BLOCK) void k_rs_write(uint64_t n, uint64_t tc, const uint32_t *__restrict__ locus,
                                                       const uint32_t *__restrict__ cell, const uint16_t *__restrict__ alt,
                                                       const uint16_t *__restrict__ ref, const uint32_t *__restrict__ rank,
                                                       const uint64_t *__restrict__ tile_off, uint64_t n_out, uint64_t T,
                                                       uint64_t seed_gold, uint32_t *__restrict__ o_locus, uint32_t *__restrict__ o_cell,
                                                       uint16_t *__restrict__ o_alt, uint16_t *__restrict__ o_ref)
{
    __shared__ uint32_t ws[RS_WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t wbase = (uint64_t)blockIdx.x * RESTAGE_TILE + (uint64_t)w * RS_WAVE_SPAN + lane;
    uint32_t nc[RS_ROUNDS];  // the entry's new cell index, RS_DROPPED for an entry that leaves
    uint32_t wtot = 0;
#pragma unroll
    for (int k = 0; k < RS_ROUNDS; k++) {
        const uint64_t i = wbase + (uint64_t)k * 64;
        uint32_t r = RS_DROPPED;
        if (i < n) {
            const uint32_t c0 = cell[i];
            if (c0 < tc) r = rank[c0];
        }
        nc[k] = r;
        wtot += (uint32_t)__popcll(__ballot(r != RS_DROPPED));
    }
    if (lane == 0) ws[w] = wtot;
    __syncthreads();
    uint64_t pos = tile_off[blockIdx.x];
#pragma unroll
    for (int k = 0; k < RS_WAVES; k++)
        if (k < w) pos += ws[k];
    const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
#pragma unroll
    for (int k = 0; k < RS_ROUNDS; k++) {
        const bool p = nc[k] != RS_DROPPED;
        const uint64_t m = __ballot(p);
        if (p) {
            const uint64_t i = wbase + (uint64_t)k * 64;
            const uint64_t q = pos + (uint64_t)__popcll(m & below);
            if (q < n_out) {  // (always: the count pass saw the same predicate)
                uint32_t a = alt[i], r = ref[i];
                if (THIN) {
                    const uint64_t h = rs_entry_hash(seed_gold, i);
                    r = rs_thin(h, r, 0u, T);
                    a = rs_thin(h, a, 1u, T);
                }
                o_locus[q] = locus[i];
                o_cell[q] = nc[k];
                o_alt[q] = (uint16_t)a;
                o_ref[q] = (uint16_t)r;
            }
        }
        pos += (uint64_t)__popcll(m);
    }
}

cellector_status restage_select(cellector_ctx *c, const CooView &in, uint64_t tc, const uint8_t *keep01, const uint32_t *rank, uint64_t T,
                                uint64_t seed, StagedCoo *out)
{
    const uint64_t n = in.n, ntiles = (n + RESTAGE_TILE - 1) / RESTAGE_TILE;
    DevBuf<uint64_t> tile_cnt;
    CHK(dev_alloc(c, &tile_cnt, ntiles + 1));
    HIPCHK(c, hipMemsetAsync(tile_cnt + ntiles, 0, 8, c->stream));
    if (ntiles) hipLaunchKernelGGL(k_rs_count, dim3((unsigned)ntiles), dim3(RS_BLOCK), 0, c->stream, n, tc, in.cell, keep01, tile_cnt.get());
    HIPCHK(c, hipGetLastError());
    uint64_t kept = 0;
    CHK(dev_exclusive_scan_u64(c, tile_cnt, ntiles + 1, &kept));
    CHK(out->alloc(c, kept));
    if (ntiles) {
        if (T)
            hipLaunchKernelGGL(k_rs_write<true>, dim3((unsigned)ntiles), dim3(RS_BLOCK), 0, c->stream, n, tc, in.locus, in.cell, in.alt, in.ref,
                               rank, tile_cnt.get(), kept, T, seed * GOLD, out->locus.get(), out->cell.get(), out->alt.get(), out->ref.get());
        else
            hipLaunchKernelGGL(k_rs_write<false>, dim3((unsigned)ntiles), dim3(RS_BLOCK), 0, c->stream, n, tc, in.locus, in.cell, in.alt, in.ref,
                               rank, tile_cnt.get(), kept, T, seed * GOLD, out->locus.get(), out->cell.get(), out->alt.get(), out->ref.get());
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CELLECTOR_OK;
}

// ---- all cells: no count pass, no scan; every entry stays where it is and only its two counts change --------------------------
__global__ __launch_bounds__(RS_BLOCK) void k_rs_thin(uint64_t n, uint16_t *__restrict__ alt, uint16_t *__restrict__ ref, uint64_t T,
                                                      uint64_t seed_gold)
{
    const uint64_t i = (uint64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t h = rs_entry_hash(seed_gold, i);
    ref[i] = (uint16_t)rs_thin(h, ref[i], 0u, T);
    alt[i] = (uint16_t)rs_thin(h, alt[i], 1u, T);
}

cellector_status restage_thin(cellector_ctx *c, StagedCoo *coo, uint64_t T, uint64_t seed)
{
    if (!coo->n || !T) return CELLECTOR_OK;
    hipLaunchKernelGGL(k_rs_thin, dim3((unsigned)((coo->n + RS_BLOCK - 1) / RS_BLOCK)), dim3(RS_BLOCK), 0, c->stream, coo->n,
                       coo->alt.get(), coo->ref.get(), T, seed * GOLD);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CELLECTOR_OK;
}
