// cellector_combine: the entries of a second staged COO merged into the one the ctx holds, without going back to the files.
// Replaces the other half of the reference's `combiner` (cellector_restage is the first): the second dataset's loci renumbered
// into the first one's (get_locus_mapping, combiner/src/main.rs:197-231), its cells put behind the first one's
// (main.rs:161-186) and everything written in the order of lines.sort() (main.rs:111) on the tuple (locus, cell, ref, alt).
//
//   map      one pass over the temporary restage_select made of src's selected entries: locus through the map, cell + n_ctx
//   check    per side, is the 64-bit key locus << 32 | cell strictly ascending?  (Every vartrix file, the synthetic generator
//            and any restage of either: yes.)  Such a side is taken as it stands: strictly ascending means no repeated pair,
//            so the tuple's last two fields never decide.
//   sort     a side that is not: two stable radix passes (ref << 16 | alt, then the key) over a permutation, then a gather
//   merge    merge path over tiles of COMBINE_TILE output entries.  A partition kernel binary-searches every tile's diagonal
//            in the two key streams; the tile kernel stages its two key ranges in LDS, ranks every entry (own index + the
//            other side's keys below it: a binary search in LDS), and writes the four arrays in output order.  Each input is
//            read once, the output written once; no sort of the large side, no double buffers.
//
// The two sides' cell ranges are disjoint, so no comparison across sides is ever equal; the partition and the rank still share
// one convention (side A first), and a run of equal keys inside one side may straddle a tile edge freely: its members' ranks
// differ by their own index only.
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "ctx.h"

// output entries per tile (combine.py exports it as TILE)
#define COMBINE_TILE 2048
#define CB_BLOCK 256
#define CB_ITEMS (COMBINE_TILE / CB_BLOCK)

static_assert(COMBINE_TILE % CB_BLOCK == 0, "a tile is whole rounds of the block");
static_assert(COMBINE_TILE <= 65536, "an entry's place inside its tile is kept in 16 bits");

static inline unsigned cb_grid(uint64_t n) { return (unsigned)((n + CB_BLOCK - 1) / CB_BLOCK ? (n + CB_BLOCK - 1) / CB_BLOCK : 1); }

__device__ __forceinline__ uint64_t cb_key(const uint32_t *__restrict__ locus, const uint32_t *__restrict__ cell, uint64_t i)
{
    return (uint64_t)locus[i] << 32 | (uint64_t)cell[i];
}

// ---- map ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CB_BLOCK) void k_cb_map(uint64_t n, uint64_t n_map, uint32_t *__restrict__ locus, uint32_t *__restrict__ cell,
                                                     const uint32_t *__restrict__ map /*null: identity*/, uint32_t cell_add)
{
    const uint64_t i = (uint64_t)blockIdx.x * CB_BLOCK + threadIdx.x;
    if (i >= n) return;
    if (map) {
        const uint32_t l = locus[i];
        if (l < n_map) locus[i] = map[l];  // (always: the staged loci are below src's total_loci)
    }
    cell[i] += cell_add;
}

cellector_status combine_map(cellector_ctx *c, StagedCoo *coo, const uint32_t *d_map, uint64_t n_map, uint32_t cell_add)
{
    if (!coo->n) return CELLECTOR_OK;
    hipLaunchKernelGGL(k_cb_map, dim3(cb_grid(coo->n)), dim3(CB_BLOCK), 0, c->stream, coo->n, n_map, coo->locus.get(), coo->cell.get(), d_map,
                       cell_add);
    HIPCHK(c, hipGetLastError());
    return CELLECTOR_OK;
}

// ---- order check --------------------------------------------------------------------------------------------------------------
// both sides in one launch: broken[0] / broken[1] become 1 when side a / b has a key that does not exceed the one before it
__global__ __launch_bounds__(CB_BLOCK) void k_cb_ascending(uint64_t na, const uint32_t *__restrict__ a_locus, const uint32_t *__restrict__ a_cell,
                                                           uint64_t nb, const uint32_t *__restrict__ b_locus, const uint32_t *__restrict__ b_cell,
                                                           uint32_t *__restrict__ broken)
{
    const uint64_t i = (uint64_t)blockIdx.x * CB_BLOCK + threadIdx.x + 1;
    const int bad_a = i < na && cb_key(a_locus, a_cell, i - 1) >= cb_key(a_locus, a_cell, i);
    const int bad_b = i < nb && cb_key(b_locus, b_cell, i - 1) >= cb_key(b_locus, b_cell, i);
    const int any_a = __syncthreads_or(bad_a), any_b = __syncthreads_or(bad_b);  // (a predicate each: the result is 0 or not 0)
    if (threadIdx.x == 0) {  // (every block that writes writes the same value)
        if (any_a) broken[0] = 1u;
        if (any_b) broken[1] = 1u;
    }
}

cellector_status combine_ascending(cellector_ctx *c, const CooView &a, const CooView &b, bool *a_ascending, bool *b_ascending)
{
    *a_ascending = *b_ascending = true;
    const uint64_t n = a.n > b.n ? a.n : b.n;
    if (n < 2) return CELLECTOR_OK;
    DevBuf<uint32_t> broken;
    CHK(dev_alloc(c, &broken, 2));
    HIPCHK(c, hipMemsetAsync(broken, 0, 8, c->stream));
    hipLaunchKernelGGL(k_cb_ascending, dim3(cb_grid(n - 1)), dim3(CB_BLOCK), 0, c->stream, a.n, a.locus, a.cell, b.n, b.locus, b.cell,
                       broken.get());
    HIPCHK(c, hipGetLastError());
    uint32_t h[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(h, broken, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *a_ascending = h[0] == 0;
    *b_ascending = h[1] == 0;
    return CELLECTOR_OK;
}

// ---- sort of a side that is not strictly ascending, by (locus, cell, ref, alt) ---------------------------------------------------
__global__ __launch_bounds__(CB_BLOCK) void k_cb_sort_init(uint64_t n, const uint16_t *__restrict__ alt, const uint16_t *__restrict__ ref,
                                                           uint32_t *__restrict__ key, uint64_t *__restrict__ perm)
{
    const uint64_t i = (uint64_t)blockIdx.x * CB_BLOCK + threadIdx.x;
    if (i >= n) return;
    key[i] = (uint32_t)ref[i] << 16 | (uint32_t)alt[i];
    perm[i] = i;
}
__global__ __launch_bounds__(CB_BLOCK) void k_cb_sort_keys(uint64_t n, const uint64_t *__restrict__ perm, const uint32_t *__restrict__ locus,
                                                           const uint32_t *__restrict__ cell, uint64_t *__restrict__ key)
{
    const uint64_t i = (uint64_t)blockIdx.x * CB_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t j = perm[i];
    if (j < n) key[i] = cb_key(locus, cell, j);
}
__global__ __launch_bounds__(CB_BLOCK) void k_cb_permute(uint64_t n, const uint64_t *__restrict__ perm, const uint32_t *__restrict__ locus,
                                                         const uint32_t *__restrict__ cell, const uint16_t *__restrict__ alt,
                                                         const uint16_t *__restrict__ ref, uint32_t *__restrict__ o_locus,
                                                         uint32_t *__restrict__ o_cell, uint16_t *__restrict__ o_alt, uint16_t *__restrict__ o_ref)
{
    const uint64_t i = (uint64_t)blockIdx.x * CB_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t j = perm[i];
    if (j >= n) return;  // (never: perm is a permutation of 0..n-1)
    o_locus[i] = locus[j]; o_cell[i] = cell[j]; o_alt[i] = alt[j]; o_ref[i] = ref[j];
}

cellector_status combine_sort(cellector_ctx *c, const CooView &v, StagedCoo *out)
{
    const uint64_t n = v.n;
    DevBuf<uint64_t> perm, perm_o;
    {
        // pass 1: the tuple's last two fields
        DevBuf<uint32_t> k32, k32_o;
        CHK(dev_alloc(c, &k32, n)); CHK(dev_alloc(c, &k32_o, n)); CHK(dev_alloc(c, &perm, n)); CHK(dev_alloc(c, &perm_o, n));
        hipLaunchKernelGGL(k_cb_sort_init, dim3(cb_grid(n)), dim3(CB_BLOCK), 0, c->stream, n, v.alt, v.ref, k32.get(), perm.get());
        HIPCHK(c, hipGetLastError());
        CHK(dev_sort_pairs_u32_u64(c, k32, k32_o, perm, perm_o, n, 32));
    }
    {
        // pass 2 (stable): the key
        DevBuf<uint64_t> k64, k64_o;
        DevBuf<char> tmp;
        CHK(dev_alloc(c, &k64, n)); CHK(dev_alloc(c, &k64_o, n));
        hipLaunchKernelGGL(k_cb_sort_keys, dim3(cb_grid(n)), dim3(CB_BLOCK), 0, c->stream, n, perm_o.get(), v.locus, v.cell, k64.get());
        HIPCHK(c, hipGetLastError());
        size_t tmp_bytes = 0;
        HIPCHK(c, rocprim::radix_sort_pairs(nullptr, tmp_bytes, k64.get(), k64_o.get(), perm_o.get(), perm.get(), (size_t)n, 0u, 64u, c->stream));
        CHK(dev_alloc(c, &tmp, tmp_bytes));
        hipError_t e = rocprim::radix_sort_pairs(tmp.get(), tmp_bytes, k64.get(), k64_o.get(), perm_o.get(), perm.get(), (size_t)n, 0u, 64u, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        HIPCHK(c, e);
    }
    perm_o.reset();
    CHK(out->alloc(c, n));
    hipLaunchKernelGGL(k_cb_permute, dim3(cb_grid(n)), dim3(CB_BLOCK), 0, c->stream, n, perm.get(), v.locus, v.cell, v.alt, v.ref,
                       out->locus.get(), out->cell.get(), out->alt.get(), out->ref.get());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    out->sorted = true;
    return CELLECTOR_OK;
}

// ---- merge ----------------------------------------------------------------------------------------------------------------------
// a_start[t] = how many of the first min(t * COMBINE_TILE, na + nb) output entries come from side A: the lowest a with
// A[a] > B[d - 1 - a] (side A first among equals)
__global__ __launch_bounds__(CB_BLOCK) void k_cb_partition(uint64_t na, const uint32_t *__restrict__ a_locus, const uint32_t *__restrict__ a_cell,
                                                           uint64_t nb, const uint32_t *__restrict__ b_locus, const uint32_t *__restrict__ b_cell,
                                                           uint64_t ntiles, uint64_t *__restrict__ a_start /*[ntiles + 1]*/)
{
    const uint64_t t = (uint64_t)blockIdx.x * CB_BLOCK + threadIdx.x;
    if (t > ntiles) return;
    const uint64_t n = na + nb;
    const uint64_t d = t * COMBINE_TILE < n ? t * COMBINE_TILE : n;
    uint64_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);  // (mid < na; 0 <= d - 1 - mid < nb)
        if (cb_key(a_locus, a_cell, mid) <= cb_key(b_locus, b_cell, d - 1 - mid)) lo = mid + 1;
        else hi = mid;
    }
    a_start[t] = lo;
}

__global__ __launch_bounds__(CB_BLOCK) void k_cb_merge(uint64_t na, const uint32_t *__restrict__ a_locus, const uint32_t *__restrict__ a_cell,
                                                       const uint16_t *__restrict__ a_alt, const uint16_t *__restrict__ a_ref, uint64_t nb,
                                                       const uint32_t *__restrict__ b_locus, const uint32_t *__restrict__ b_cell,
                                                       const uint16_t *__restrict__ b_alt, const uint16_t *__restrict__ b_ref,
                                                       const uint64_t *__restrict__ a_start, uint32_t *__restrict__ o_locus,
                                                       uint32_t *__restrict__ o_cell, uint16_t *__restrict__ o_alt, uint16_t *__restrict__ o_ref,
                                                       uint32_t *__restrict__ inconsistent)
{
    __shared__ uint64_t keys[COMBINE_TILE];  // side A's range, then side B's
    __shared__ uint16_t from[COMBINE_TILE];  // per output entry of the tile: its index in keys
    const uint64_t n = na + nb;
    const uint64_t base = (uint64_t)blockIdx.x * COMBINE_TILE;
    const uint64_t end = base + COMBINE_TILE < n ? base + COMBINE_TILE : n;
    const uint64_t a0 = a_start[blockIdx.x], a1 = a_start[blockIdx.x + 1];
    // A partition that is not monotone or leaves a side, or a rank outside the tile, means a side was not ascending: nothing out
    // of range is touched, the word is raised and the host fails the call (the tile's output is then not complete)
    if (a0 > a1 || a1 > na || a0 > base || a1 > end || base - a0 > end - a1 || end - a1 > nb) {
        if (threadIdx.x == 0) *inconsistent = 1u;
        return;
    }
    const uint64_t b0 = base - a0, b1 = end - a1;
    const uint32_t ca = (uint32_t)(a1 - a0), cb = (uint32_t)(b1 - b0), cnt = ca + cb;  // cnt = end - base <= COMBINE_TILE
#pragma unroll
    for (int k = 0; k < CB_ITEMS; k++) {
        const uint32_t j = (uint32_t)k * CB_BLOCK + threadIdx.x;
        if (j < ca) keys[j] = cb_key(a_locus, a_cell, a0 + j);
        else if (j < cnt) keys[j] = cb_key(b_locus, b_cell, b0 + (j - ca));
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CB_ITEMS; k++) {
        const uint32_t j = (uint32_t)k * CB_BLOCK + threadIdx.x;
        if (j >= cnt) continue;
        const uint64_t key = keys[j];
        uint32_t pos;
        if (j < ca) {  // own index + side B's keys below
            uint32_t lo = 0, hi = cb;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (keys[ca + mid] < key) lo = mid + 1;
                else hi = mid;
            }
            pos = j + lo;
        } else {  // own index + side A's keys not above
            uint32_t lo = 0, hi = ca;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (keys[mid] <= key) lo = mid + 1;
                else hi = mid;
            }
            pos = (j - ca) + lo;
        }
        if (pos < cnt) from[pos] = (uint16_t)j;
        else *inconsistent = 1u;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CB_ITEMS; k++) {
        const uint32_t r = (uint32_t)k * CB_BLOCK + threadIdx.x;
        if (r >= cnt) continue;
        const uint32_t j = from[r];
        if (j >= cnt) { *inconsistent = 1u; continue; }
        const uint64_t key = keys[j];
        uint16_t a, f;
        if (j < ca) { a = a_alt[a0 + j]; f = a_ref[a0 + j]; }
        else { a = b_alt[b0 + (j - ca)]; f = b_ref[b0 + (j - ca)]; }
        o_locus[base + r] = (uint32_t)(key >> 32);
        o_cell[base + r] = (uint32_t)key;
        o_alt[base + r] = a;
        o_ref[base + r] = f;
    }
}

cellector_status combine_merge(cellector_ctx *c, const CooView &a, const CooView &b, StagedCoo *out)
{
    const uint64_t n = a.n + b.n, ntiles = (n + COMBINE_TILE - 1) / COMBINE_TILE;
    DevBuf<uint64_t> a_start;
    DevBuf<uint32_t> inconsistent;
    CHK(dev_alloc(c, &a_start, ntiles + 1)); CHK(dev_alloc(c, &inconsistent, 1));
    HIPCHK(c, hipMemsetAsync(inconsistent, 0, 4, c->stream));
    CHK(out->alloc(c, n));
    if (ntiles) {
        hipLaunchKernelGGL(k_cb_partition, dim3(cb_grid(ntiles + 1)), dim3(CB_BLOCK), 0, c->stream, a.n, a.locus, a.cell, b.n, b.locus, b.cell,
                           ntiles, a_start.get());
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(k_cb_merge, dim3((unsigned)ntiles), dim3(CB_BLOCK), 0, c->stream, a.n, a.locus, a.cell, a.alt, a.ref, b.n, b.locus,
                           b.cell, b.alt, b.ref, a_start.get(), out->locus.get(), out->cell.get(), out->alt.get(), out->ref.get(), inconsistent.get());
        HIPCHK(c, hipGetLastError());
    }
    uint32_t bad = 0;
    HIPCHK(c, hipMemcpyAsync(&bad, inconsistent, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (bad) return ctx_fail(c, CELLECTOR_EDEVICE, "combine: the merge met a side that does not ascend by (locus, cell)");
    out->sorted = true;
    return CELLECTOR_OK;
}

// ---- the cells: origin and source ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CB_BLOCK) void k_cb_cells(uint64_t n_ctx, uint64_t n_kept, const uint32_t *__restrict__ old_origin /*null: identity*/,
                                                       const uint32_t *__restrict__ src_origin, const uint8_t *__restrict__ old_source /*null: 0*/,
                                                       uint8_t k, uint32_t *__restrict__ origin, uint8_t *__restrict__ source)
{
    const uint64_t i = (uint64_t)blockIdx.x * CB_BLOCK + threadIdx.x;
    if (i >= n_ctx + n_kept) return;
    if (i < n_ctx) {
        origin[i] = old_origin ? old_origin[i] : (uint32_t)i;
        source[i] = old_source ? old_source[i] : (uint8_t)0;
    } else {
        origin[i] = src_origin[i - n_ctx];
        source[i] = k;
    }
}

cellector_status combine_cells(cellector_ctx *c, uint64_t n_ctx, uint64_t n_kept, const uint32_t *old_origin, const uint32_t *src_origin,
                               const uint8_t *old_source, uint8_t k, DevBuf<uint32_t> *origin, DevBuf<uint8_t> *source)
{
    const uint64_t n = n_ctx + n_kept;
    CHK(dev_alloc(c, origin, n)); CHK(dev_alloc(c, source, n));
    hipLaunchKernelGGL(k_cb_cells, dim3(cb_grid(n)), dim3(CB_BLOCK), 0, c->stream, n_ctx, n_kept, old_origin, src_origin, old_source, k,
                       origin->get(), source->get());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CELLECTOR_OK;
}

// cellector_restage composes the source like the origin: the kept cells' values at their new index
__global__ __launch_bounds__(CB_BLOCK) void k_cb_source_select(uint64_t tc, uint64_t n_keep, const uint32_t *__restrict__ rank,
                                                               const uint8_t *__restrict__ old_source, uint8_t *__restrict__ source)
{
    const uint64_t i = (uint64_t)blockIdx.x * CB_BLOCK + threadIdx.x;
    if (i >= tc) return;
    const uint32_t r = rank[i];
    if (r < n_keep) source[r] = old_source[i];  // (a dropped cell's rank is ~0u)
}

cellector_status combine_source_select(cellector_ctx *c, uint64_t tc, uint64_t n_keep, const uint32_t *rank, const uint8_t *old_source,
                                       DevBuf<uint8_t> *source)
{
    CHK(dev_alloc(c, source, n_keep));
    hipLaunchKernelGGL(k_cb_source_select, dim3(cb_grid(tc)), dim3(CB_BLOCK), 0, c->stream, tc, n_keep, rank, old_source, source->get());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CELLECTOR_OK;
}
