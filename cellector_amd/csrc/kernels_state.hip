// Placing the EM state (cellector_set_excluded, cellector_set_loci_mask, cellector_em_reset): the kernels that form, from a
// caller's exclusion flags, the per-locus minority tallies an iteration's locus pass would have left in CELLECTOR_XCHG_LOCUS.
//
// The exclusion set and the loci mask are the whole EM state (main.rs:37-48); the tallies are derived from the set:
//   cells_min[l] = entries of the set's cells at locus l, alt_min[l] / ref_min[l] = their allele counts (main.rs:368-420).
// They seed init_alpha_betas (main.rs:598-611) and the posterior alpha/betas (main.rs:239-246).  The recount walks only the
// excluded cells' rows of the by-cell CSR (resident under both engines) and adds with integer atomics: sums of integers are
// exact and independent of the order the hardware performs them in, so the planes are the bits any other tally of the same
// set gives (k_locus_stats, k_locus_finalize).
#include "ctx.h"

#define ST_THREADS 256
#define ST_WAVES (ST_THREADS / 64)

// the excluded local cells as a list: one atomic per wave reserves the wave's slots (the idiom of res_append, kernels_resolve.hip).
// The list's order depends on the order of those atomics; only order-independent integer sums are derived from it.
__global__ __launch_bounds__(ST_THREADS) void k_state_list(uint64_t n, const uint8_t *__restrict__ flags, uint32_t *__restrict__ list,
                                                           uint32_t *__restrict__ cnt)
{
    const uint64_t stride = (uint64_t)gridDim.x * ST_THREADS;
    const uint64_t n_round = (n + 63) / 64 * 64;  // whole waves take part in the ballot
    const int lane = threadIdx.x & 63;
    for (uint64_t i = (uint64_t)blockIdx.x * ST_THREADS + threadIdx.x; i < n_round; i += stride) {
        const bool in = i < n && flags[i] != 0;
        const unsigned long long m = __ballot(in);
        if (!m) continue;
        const int leader = __ffsll((long long)m) - 1;
        uint32_t pos = 0;
        if (lane == leader) pos = atomicAdd(cnt, (uint32_t)__popcll(m));
        pos = __shfl(pos, leader, 64);
        if (in) list[pos + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (uint32_t)i;
    }
}

// one wave per listed cell, lanes over the row's entries (a row is ~2000 entries at 200k loci x 1 % density); acc = [3][L] u64:
// entries, alt, ref per locus.  64-bit sums: 65535 reads per entry times 10^6 cells does not fit 32 bits.
__global__ __launch_bounds__(ST_THREADS) void k_state_tally(const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ list,
                                                            const uint64_t *__restrict__ row_ptr, const uint64_t *__restrict__ ent, uint64_t L,
                                                            unsigned long long *__restrict__ acc)
{
    const uint32_t n_list = *cnt;
    const int lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t)blockIdx.x * ST_WAVES + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * ST_WAVES;
    for (uint64_t j = wave0; j < n_list; j += nwaves) {
        const uint32_t row = list[j];
        const uint64_t beg = row_ptr[row], end = row_ptr[row + 1];
        for (uint64_t i = beg + lane; i < end; i += 64) {
            const uint64_t en = ent[i];
            const uint64_t l = ENT_IDX(en);
            const uint32_t a = ENT_ALT(en), r = ENT_REF(en);
            atomicAdd(&acc[l], 1ull);
            if (a) atomicAdd(&acc[L + l], (unsigned long long)a);
            if (r) atomicAdd(&acc[2 * L + l], (unsigned long long)r);
        }
    }
}

// the five planes and the counters of this shard's LOCUS buffer: what an iteration that ended with this set would have left,
// its contribution sums apart (they belong to a pass that was never run: zero).  A masked locus has no PMFData (main.rs:556):
// its cell count is zero, its allele tallies count (they ignore the mask, like k_locus_stats').
__global__ void k_state_planes(uint64_t L, const unsigned long long *__restrict__ acc, const uint8_t *__restrict__ mask,
                               const uint32_t *__restrict__ cnt, double *__restrict__ out)
{
    const uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < LC_COUNTERS)
        out[(uint64_t)LB_PLANES * L + threadIdx.x] = threadIdx.x == LC_N_EXCLUDED ? (double)*cnt : 0.0;
    if (l >= L) return;
    out[LB_CONTRIB_MIN * L + l] = 0.0;
    out[LB_CONTRIB_MAJ * L + l] = 0.0;
    out[LB_CELLS_MIN * L + l] = mask[l] ? (double)acc[l] : 0.0;
    out[LB_ALT_MIN * L + l] = (double)acc[L + l];
    out[LB_REF_MIN * L + l] = (double)acc[2 * L + l];
}

static inline unsigned st_grid(uint64_t n, unsigned per_block, unsigned cap)
{
    uint64_t g = (n + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (unsigned)g;
}

// places host_flags [nloc, 0 / 1] in c->flags and forms this shard's tallies and its member count in c->x_locus (the caller
// exchanges them).  The scratch is allocated before anything is written: a failed allocation leaves the ctx as it was.
cellector_status launch_state_tallies(cellector_ctx *c, const uint8_t *host_flags)
{
    const uint64_t L = c->L, n = c->nloc;
    DevBuf<uint32_t> list, cnt;
    DevBuf<unsigned long long> acc;
    CHK(dev_alloc(c, &list, n));
    CHK(dev_alloc(c, &cnt, 1));
    CHK(dev_alloc(c, &acc, 3 * L));
    if (n) HIPCHK(c, hipMemcpyAsync(c->flags, host_flags, n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(cnt, 0, sizeof(uint32_t), c->stream));
    HIPCHK(c, hipMemsetAsync(acc, 0, (L ? 3 * L : 1) * sizeof(unsigned long long), c->stream));
    if (n) {
        hipLaunchKernelGGL(k_state_list, dim3(st_grid(n, ST_THREADS * 4, 4096)), dim3(ST_THREADS), 0, c->stream, n, c->flags.get(),
                           list.get(), cnt.get());
        // (the grid is sized for the whole shard: the list's length stays on the device)
        hipLaunchKernelGGL(k_state_tally, dim3(st_grid(n, ST_WAVES, 8192)), dim3(ST_THREADS), 0, c->stream, cnt.get(), list.get(),
                           c->csr_ptr.get(), c->csr_ent.get(), L, acc.get());
    }
    hipLaunchKernelGGL(k_state_planes, dim3(st_grid(L, 256, 0x7fffffffu)), dim3(256), 0, c->stream, L, acc.get(), c->mask.get(), cnt.get(),
                       c->x_locus);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (the scratch goes back to the cache on return; host_flags may go)
    return CELLECTOR_OK;
}
