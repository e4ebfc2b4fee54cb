// Locus moments: per used locus the expected log-likelihood contribution and its variance, split by an exclusion set — what
// locus_expected_contribution_minority / _majority of get_locus_log_likelihoods would hold if main.rs:394 pushed
// pmf_data.expected_log_pmf instead of a copy of log_pmf (quirk Q6), plus the matching sums of expected_log_variance.
//
// E (stats.rs:19-22) and V (stats.rs:23-28) depend on (locus, alt + ref) alone, so a locus' sum over the entries of a class of
// cells is a count per total times a table value.  The kernels stream the by-cell CSR only, which both engines keep:
//   k_lm_count     a wave per row (rows of the class only): one integer atomic per entry with a total up to DM_MOM_SMALL on
//                  hist[locus][total] — exact and free of any order;
//   far list       the entries with larger totals as (locus; cell, total), grouped by locus, ascending cell inside a locus, a
//                  repeated (locus, cell) pair in row order: count / scan / fill over the rows in cell order (k_lm_far_count,
//                  k_lm_far_fill), a stable sort by locus, a pointer array (k_lm_far_ptr).  Static per matrix, as is the
//                  all-cells histogram (k_lm_count without flags): the majority's counts are all - minority, as integers;
//   k_lm_finalize  a wave per used locus: lanes 0..16 evaluate E and V of the totals 1..17 (dm_pmf_moments_small, the bits
//                  cellector_cell_pmfs returns), the four sums are formed total by total, ascending, one rounded product and one
//                  rounded addition each, then the locus' far entries are added one by one in list order, each evaluated by the
//                  whole wave (dm_pmf_moments_wave).
// The result depends on the matrix, the flags and alpha/beta alone: not on the engine, bank_order or the grid.
#include "ctx.h"
#include "device_math.h"

#define LMOM_WAVES 4
#define LMOM_BLOCK (LMOM_WAVES * 64)
#define LMOM_ROW (DM_MOM_SMALL + 1)  // counters per locus: totals 0..17

__global__ __launch_bounds__(LMOM_BLOCK) void k_lm_count(uint64_t n_rows, const uint64_t *__restrict__ row_ptr,
                                                         const uint64_t *__restrict__ ent, const uint8_t *__restrict__ flags /*null: every row*/,
                                                         uint32_t *__restrict__ hist)
{
    const int lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t)blockIdx.x * LMOM_WAVES + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * LMOM_WAVES;
    for (uint64_t row = wave0; row < n_rows; row += nwaves) {
        if (flags && !flags[row]) continue;
        const uint64_t beg = row_ptr[row], end = row_ptr[row + 1];
        // (a row is sorted by locus: the lanes of a step hit 64 different loci, repeated pairs aside)
        for (uint64_t i = beg + lane; i < end; i += 64) {
            const uint64_t e = ent[i];
            const uint32_t n = ENT_ALT(e) + ENT_REF(e);
            if (n <= (uint32_t)DM_MOM_SMALL) atomicAdd(&hist[(uint64_t)ENT_IDX(e) * LMOM_ROW + n], 1u);
        }
    }
}

// far list, count: cnt[row] = the row's entries with a total above DM_MOM_SMALL (cnt[n_rows] is the scan's trailing zero)
__global__ __launch_bounds__(LMOM_BLOCK) void k_lm_far_count(uint64_t n_rows, const uint64_t *__restrict__ row_ptr,
                                                             const uint64_t *__restrict__ ent, uint64_t *__restrict__ cnt)
{
    const int lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t)blockIdx.x * LMOM_WAVES + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * LMOM_WAVES;
    for (uint64_t row = wave0; row < n_rows; row += nwaves) {
        const uint64_t beg = row_ptr[row], end = row_ptr[row + 1];
        uint32_t k = 0;
        for (uint64_t i = beg + lane; i < end; i += 64) {
            const uint64_t e = ent[i];
            k += ENT_ALT(e) + ENT_REF(e) > (uint32_t)DM_MOM_SMALL ? 1u : 0u;
        }
        k = wave_sum_u32(k);
        if (lane == 0) cnt[row] = k;
    }
}

// far list, fill: the row's far entries from pos[row] on, in row order (ballot prefix per 64-entry step)
__global__ __launch_bounds__(LMOM_BLOCK) void k_lm_far_fill(uint64_t n_rows, const uint64_t *__restrict__ row_ptr,
                                                            const uint64_t *__restrict__ ent, const uint64_t *__restrict__ pos,
                                                            uint32_t *__restrict__ key, uint64_t *__restrict__ val)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    const uint64_t wave0 = (uint64_t)blockIdx.x * LMOM_WAVES + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * LMOM_WAVES;
    for (uint64_t row = wave0; row < n_rows; row += nwaves) {
        const uint64_t beg = row_ptr[row], end = row_ptr[row + 1];
        uint64_t at = pos[row];
        if (pos[row + 1] == at) continue;  // (wave-uniform)
        for (uint64_t i0 = beg; i0 < end; i0 += 64) {  // (wave-uniform bounds: the whole wave takes part in the ballot)
            const bool in = i0 + lane < end;
            const uint64_t e = in ? ent[i0 + lane] : 0ull;
            const uint32_t n = ENT_ALT(e) + ENT_REF(e);
            const bool far = n > (uint32_t)DM_MOM_SMALL;
            const unsigned long long m = __ballot(far);
            if (far) {
                const uint64_t o = at + (uint64_t)__popcll(m & below);
                key[o] = ENT_IDX(e);
                val[o] = (row << 32) | (uint64_t)n;  // local cell, total (at most 2 * 65535)
            }
            at += (uint64_t)__popcll(m);
        }
    }
}

// ptr[l] = the first position of the sorted keys that holds a locus >= l; ptr[L] = m.  Thread i fills the loci in
// (key[i - 1], key[i]] (from 0 for i = 0, up to L for i = m).
__global__ __launch_bounds__(256) void k_lm_far_ptr(uint64_t m, uint64_t L, const uint32_t *__restrict__ key, uint64_t *__restrict__ ptr)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > m) return;
    const uint64_t a = i == 0 ? 0 : (uint64_t)key[i - 1] + 1;
    uint64_t b = i == m ? L + 1 : (uint64_t)key[i] + 1;
    if (b > L + 1) b = L + 1;
    for (uint64_t l = a; l < b; l++) ptr[l] = i;
}

// out: [4][L] = expected minority, expected majority, variance minority, variance majority
__global__ __launch_bounds__(LMOM_BLOCK) void k_lm_finalize(uint64_t L, const double2 *__restrict__ ab,
                                                            const uint32_t *__restrict__ hist_all, const uint32_t *__restrict__ hist_min,
                                                            const uint64_t *__restrict__ far_ptr, const uint64_t *__restrict__ far_ent,
                                                            const uint8_t *__restrict__ flags, const double *__restrict__ lf_g,
                                                            double *__restrict__ out)
{
    __shared__ double lf[LF_TABLE_N];
    for (int i = threadIdx.x; i < LF_TABLE_N; i += LMOM_BLOCK) lf[i] = lf_g[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t)blockIdx.x * LMOM_WAVES + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * LMOM_WAVES;
    for (uint64_t l = wave0; l < L; l += nwaves) {
        const double2 p = ab[l];
        if (p.x < 0.0) {  // a masked locus has no PMFData (main.rs:556); wave-uniform
            if (lane < 4) out[(uint64_t)lane * L + l] = 0.0;
            continue;
        }
        // the table's share: lane n - 1 holds E(n), V(n) and the two counts of the total n
        double e = 0.0, v = 0.0;
        uint32_t c_all = 0, c_min = 0;
        if (lane < DM_MOM_SMALL) {
            const uint32_t n = (uint32_t)lane + 1u;
            dm_pmf_moments_small(p.x, p.y, n, true, &e, &v);
            c_all = hist_all[l * LMOM_ROW + n];
            c_min = hist_min[l * LMOM_ROW + n];
        }
        const double d_min = (double)c_min, d_maj = (double)(c_all - c_min);
        const double pe_min = __dmul_rn(d_min, e), pe_maj = __dmul_rn(d_maj, e);
        const double pv_min = __dmul_rn(d_min, v), pv_maj = __dmul_rn(d_maj, v);
        double e_min = 0.0, e_maj = 0.0, v_min = 0.0, v_maj = 0.0;  // every lane forms the same four sums
#pragma unroll
        for (int i = 0; i < DM_MOM_SMALL; i++) {
            e_min = __dadd_rn(e_min, __shfl(pe_min, i, 64));
            e_maj = __dadd_rn(e_maj, __shfl(pe_maj, i, 64));
            v_min = __dadd_rn(v_min, __shfl(pv_min, i, 64));
            v_maj = __dadd_rn(v_maj, __shfl(pv_maj, i, 64));
        }
        // the totals above the table, in list order: ascending cell, a repeated pair in row order
        const uint64_t fb = far_ptr[l], fe = far_ptr[l + 1];
        for (uint64_t j = fb; j < fe; j++) {
            const uint64_t f = far_ent[j];
            double ef = 0.0, vf = 0.0;
            dm_pmf_moments_wave(lf, p.x, p.y, (uint32_t)f, lane, true, &ef, &vf);
            if (flags[f >> 32]) {
                e_min = __dadd_rn(e_min, ef);
                v_min = __dadd_rn(v_min, vf);
            } else {
                e_maj = __dadd_rn(e_maj, ef);
                v_maj = __dadd_rn(v_maj, vf);
            }
        }
        if (lane == 0) {
            out[l] = e_min;
            out[L + l] = e_maj;
            out[2 * L + l] = v_min;
            out[3 * L + l] = v_maj;
        }
    }
}

static inline unsigned lm_grid(uint64_t n, uint64_t per_block, uint64_t cap)
{
    uint64_t g = (n + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (unsigned)g;
}

static cellector_status lm_check(cellector_ctx *c, const char *what)
{
    // the counters are 32-bit: a locus cannot have more entries than the shard
    if (c->nnz >= (1ull << 32))
        return ctx_fail(c, CELLECTOR_EINVAL, "%s: %llu entries on this shard, the locus histograms count in 32 bits (below 2^32 entries)", what,
                        (unsigned long long)c->nnz);
    return CELLECTOR_OK;
}

static void lm_launch_count(cellector_ctx *c, const uint8_t *flags, uint32_t *hist)
{
    hipLaunchKernelGGL(k_lm_count, dim3(lm_grid(c->nloc, LMOM_WAVES, (uint64_t)c->n_cu * 16)), dim3(LMOM_BLOCK), 0, c->stream, c->nloc,
                       c->csr_ptr.get(), c->csr_ent.get(), flags, hist);
}

// The all-cells histogram and the far list of this matrix, made on first use (cache: dropped with CtxBuilt).
static cellector_status lm_static(cellector_ctx *c)
{
    if (c->lm_static_ready) return CELLECTOR_OK;
    const uint64_t L = c->L, n = c->nloc;
    const unsigned rows_grid = lm_grid(n, LMOM_WAVES, (uint64_t)c->n_cu * 16);
    DevBuf<uint32_t> hist, key, key_o;
    DevBuf<uint64_t> pos, val, far_ent, far_ptr;
    CHK(dev_alloc(c, &hist, L * LMOM_ROW));
    CHK(dev_alloc(c, &pos, n + 1));
    HIPCHK(c, hipMemsetAsync(hist, 0, (L * LMOM_ROW ? L * LMOM_ROW : 1) * sizeof(uint32_t), c->stream));
    HIPCHK(c, hipMemsetAsync(pos, 0, (n + 1) * sizeof(uint64_t), c->stream));
    lm_launch_count(c, nullptr, hist);
    hipLaunchKernelGGL(k_lm_far_count, dim3(rows_grid), dim3(LMOM_BLOCK), 0, c->stream, n, c->csr_ptr.get(), c->csr_ent.get(), pos.get());
    HIPCHK(c, hipGetLastError());
    uint64_t m = 0;
    CHK(dev_exclusive_scan_u64(c, pos, n + 1, &m));
    CHK(dev_alloc(c, &key, m)); CHK(dev_alloc(c, &key_o, m)); CHK(dev_alloc(c, &val, m));
    CHK(dev_alloc(c, &far_ent, m)); CHK(dev_alloc(c, &far_ptr, L + 1));
    if (m) {
        hipLaunchKernelGGL(k_lm_far_fill, dim3(rows_grid), dim3(LMOM_BLOCK), 0, c->stream, n, c->csr_ptr.get(), c->csr_ent.get(),
                           pos.get(), key.get(), val.get());
        HIPCHK(c, hipGetLastError());
        int bits = 1;
        while (bits < 32 && (1ull << bits) < L) bits++;
        CHK(dev_sort_pairs_u32_u64(c, key, key_o, val, far_ent, m, bits));  // (stable: ascending cell inside a locus)
    }
    hipLaunchKernelGGL(k_lm_far_ptr, dim3(lm_grid(m + 1, 256, 0x7fffffffu)), dim3(256), 0, c->stream, m, L, key_o.get(), far_ptr.get());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (the scratch goes)
    c->lm_hist_all = std::move(hist);
    c->lm_far_ent = std::move(far_ent);
    c->lm_far_ptr = std::move(far_ptr);
    c->lm_far_n = m;
    c->lm_static_ready = true;
    return CELLECTOR_OK;
}

// the minority's histogram under flags, then the four sums under ab into out [4][L]
static cellector_status lm_launch(cellector_ctx *c, const double2 *ab, const uint8_t *flags, uint32_t *hist_min, double *out)
{
    const uint64_t L = c->L;
    HIPCHK(c, hipMemsetAsync(hist_min, 0, L * LMOM_ROW * sizeof(uint32_t), c->stream));
    lm_launch_count(c, flags, hist_min);
    hipLaunchKernelGGL(k_lm_finalize, dim3(lm_grid(L, LMOM_WAVES, (uint64_t)c->n_cu * 16)), dim3(LMOM_BLOCK), 0, c->stream, L, ab,
                       (const uint32_t *)c->lm_hist_all.get(), (const uint32_t *)hist_min, (const uint64_t *)c->lm_far_ptr.get(),
                       (const uint64_t *)c->lm_far_ent.get(), flags, (const double *)c->lf.get(), out);
    HIPCHK(c, hipGetLastError());
    return CELLECTOR_OK;
}

// The loop's pass (cellector_em_threshold, behind the locus pass; option locus_moments): c->lm_out under the iteration's
// alpha/beta and mask (c->ab: the next iteration's table kernel has not rewritten it yet) and the NEW exclusion set (flags_new:
// em_finish has not swapped it in yet) — the inputs of main.rs:343.  The buffers are made on first use.
cellector_status launch_locus_moments(cellector_ctx *c)
{
    if (c->L == 0) return CELLECTOR_OK;
    CHK(lm_check(c, "locus_moments"));
    if (!c->lm_out) {
        CHK(dev_alloc(c, &c->lm_out, 4 * c->L));
        CHK(dev_alloc(c, &c->lm_hist_min, c->L * LMOM_ROW));
    }
    CHK(lm_static(c));
    timer_begin(c, CELLECTOR_K_LOCUS_MOM);
    CHK(lm_launch(c, c->ab, c->flags_new, c->lm_hist_min, c->lm_out));
    timer_end(c, CELLECTOR_K_LOCUS_MOM);
    return CELLECTOR_OK;
}

// The call behind cellector_locus_moments: scratch of its own for alpha/beta, the flags, the minority's histogram and the
// outputs; the ctx keeps at most the static cache.
cellector_status locus_moments_run(cellector_ctx *c, const double *alpha, const double *beta, const uint8_t *mask, const uint8_t *flags,
                                   double *exp_min, double *exp_maj, double *var_min, double *var_maj)
{
    const uint64_t L = c->L, n = c->nloc;
    if (L == 0) return CELLECTOR_OK;
    CHK(lm_check(c, "locus_moments"));
    // alpha/beta of this call, a masked locus marked by alpha = -1 as in the passes' own array (k_ab_from_arrays)
    std::vector<double2> h_ab(L);
    for (uint64_t l = 0; l < L; l++) h_ab[l] = mask && !mask[l] ? make_double2(-1.0, -1.0) : make_double2(alpha[l], beta[l]);
    DevBuf<double2> d_ab;
    DevBuf<uint8_t> d_flags;
    DevBuf<uint32_t> d_hist;
    DevBuf<double> d_out;
    CHK(dev_alloc(c, &d_ab, L));
    CHK(dev_alloc(c, &d_flags, n));
    CHK(dev_alloc(c, &d_hist, L * LMOM_ROW));
    CHK(dev_alloc(c, &d_out, 4 * L));
    CHK(lm_static(c));
    HIPCHK(c, hipMemcpyAsync(d_ab, h_ab.data(), L * sizeof(double2), hipMemcpyHostToDevice, c->stream));
    if (n) HIPCHK(c, hipMemcpyAsync(d_flags, flags, n, hipMemcpyHostToDevice, c->stream));
    CHK(lm_launch(c, d_ab, d_flags, d_hist, d_out));
    double *const h_out[4] = {exp_min, exp_maj, var_min, var_maj};
    for (int k = 0; k < 4; k++)
        if (h_out[k]) HIPCHK(c, hipMemcpyAsync(h_out[k], d_out + (uint64_t)k * L, L * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CELLECTOR_OK;
}

// The call behind cellector_locus_total_counts: out [L][19], the histogram of the flagged cells (null: all cells) and, in slot
// 18, their entries in the far list.
cellector_status locus_total_counts_run(cellector_ctx *c, const uint8_t *flags, uint32_t *out)
{
    const uint64_t L = c->L, n = c->nloc;
    if (L == 0) return CELLECTOR_OK;
    CHK(lm_check(c, "locus_total_counts"));
    CHK(lm_static(c));
    std::vector<uint32_t> h(L * LMOM_ROW);
    if (flags) {
        DevBuf<uint8_t> d_flags;
        DevBuf<uint32_t> d_hist;
        CHK(dev_alloc(c, &d_flags, n));
        CHK(dev_alloc(c, &d_hist, L * LMOM_ROW));
        if (n) HIPCHK(c, hipMemcpyAsync(d_flags, flags, n, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(d_hist, 0, L * LMOM_ROW * sizeof(uint32_t), c->stream));
        lm_launch_count(c, d_flags, d_hist);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(h.data(), d_hist, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    } else {
        HIPCHK(c, hipMemcpyAsync(h.data(), c->lm_hist_all, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    }
    // slot 18 from the far list itself, the segments the finalize walks
    std::vector<uint64_t> fp(L + 1), fe(c->lm_far_n);
    HIPCHK(c, hipMemcpyAsync(fp.data(), c->lm_far_ptr, (L + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (c->lm_far_n) HIPCHK(c, hipMemcpyAsync(fe.data(), c->lm_far_ent, c->lm_far_n * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (uint64_t l = 0; l < L; l++) {
        for (int k = 0; k < LMOM_ROW; k++) out[l * (LMOM_ROW + 1) + k] = h[l * LMOM_ROW + k];
        uint32_t far = 0;
        for (uint64_t j = fp[l]; j < fp[l + 1]; j++) far += !flags || flags[fe[j] >> 32] ? 1u : 0u;
        out[l * (LMOM_ROW + 1) + LMOM_ROW] = far;
    }
    return CELLECTOR_OK;
}
