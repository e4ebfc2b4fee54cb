// expected_log_variances, the fourth per-cell vector of get_cell_log_likelihoods (main.rs:541-591, :587): the sum over a cell's
// entries at used loci of the variance of stats.rs:23-28, and the z-score the reference's author wrote next to the normalisation
// that ships (main.rs:316-318).  One streaming pass over the by-cell CSR, which both engines keep, so it serves both.
//
// Per pass: a table of the variance for the totals 0..DM_MOM_SMALL per used locus with a compact copy of the totals 1..4
// (k_var_tables), then a wave per row
// (k_cell_variance): an entry whose total the table covers costs one 8-byte gather; the few larger ones are handed to the whole
// wave (dm_pmf_moments_wave), one after the other, in a second walk over the rows that have any.  A lane adds its table terms
// in the row's order, then its larger entries' in the row's order, and the lanes are reduced by wave_sum, so a cell's sum
// depends on its row alone: not on the shard the cell is in, nor on engine 2's tile order.
#include "ctx.h"
#include "device_math.h"

#define CV_WAVES 4
#define CV_BLOCK (CV_WAVES * 64)
#define CV_STEPS 4  // 64-entry steps of a row whose loads are issued together
#define CV_ROW (DM_MOM_SMALL + 1)  // doubles per locus of the table: totals 0..17

// row[n] = V(alpha_l, beta_l, n) by dm_pmf_moments_small, the arithmetic cellector_cell_pmfs uses for these totals (same bits);
// a masked locus (alpha < 0: k_alpha_beta, k_ab_from_arrays, k_build_tables) gets zeros, so the cell pass gathers no mask.
// The totals 1..4 (99 % of the entries at shallow coverage) also go into a compact copy, 32 bytes per locus: gathered from the
// 144-byte rows every such entry pulls a cache line of its own (26 MB of lines at 200k loci against 4 MB of L2 per XCD), from the
// copy four loci share a line (6.4 MB).
#define CV_HOT 4
__global__ __launch_bounds__(256) void k_var_tables(uint64_t L, const double2 *__restrict__ ab, double *__restrict__ vt,
                                                    double *__restrict__ hot)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= L * CV_ROW) return;
    const uint64_t l = t / CV_ROW;
    const uint32_t n = (uint32_t)(t % CV_ROW);
    const double2 p = ab[l];
    double e = 0.0, v = 0.0;
    if (p.x >= 0.0 && n > 0) dm_pmf_moments_small(p.x, p.y, n, true, &e, &v);
    vt[t] = v;
    if (n >= 1 && n <= CV_HOT) hot[l * CV_HOT + (n - 1)] = v;
}

__global__ __launch_bounds__(CV_BLOCK) void k_cell_variance(uint64_t n_rows, const uint64_t *__restrict__ row_ptr,
                                                            const uint64_t *__restrict__ ent, const double2 *__restrict__ ab,
                                                            const double *__restrict__ vt, const double *__restrict__ hot,
                                                            const double *__restrict__ lf_g, double *__restrict__ var)
{
    __shared__ double lf[LF_TABLE_N];
    for (int i = threadIdx.x; i < LF_TABLE_N; i += CV_BLOCK) lf[i] = lf_g[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t)blockIdx.x * CV_WAVES + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * CV_WAVES;
    for (uint64_t row = wave0; row < n_rows; row += nwaves) {
        const uint64_t beg = row_ptr[row], end = row_ptr[row + 1];
        double s = 0.0;
        bool any_far = false;
        // the table's share, four steps of 64 entries at a time: their loads and gathers are in flight together
        for (uint64_t i0 = beg; i0 < end; i0 += 64 * CV_STEPS) {
            uint64_t en[CV_STEPS];
#pragma unroll
            for (int u = 0; u < CV_STEPS; u++) {
                const uint64_t i = i0 + (uint64_t)u * 64 + lane;
                en[u] = i < end ? ent[i] : 0ull;  // (0: locus 0, total 0 -> the table's zero)
            }
            double v[CV_STEPS];
#pragma unroll
            for (int u = 0; u < CV_STEPS; u++) {
                const uint32_t n = ENT_ALT(en[u]) + ENT_REF(en[u]);
                const bool far = n > (uint32_t)DM_MOM_SMALL;
                any_far = any_far || far;
                const uint64_t l = ENT_IDX(en[u]);
                const uint32_t nt = far ? 0u : n;  // (slot 0 holds the zero: no address beyond the row is ever formed)
                const double *src = nt - 1u < (uint32_t)CV_HOT ? hot + l * CV_HOT + (nt - 1u) : vt + l * CV_ROW + nt;  // (the same bits)
                v[u] = *src;
            }
#pragma unroll
            for (int u = 0; u < CV_STEPS; u++) s += v[u];  // (every term is >= 0: adding a zero changes nothing)
        }
        // totals above the table (rare; none in most rows): the row once more, each such entry by the whole wave
        if (__ballot(any_far)) {
            for (uint64_t i0 = beg; i0 < end; i0 += 64) {  // (wave-uniform bounds: the whole wave takes part in the ballots)
                const bool in = i0 + lane < end;
                const uint64_t e1 = in ? ent[i0 + lane] : 0ull;
                const uint32_t n = ENT_ALT(e1) + ENT_REF(e1);
                const bool far = n > (uint32_t)DM_MOM_SMALL;
                if (!__ballot(far)) continue;
                const double2 p = far ? ab[ENT_IDX(e1)] : make_double2(-1.0, -1.0);
                unsigned long long big = __ballot(far && p.x >= 0.0);  // a masked locus adds nothing (main.rs:556)
                while (big) {
                    const int src = __ffsll((long long)big) - 1;
                    big &= big - 1ull;
                    const double al = __shfl(p.x, src, 64), be = __shfl(p.y, src, 64);
                    const uint32_t nn = (uint32_t)__shfl((int)n, src, 64);
                    double e = 0.0, v = 0.0;
                    dm_pmf_moments_wave(lf, al, be, nn, lane, true, &e, &v);
                    if (lane == src) s += v;
                }
            }
        }
        s = wave_sum(s);
        if (lane == 0) var[row] = s;
    }
}

// main.rs:317-318: (ll - expected_ll) / sqrt(expected_log_variance); main.rs:320-322's zero for a cell without used loci, and
// for one whose variance is zero.  Two rows per thread, 16-byte loads (k_cell_finalize); norm is a slice of the exchange
// buffer that starts at the shard's first cell, any parity.
__global__ __launch_bounds__(256) void k_zscore(uint64_t n_rows, const double *__restrict__ ll, const double *__restrict__ ell,
                                                const double *__restrict__ nloci, const double *__restrict__ var,
                                                double *__restrict__ norm)
{
    const uint64_t row = 2 * ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x);
    if (row >= n_rows) return;
    if (row + 1 < n_rows) {
        const double2 s = *reinterpret_cast<const double2 *>(ll + row), e = *reinterpret_cast<const double2 *>(ell + row);
        const double2 c = *reinterpret_cast<const double2 *>(nloci + row), v = *reinterpret_cast<const double2 *>(var + row);
        norm[row] = c.x > 0.0 && v.x > 0.0 ? (s.x - e.x) / sqrt(v.x) : 0.0;
        norm[row + 1] = c.y > 0.0 && v.y > 0.0 ? (s.y - e.y) / sqrt(v.y) : 0.0;
    } else {
        norm[row] = nloci[row] > 0.0 && var[row] > 0.0 ? (ll[row] - ell[row]) / sqrt(var[row]) : 0.0;
    }
}

static inline unsigned cv_grid(uint64_t n, uint64_t per_block, uint64_t cap)
{
    uint64_t g = (n + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (unsigned)g;
}

// table + row pass under ab into var [nloc]; vt: [L * (CV_ROW + CV_HOT)] scratch, the compact copy behind the rows
static cellector_status variance_launch(cellector_ctx *c, const double2 *ab, double *vt, double *var)
{
    double *hot = vt + c->L * CV_ROW;
    if (c->L)
        hipLaunchKernelGGL(k_var_tables, dim3(cv_grid(c->L * CV_ROW, 256, 0x7fffffffu)), dim3(256), 0, c->stream, c->L, ab, vt, hot);
    // rows are dealt grid-stride to a grid sized by the CUs (16 blocks each: four resident, the rest level the tail), so a block's
    // copy of the factorial table, which only the rare totals above the variance table read, is paid a few times per CU
    hipLaunchKernelGGL(k_cell_variance, dim3(cv_grid(c->nloc, CV_WAVES, (uint64_t)c->n_cu * 16)), dim3(CV_BLOCK), 0, c->stream, c->nloc,
                       c->csr_ptr.get(), c->csr_ent.get(), ab, (const double *)vt, (const double *)hot, (const double *)c->lf.get(), var);
    HIPCHK(c, hipGetLastError());
    return CELLECTOR_OK;
}

// The loop's pass (cellector_em_begin, behind the cell pass; options cell_variance / normalization): c->var under the
// iteration's alpha/beta, then, zscore, this shard's slice of NORM written over.  The two buffers are made on first use.
cellector_status launch_cell_variance(cellector_ctx *c, bool zscore, double *norm_out)
{
    if (c->nloc == 0) return CELLECTOR_OK;
    if (!c->var) {
        CHK(dev_alloc(c, &c->var, c->nloc));
        CHK(dev_alloc(c, &c->var_tab, c->L * (CV_ROW + CV_HOT)));
    }
    timer_begin(c, CELLECTOR_K_CELL_VAR);
    CHK(variance_launch(c, c->ab, c->var_tab, c->var));
    timer_end(c, CELLECTOR_K_CELL_VAR);  // (the table and the row pass: k_zscore is not inside)
    if (zscore)
        hipLaunchKernelGGL(k_zscore, dim3(cv_grid((c->nloc + 1) / 2, 256, 0x7fffffffu)), dim3(256), 0, c->stream, c->nloc, c->ll.get(),
                           c->ell.get(), c->nloci.get(), c->var.get(), norm_out);
    HIPCHK(c, hipGetLastError());
    return CELLECTOR_OK;
}

// The call behind cellector_cell_log_variances on one device: everything in scratch of its own, the ctx's state stays.
cellector_status variance_run(cellector_ctx *c, const double *alpha, const double *beta, const uint8_t *mask, double *out)
{
    if (c->nloc == 0) return CELLECTOR_OK;
    const uint64_t L = c->L;
    // alpha/beta of this call, a masked locus marked by alpha = -1 as in the passes' own array (k_ab_from_arrays)
    std::vector<double2> h_ab(L);
    for (uint64_t l = 0; l < L; l++) h_ab[l] = mask && !mask[l] ? make_double2(-1.0, -1.0) : make_double2(alpha[l], beta[l]);
    DevBuf<double2> d_ab;
    DevBuf<double> d_vt, d_var;
    CHK(dev_alloc(c, &d_ab, L));
    CHK(dev_alloc(c, &d_vt, L * (CV_ROW + CV_HOT)));
    CHK(dev_alloc(c, &d_var, c->nloc));
    HIPCHK(c, hipMemcpyAsync(d_ab, h_ab.data(), L * sizeof(double2), hipMemcpyHostToDevice, c->stream));
    CHK(variance_launch(c, d_ab, d_vt, d_var));
    HIPCHK(c, hipMemcpyAsync(out, d_var, c->nloc * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CELLECTOR_OK;
}
