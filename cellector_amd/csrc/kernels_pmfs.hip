// cellector_cell_pmfs: the reference's PMFData (main.rs:527-539) of listed cells — one record per entry of the cell at a used
// locus, as get_cell_log_likelihoods pushes them into all_pmfs (main.rs:556-575) — from the by-cell CSR, which both engines keep.
//
// A count pass under the call's mask, an exclusive scan, a fill pass.  Both give a wave to a listed cell; its lanes stride the
// row in 64-entry steps, so a step's records are compacted with a ballot prefix and keep the row's order.  Everything the call
// needs lives in scratch of its own: the ctx's alpha/beta, tables and iteration outputs are not touched.
#include "ctx.h"
#include "device_math.h"

#define PM_WAVES 4
#define PM_BLOCK (PM_WAVES * 64)

__global__ __launch_bounds__(PM_BLOCK) void k_pmf_count(uint64_t n_list, const uint32_t *__restrict__ cells,
                                                        const uint64_t *__restrict__ row_ptr, const uint64_t *__restrict__ ent,
                                                        const double2 *__restrict__ ab, uint64_t *__restrict__ cnt_out)
{
    const int lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t)blockIdx.x * PM_WAVES + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * PM_WAVES;
    for (uint64_t j = wave0; j < n_list; j += nwaves) {
        const uint32_t row = cells[j];
        const uint64_t beg = row_ptr[row], end = row_ptr[row + 1];
        uint32_t cnt = 0;
        for (uint64_t i = beg + lane; i < end; i += 64) cnt += ab[ENT_IDX(ent[i])].x >= 0.0 ? 1u : 0u;
        cnt = wave_sum_u32(cnt);
        if (lane == 0) cnt_out[j] = cnt;
    }
}

struct PmfColumns {  // device arrays of [records] each; a null column is not computed
    uint32_t *locus, *alt, *ref;
    double *lp, *e, *v;
};

__global__ __launch_bounds__(PM_BLOCK) void k_pmf_fill(uint64_t n_list, const uint32_t *__restrict__ cells,
                                                       const uint64_t *__restrict__ rec_ptr, const uint64_t *__restrict__ row_ptr,
                                                       const uint64_t *__restrict__ ent, const double2 *__restrict__ ab,
                                                       const double *__restrict__ lf_g, PmfColumns out)
{
    __shared__ double lf[LF_TABLE_N];
    for (int i = threadIdx.x; i < LF_TABLE_N; i += PM_BLOCK) lf[i] = lf_g[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    const bool moments = out.e != nullptr || out.v != nullptr, want_v = out.v != nullptr;
    const uint64_t wave0 = (uint64_t)blockIdx.x * PM_WAVES + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * PM_WAVES;
    for (uint64_t j = wave0; j < n_list; j += nwaves) {
        const uint32_t row = cells[j];
        const uint64_t beg = row_ptr[row], end = row_ptr[row + 1];
        uint64_t pos = rec_ptr[j];
        for (uint64_t i0 = beg; i0 < end; i0 += 64) {  // (wave-uniform bounds: the whole wave takes part in the ballots)
            const bool in = i0 + lane < end;
            const uint64_t en = in ? ent[i0 + lane] : 0ull;
            const double2 p = in ? ab[ENT_IDX(en)] : make_double2(-1.0, -1.0);
            const bool live = in && p.x >= 0.0;  // else a masked locus: no PMFData (main.rs:556)
            const unsigned long long m = __ballot(live);
            const uint64_t at = pos + (uint64_t)__popcll(m & below);
            const uint32_t a = ENT_ALT(en), r = ENT_REF(en), n = a + r;
            if (live) {
                if (out.locus) out.locus[at] = ENT_IDX(en);
                if (out.alt) out.alt[at] = a;
                if (out.ref) out.ref[at] = r;
                if (out.lp) out.lp[at] = dm_log_bb_pmf(lf, p.x, p.y, a, r);
            }
            if (moments) {
                const bool small = n <= (uint32_t)DM_MOM_SMALL;
                if (live && small) {
                    double e = 0.0, v = 0.0;
                    dm_pmf_moments_small(p.x, p.y, n, want_v, &e, &v);
                    if (out.e) out.e[at] = e;
                    if (want_v) out.v[at] = v;
                }
                // the larger totals one after the other, each by the whole wave: its k loop is O(total)
                unsigned long long big = __ballot(live && !small);
                while (big) {
                    const int src = __ffsll((long long)big) - 1;
                    big &= big - 1ull;
                    const double al = __shfl(p.x, src, 64), be = __shfl(p.y, src, 64);
                    const uint32_t nn = (uint32_t)__shfl((int)n, src, 64);
                    double e = 0.0, v = 0.0;
                    dm_pmf_moments_wave(lf, al, be, nn, lane, want_v, &e, &v);
                    if (lane == src) {
                        if (out.e) out.e[at] = e;
                        if (want_v) out.v[at] = v;
                    }
                }
            }
            pos += (uint64_t)__popcll(m);
        }
    }
}

static inline unsigned pm_grid(uint64_t n)
{
    uint64_t g = (n + PM_WAVES - 1) / PM_WAVES;
    if (g < 1) g = 1;
    if (g > (1u << 20)) g = 1u << 20;
    return (unsigned)g;
}

// The call behind cellector_cell_pmfs on one device; the ids are validated (api_em.cpp).
cellector_status pmfs_run(cellector_ctx *c, const double *alpha, const double *beta, const uint8_t *mask, const uint32_t *cells,
                          uint64_t n_cells, uint64_t *rec_ptr, uint64_t capacity, uint32_t *locus_index, uint32_t *alt, uint32_t *ref,
                          double *log_pmf, double *expected_log_pmf, double *expected_log_variance)
{
    rec_ptr[0] = 0;
    if (n_cells == 0) return CELLECTOR_OK;
    const uint64_t L = c->L;
    // alpha/beta of this call, a masked locus marked by alpha = -1 as in the passes' own array (k_ab_from_arrays)
    std::vector<double2> h_ab(L);
    for (uint64_t l = 0; l < L; l++) h_ab[l] = mask && !mask[l] ? make_double2(-1.0, -1.0) : make_double2(alpha[l], beta[l]);
    DevBuf<double2> d_ab;
    DevBuf<uint32_t> d_cells;
    DevBuf<uint64_t> d_ptr;
    CHK(dev_alloc(c, &d_ab, L));
    CHK(dev_alloc(c, &d_cells, n_cells));
    CHK(dev_alloc(c, &d_ptr, n_cells + 1));
    HIPCHK(c, hipMemcpyAsync(d_ab, h_ab.data(), L * sizeof(double2), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_cells, cells, n_cells * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(d_ptr + n_cells, 0, sizeof(uint64_t), c->stream));
    hipLaunchKernelGGL(k_pmf_count, dim3(pm_grid(n_cells)), dim3(PM_BLOCK), 0, c->stream, n_cells, d_cells.get(), c->csr_ptr.get(),
                       c->csr_ent.get(), d_ab.get(), d_ptr.get());
    HIPCHK(c, hipGetLastError());
    uint64_t total = 0;
    CHK(dev_exclusive_scan_u64(c, d_ptr, n_cells + 1, &total));
    HIPCHK(c, hipMemcpyAsync(rec_ptr, d_ptr, (n_cells + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!locus_index && !alt && !ref && !log_pmf && !expected_log_pmf && !expected_log_variance) return CELLECTOR_OK;  // the counting call
    if (capacity < total)
        return ctx_fail(c, CELLECTOR_EINVAL, "cell_pmfs: capacity %llu is below the %llu records of the list", (unsigned long long)capacity,
                        (unsigned long long)total);
    if (total == 0) return CELLECTOR_OK;
    // device scratch for exactly the counted records, all of it before the fill pass is launched
    DevBuf<uint32_t> d_u[3];
    DevBuf<double> d_f[3];
    uint32_t *const h_u[3] = {locus_index, alt, ref};
    double *const h_f[3] = {log_pmf, expected_log_pmf, expected_log_variance};
    for (int i = 0; i < 3; i++) {
        if (h_u[i]) CHK(dev_alloc(c, &d_u[i], total));
        if (h_f[i]) CHK(dev_alloc(c, &d_f[i], total));
    }
    const PmfColumns cols = {d_u[0].get(), d_u[1].get(), d_u[2].get(), d_f[0].get(), d_f[1].get(), d_f[2].get()};
    hipLaunchKernelGGL(k_pmf_fill, dim3(pm_grid(n_cells)), dim3(PM_BLOCK), 0, c->stream, n_cells, d_cells.get(), d_ptr.get(),
                       c->csr_ptr.get(), c->csr_ent.get(), d_ab.get(), c->lf.get(), cols);
    HIPCHK(c, hipGetLastError());
    for (int i = 0; i < 3; i++) {
        if (h_u[i]) HIPCHK(c, hipMemcpyAsync(h_u[i], d_u[i], total * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        if (h_f[i]) HIPCHK(c, hipMemcpyAsync(h_f[i], d_f[i], total * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CELLECTOR_OK;
}
