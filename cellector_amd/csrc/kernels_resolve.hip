// Option resolve_ties: the cells next to an order statistic or the threshold, evaluated with the reference's arithmetic.
//
// The default cell pass evaluates log_beta_binomial_pmf as an exact product ratio (device_math.h), more accurate than the
// reference's ln_gamma differences (stats.rs:41-53) but not the same bits: a normalised LL differs from the reference's by
// at most e = near_rel * max(1, |v|) (cellector_ingest_finish).  Between select_threshold and k_flag (all on c->stream, no
// host round trip):
//   k_res_mark    one pass over the keys: the cells within 2 e_t of one of the six order statistics v_t (mode 2: every cell)
//                 into a candidate list (wave-aggregated atomics), their device keys kept beside it;
//   k_res_eval    one workgroup per candidate (persistent grid, the count read on the device): the terms of the row's entries
//                 at used loci in parallel (ref_log.h: the C library's log, statrs' Lanczos ln_gamma), added strictly left to
//                 right in FILE order (res_ent: the by-cell CSR's rows in the order their lines were read, built at ingest
//                 when the option is set; the CSR itself holds a row by ascending locus) — staged in LDS, summed by one
//                 thread — divided by the used-locus
//                 count; the reference's LL and key overwrite the cell's ll and key;
//   select_threshold again over the corrected keys: the reference's order statistics, median, iqr and threshold (DESIGN §5:
//                 a cell outside band t keeps its side of the reference's t-th value, so the corrected keys have the same
//                 t-th value as the reference's);
//   k_res_mark_thr the cells within 2 e_T of the reference's threshold T not evaluated yet, then k_res_eval over them;
//   k_res_report  counts for cellector_iter_resolution.
// k_flag then runs unchanged on the corrected keys and threshold.
#include "ctx.h"
#include "device_math.h"
#include "ref_log.h"

#define RES_THREADS 256
#define RES_EVAL_THREADS 1024
#define RES_EVAL_GRID 256  // workgroups of the persistent evaluation kernel

// res_cnt slots (u32)
enum { RC_BAND = 0 /* candidates of the six order-statistic bands */, RC_THR = 1 /* ... of the threshold band after them */,
       RC_FLIPS = 2 /* flags that differ from the device keys and threshold alone */, RC_CHANGED = 3 /* bits: median, iqr, thr */ };

__device__ __forceinline__ bool res_near(double k, double v, double near_rel)
{
    return fabs(k - v) <= 2.0 * near_rel * fmax(1.0, fabs(v));
}

// wave-aggregated append of the lanes with `in` to list[base + ...]; returns nothing, bumps *cnt once per wave
__device__ __forceinline__ void res_append(bool in, uint32_t id, double key, uint32_t *cnt, uint32_t base, uint32_t *cand,
                                           double *cand_key)
{
    const unsigned long long m = __ballot(in);
    if (!m) return;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)m) - 1;
    uint32_t pos = 0;
    if (lane == leader) pos = atomicAdd(cnt, (uint32_t)__popcll(m));
    pos = __shfl(pos, leader, 64);
    if (in) {
        const uint32_t j = base + pos + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        cand[j] = id;
        cand_key[j] = key;
    }
}

__global__ __launch_bounds__(RES_THREADS) void k_res_mark(uint64_t n, const double *__restrict__ keys, const double *__restrict__ sel,
                                                          double near_rel, int mode, uint8_t *__restrict__ done,
                                                          uint32_t *__restrict__ cand, double *__restrict__ cand_key,
                                                          uint32_t *__restrict__ cnt, double *__restrict__ dev_sum)
{
    double v[SEL_T];
#pragma unroll
    for (int t = 0; t < SEL_T; t++) v[t] = sel[t];
    if (blockIdx.x == 0 && threadIdx.x < 3) dev_sum[threadIdx.x] = sel[8 + threadIdx.x];  // the device's median, iqr, threshold
    const uint64_t stride = (uint64_t)gridDim.x * RES_THREADS;
    const uint64_t n_round = (n + 63) / 64 * 64;  // whole waves take part in the ballot
    for (uint64_t i = (uint64_t)blockIdx.x * RES_THREADS + threadIdx.x; i < n_round; i += stride) {
        bool in = false;
        double k = 0.0;
        if (i < n) {
            k = keys[i];
            in = mode == 2;
#pragma unroll
            for (int t = 0; t < SEL_T; t++) in = in || res_near(k, v[t], near_rel);
            done[i] = in ? 1 : 0;
        }
        res_append(in, (uint32_t)i, k, &cnt[RC_BAND], 0u, cand, cand_key);
    }
}

__global__ __launch_bounds__(RES_THREADS) void k_res_mark_thr(uint64_t n, const double *__restrict__ keys, const double *__restrict__ sel,
                                                              const double *__restrict__ dev_sum, double near_rel,
                                                              const uint8_t *__restrict__ done, uint32_t *__restrict__ cand,
                                                              double *__restrict__ cand_key, uint32_t *__restrict__ cnt)
{
    const double thr = sel[10], thr_dev = dev_sum[2];
    const uint32_t base = cnt[RC_BAND];
    const uint64_t stride = (uint64_t)gridDim.x * RES_THREADS;
    const uint64_t n_round = (n + 63) / 64 * 64;
    uint32_t flips = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * RES_THREADS + threadIdx.x; i < n_round; i += stride) {
        bool in = false;
        double k = 0.0;
        if (i < n && !done[i]) {
            k = keys[i];
            in = res_near(k, thr, near_rel);
            // a cell left as it is: its flag against the device's threshold and against the reference's
            if (!in) flips += ((k < thr_dev) != (k < thr)) ? 1u : 0u;
        }
        res_append(in, (uint32_t)i, k, &cnt[RC_THR], base, cand, cand_key);
    }
    flips = wave_sum_u32(flips);
    if ((threadIdx.x & 63) == 0 && flips) atomicAdd(&cnt[RC_FLIPS], flips);
}

// one workgroup per candidate of the list slice [first, last) (read from cnt on the device): the threads evaluate a chunk of
// RES_EVAL_THREADS terms of the row into LDS, then thread 0 adds them one after the other (a row of 2000 entries is two chunks)
__global__ __launch_bounds__(RES_EVAL_THREADS) void k_res_eval(int which /*0: the order-statistic bands, 1: the threshold band*/,
                                                               const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ cand,
                                                               const uint64_t *__restrict__ row_ptr, const uint64_t *__restrict__ ent,
                                                               const double2 *__restrict__ ab, const double *__restrict__ lf_g,
                                                               double *__restrict__ ll, double *__restrict__ keys)
{
    __shared__ double lf[LF_TABLE_N];
    __shared__ double term[RES_EVAL_THREADS];
    __shared__ uint8_t used[RES_EVAL_THREADS];
    for (int i = threadIdx.x; i < LF_TABLE_N; i += RES_EVAL_THREADS) lf[i] = lf_g[i];
    __syncthreads();
    const uint32_t first = which == 0 ? 0u : cnt[RC_BAND];
    const uint32_t last = which == 0 ? cnt[RC_BAND] : cnt[RC_BAND] + cnt[RC_THR];
    for (uint32_t j = first + blockIdx.x; j < last; j += gridDim.x) {
        const uint32_t row = cand[j];
        const uint64_t beg = row_ptr[row], end = row_ptr[row + 1];
        double s = 0.0;  // main.rs:541-591: log_likelihood += log_pmf, in the row's order (thread 0)
        uint32_t n_used = 0;
        for (uint64_t c0 = beg; c0 < end; c0 += RES_EVAL_THREADS) {
            const uint64_t i = c0 + threadIdx.x;
            bool u = false;
            if (i < end) {
                const uint64_t en = ent[i];
                const double2 p = ab[ENT_IDX(en)];
                u = p.x >= 0.0;  // (masked loci carry alpha = -1)
                term[threadIdx.x] = u ? ref_log_bb_pmf(lf, p.x, p.y, ENT_ALT(en), ENT_REF(en)) : 0.0;
            }
            used[threadIdx.x] = u ? 1 : 0;
            __syncthreads();
            if (threadIdx.x == 0) {
                const int nk = (int)min((uint64_t)RES_EVAL_THREADS, end - c0);
                // strictly left to right; a select instead of a branch, so that the LDS reads run ahead of the add chain
#pragma unroll 16
                for (int k = 0; k < nk; k++) {
                    const double t = term[k];
                    const bool u = used[k] != 0;
                    const double s2 = s + t;
                    s = u ? s2 : s;
                    n_used += u ? 1u : 0u;
                }
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            ll[row] = s;
            keys[row] = n_used > 0 ? s / (double)n_used : 0.0;  // main.rs:315-322
        }
    }
}

__global__ __launch_bounds__(RES_THREADS) void k_res_report(const uint32_t *__restrict__ cand, const double *__restrict__ cand_key,
                                                            const double *__restrict__ keys, const double *__restrict__ sel,
                                                            const double *__restrict__ dev_sum, uint32_t *__restrict__ cnt)
{
    __shared__ uint32_t s_flips[RES_THREADS / 64];
    const uint32_t n = cnt[RC_BAND] + cnt[RC_THR];
    const double thr = sel[10], thr_dev = dev_sum[2];
    uint32_t flips = 0;
    for (uint32_t j = threadIdx.x; j < n; j += RES_THREADS)
        flips += ((cand_key[j] < thr_dev) != (keys[cand[j]] < thr)) ? 1u : 0u;
    flips = wave_sum_u32(flips);
    if ((threadIdx.x & 63) == 0) s_flips[threadIdx.x >> 6] = flips;
    __syncthreads();
    if (threadIdx.x != 0) return;
    uint32_t tot = 0;
    for (int w = 0; w < RES_THREADS / 64; w++) tot += s_flips[w];
    cnt[RC_FLIPS] += tot;
    uint32_t changed = 0;
    for (int t = 0; t < 3; t++)
        if (__double_as_longlong(sel[8 + t]) != __double_as_longlong(dev_sum[t])) changed |= 1u << t;
    cnt[RC_CHANGED] = changed;
}

// ---- each cell's entries in file order (ingest, option set): the reference adds a cell's terms as its lines were read -------
__global__ void k_res_used(uint64_t n, const uint32_t *__restrict__ locus, const uint64_t *__restrict__ to_used,
                           uint64_t *__restrict__ pos)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) pos[i] = to_used[locus[i]] != ~0ull ? 1u : 0u;
    else if (i == n) pos[n] = 0;
}
__global__ void k_res_scatter(uint64_t n, const uint32_t *__restrict__ locus, const uint32_t *__restrict__ cell,
                              const uint16_t *__restrict__ alt, const uint16_t *__restrict__ ref,
                              const uint64_t *__restrict__ to_used, const uint64_t *__restrict__ pos, uint32_t *__restrict__ key,
                              uint64_t *__restrict__ val)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t u = to_used[locus[i]];
    if (u == ~0ull) return;
    key[pos[i]] = cell[i];
    val[pos[i]] = u | ((uint64_t)alt[i] << 32) | ((uint64_t)ref[i] << 48);  // packed like csr_ent
}

// the staged entries (file order) at used loci, stably sorted by cell alone: res_ent has the layout of csr_ent (same row
// pointers) with every row in file order.  Called by ingest_build once to_used is final, before the entries are sorted by locus.
cellector_status resolve_build_file_order(cellector_ctx *c)
{
    c->res_ent.reset();
    const uint64_t n = c->coo.n;
    DevBuf<uint64_t> pos, val;
    DevBuf<uint32_t> key, key_o;
    CHK(dev_alloc(c, &pos, n + 1));
    hipLaunchKernelGGL(k_res_used, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, c->stream, n, c->coo.locus, c->to_used, pos);
    HIPCHK(c, hipGetLastError());
    uint64_t m = 0;
    CHK(dev_exclusive_scan_u64(c, pos, n + 1, &m));
    CHK(dev_alloc(c, &key, m)); CHK(dev_alloc(c, &key_o, m)); CHK(dev_alloc(c, &val, m)); CHK(dev_alloc(c, &c->res_ent, m));
    if (n)
        hipLaunchKernelGGL(k_res_scatter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, n, c->coo.locus, c->coo.cell,
                           c->coo.alt, c->coo.ref, c->to_used, pos, key, val);
    HIPCHK(c, hipGetLastError());
    int bits = 1;
    while (bits < 32 && (1ull << bits) < c->nloc) bits++;
    CHK(dev_sort_pairs_u32_u64(c, key, key_o, val, c->res_ent, m, bits));  // (stable: file order inside a cell)
    c->res_nnz = m;
    return CELLECTOR_OK;
}

static inline unsigned res_grid(uint64_t n)
{
    uint64_t g = (n + RES_THREADS - 1) / RES_THREADS;
    return (unsigned)(g < 1 ? 1 : (g > 1024 ? 1024 : g));
}

// after select_threshold over this ctx's keys (single device: cell_begin = 0, nloc = total_cells), before launch_flag
cellector_status resolve_ties(cellector_ctx *c, double iqr_multiple)
{
    const uint64_t n = c->nloc;
    if (c->nnz && (!c->res_ent || c->res_nnz != c->nnz))
        return ctx_fail(c, CELLECTOR_EINVAL, "resolve_ties needs every cell's entries in file order, kept by an ingest that ran with "
                                             "the option set: set it before the ingest");
    if (c->res_n != n) {
        c->res_cand.reset(); c->res_key.reset(); c->res_done.reset();
        CHK(dev_alloc(c, &c->res_cand, n)); CHK(dev_alloc(c, &c->res_key, n)); CHK(dev_alloc(c, &c->res_done, n));
        c->res_n = n;
    }
    if (!c->res_cnt) CHK(dev_alloc(c, &c->res_cnt, 4));
    if (!c->res_dev) CHK(dev_alloc(c, &c->res_dev, 4));
    double *keys = c->x_norm + c->cell_begin;
    HIPCHK(c, hipMemsetAsync(c->res_cnt, 0, 4 * sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(k_res_mark, dim3(res_grid(n)), dim3(RES_THREADS), 0, c->stream, n, keys, c->sel_out, c->near_rel,
                       c->resolve_ties, c->res_done, c->res_cand, c->res_key, c->res_cnt, c->res_dev);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_res_eval, dim3(RES_EVAL_GRID), dim3(RES_EVAL_THREADS), 0, c->stream, 0, c->res_cnt, c->res_cand, c->csr_ptr, c->res_ent,
                       c->ab, c->lf, c->ll, keys);
    HIPCHK(c, hipGetLastError());
    CHK(select_threshold(c, c->x_norm, c->total_cells, iqr_multiple));
    hipLaunchKernelGGL(k_res_mark_thr, dim3(res_grid(n)), dim3(RES_THREADS), 0, c->stream, n, keys, c->sel_out, c->res_dev,
                       c->near_rel, c->res_done, c->res_cand, c->res_key, c->res_cnt);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_res_eval, dim3(RES_EVAL_GRID), dim3(RES_EVAL_THREADS), 0, c->stream, 1, c->res_cnt, c->res_cand, c->csr_ptr, c->res_ent,
                       c->ab, c->lf, c->ll, keys);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_res_report, dim3(1), dim3(RES_THREADS), 0, c->stream, c->res_cand, c->res_key, keys, c->sel_out,
                       c->res_dev, c->res_cnt);
    HIPCHK(c, hipGetLastError());
    return CELLECTOR_OK;
}
