// Genotype clustering without labels (cellector_cluster, cellector_cluster_e_step, cellector_cluster_m_step): a mixture of
// per-locus binomials over allele fractions fitted by soft EM, a depth-dependent temperature annealed away over a few stages, R
// random restarts run side by side.  include/cellector_ffi.h states the model completely; cellector_amd/cluster.py is its twin.
//
// The restarts are COLUMNS: column j = r K + k is cluster k of restart r, J = K R <= 64 of them.  Every per-locus quantity is a
// row of J values ([L][J] theta, [L][J][2] the two logs), every per-cell one a row of J ([cells][J] sums s and weights w).  Both
// passes put the columns on the lanes, in the shape lane_rows.h states: the restarts share the entry stream, the pointers and the
// launches (measured at cfg4, K = 3: sixteen restarts cost 7.4 E steps and 5.0 M steps of one).
//   E step  k_cluster_e  rows = cells of the by-cell CSR, per entry the double2 row of the table; tail: softmax per restart,
//                        the cell's objective terms, its depth and its entry count
//   M step  k_cluster_m  rows = loci of a by-locus list in ascending cell order, per entry a gather of the cell's w row
// The by-locus list is a stable sort of the by-cell CSR by locus (the ingest's sorter): ascending cell, file order among the
// repeats of a pair, whatever order the file had its cells in; engine 2 keeps no by-locus copy of the packed entries anyway.  It
// lives in call-owned scratch.  Nothing of the ctx is written: the EM state, its tables and its outputs stay.
#include "lane_rows.h"
#include "mix64.h"

#include <cmath>

// theta[l][j] = floor + (1 - 2 floor) u(l, j), u = (mix64(sm + (l J + j + 1) GOLD) >> 11) 2^-53, sm = mix64(seed GOLD + GOLD)
__global__ __launch_bounds__(LANE_THREADS) void k_cluster_start(uint64_t n /*L J*/, uint64_t sm, double floor, double *__restrict__ theta)
{
    const uint64_t i = (uint64_t)blockIdx.x * LANE_THREADS + threadIdx.x;
    if (i >= n) return;
    const double u = (double)(mix64(sm + (i + 1) * GOLD) >> 11) * 0x1p-53;
    const double span = 1.0 - 2.0 * floor;
    theta[i] = floor + span * u;
}

// tab[l][j] = (log theta, log(1 - theta)); a masked locus takes no part anywhere and carries (0, 0)
__global__ __launch_bounds__(LANE_THREADS) void k_cluster_tables(uint64_t n /*L J*/, uint32_t J, const double *__restrict__ theta,
                                                                 const uint8_t *__restrict__ mask /*or null*/, double2 *__restrict__ tab)
{
    const uint64_t i = (uint64_t)blockIdx.x * LANE_THREADS + threadIdx.x;
    if (i >= n) return;
    const bool used = !mask || mask[i / J] != 0;
    const double t = theta[i];
    tab[i] = used ? make_double2(log(t), log(1.0 - t)) : make_double2(0.0, 0.0);
}

// E step.  A group of JP lanes per cell, lane = column.  s = the ordered sum of (alt la + ref lb) over the row's entries at unmasked
// loci; then per restart x_k = s_k / T, m = max, den = sum exp(x_k - m) in ascending k, w = exp(x - m) / den, o = m + log(den).
// T = temp[cell], or max(1, depth / div) with the cell's own depth (div > 0), or 1.
template <int JP>
__global__ __launch_bounds__(LANE_THREADS) void k_cluster_e(uint64_t n_rows, uint32_t J, uint32_t K, const uint64_t *__restrict__ row_ptr,
                                                            const uint64_t *__restrict__ ent, const double2 *__restrict__ tab,
                                                            const uint8_t *__restrict__ mask /*or null*/,
                                                            const double *__restrict__ temp /*or null*/, double div,
                                                            double *__restrict__ s_out, double *__restrict__ w_out,
                                                            double *__restrict__ o_out /*[rows][R]*/,
                                                            unsigned long long *__restrict__ depth_out, uint32_t *__restrict__ cnt_out)
{
    const LaneGeom<JP> geo(n_rows, J);
    const int col = geo.col;
    const bool col_ok = geo.ok;
    const uint32_t R = J / K;
    for (uint64_t g = geo.wave0; g < geo.n_groups; g += geo.n_waves) {
        const uint64_t row = geo.row(g);
        const bool have = row < n_rows;
        const uint64_t beg = have ? row_ptr[row] : 0, end = have ? row_ptr[row + 1] : 0;
        double acc = 0.0;
        unsigned long long depth = 0;
        uint32_t cnt = 0;
        // the entry loop of lane_rows.h: a fix here belongs in k_donor_e, k_donor_fit, k_ambient_e, k_pair_fraction_e and k_donor_match as well
        for (uint64_t i = beg; i < end; i += LANE_AHEAD) {
            uint64_t en[LANE_AHEAD];
            double2 t[LANE_AHEAD];
            bool use[LANE_AHEAD];
#pragma unroll
            for (int q = 0; q < LANE_AHEAD; q++) {
                const bool in = i + q < end;
                en[q] = in ? ent[i + q] : 0ull;
                const uint64_t l = ENT_IDX(en[q]);
                use[q] = in && (!mask || mask[l] != 0);
                t[q] = use[q] && col_ok ? tab[l * J + col] : make_double2(0.0, 0.0);
            }
#pragma unroll
            for (int q = 0; q < LANE_AHEAD; q++) {
                if (!use[q]) continue;
                const uint32_t a = ENT_ALT(en[q]), r = ENT_REF(en[q]);
                const double pa = (double)a * t[q].x, pb = (double)r * t[q].y;
                const double term = pa + pb;
                acc = acc + term;
                depth += a + r;
                cnt++;
            }
        }
        // the tail (the restart's K lanes from base on)
        double T = 1.0;
        if (have) T = temp ? temp[row] : (div > 0.0 ? fmax(1.0, (double)depth / div) : 1.0);
        const double x = acc / T;
        const uint32_t r = col_ok ? (uint32_t)col / K : 0;
        const int base = geo.sub * JP + (int)(r * K);
        double m = -INFINITY;
        for (uint32_t k = 0; k < K; k++) m = fmax(m, __shfl(x, (base + (int)k) & 63, 64));
        double den = 0.0;
        for (uint32_t k = 0; k < K; k++) den = den + exp(__shfl(x, (base + (int)k) & 63, 64) - m);
        if (have && col_ok) {
            s_out[row * J + col] = acc;
            w_out[row * J + col] = exp(x - m) / den;
            if ((uint32_t)col == r * K) o_out[row * R + r] = m + log(den);
        }
        if (have && col == 0) {
            depth_out[row] = depth;
            cnt_out[row] = cnt;
        }
    }
}

// obj[r] = sum over the cells of o[cell][r] in a fixed order: thread t of block r adds the cells t, t + 256, ... in ascending order,
// the 256 partial sums are folded pairwise
__global__ __launch_bounds__(LANE_THREADS) void k_cluster_objective(uint64_t n, uint32_t R, const double *__restrict__ o, double *__restrict__ obj)
{
    __shared__ double sh[LANE_THREADS];
    const uint32_t r = blockIdx.x;
    double a = 0.0;
    for (uint64_t i = threadIdx.x; i < n; i += LANE_THREADS) a = a + o[i * R + r];
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int h = LANE_THREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) obj[r] = sh[0];
}

// M step.  A group of JP lanes per locus, lane = column: A = the ordered sum of w alt, T = of w (alt + ref) over the locus' entries
// in ascending cell order (a rounded product, then the add), theta = min(max((A + 1) / (T + 2), floor), 1 - floor).  A locus without
// an entry gets 1 / 2 = 0.5 by the same formula; a masked locus is not walked: A = T = 0, theta = 0.5.
template <int JP>
__global__ __launch_bounds__(LANE_THREADS) void k_cluster_m(uint64_t L, uint32_t J, const uint64_t *__restrict__ col_ptr,
                                                            const uint64_t *__restrict__ ent /*by locus, ascending cell*/,
                                                            const double *__restrict__ w /*[cells][J]*/,
                                                            const uint8_t *__restrict__ mask /*or null*/, double floor,
                                                            double *__restrict__ A_out /*or null*/, double *__restrict__ T_out /*or null*/,
                                                            double *__restrict__ theta)
{
    const LaneGeom<JP> geo(L, J);
    const int col = geo.col;
    const double ceil_ = 1.0 - floor;
    for (uint64_t g = geo.wave0; g < geo.n_groups; g += geo.n_waves) {
        const uint64_t l = geo.row(g);
        const bool have = l < L && geo.ok;
        const bool used = have && (!mask || mask[l] != 0);
        const uint64_t beg = used ? col_ptr[l] : 0, end = used ? col_ptr[l + 1] : 0;
        double A = 0.0, T = 0.0;
        for (uint64_t i = beg; i < end; i += LANE_AHEAD) {
            uint64_t en[LANE_AHEAD];
            double wv[LANE_AHEAD];
#pragma unroll
            for (int q = 0; q < LANE_AHEAD; q++) {
                const bool in = i + q < end;
                en[q] = in ? ent[i + q] : 0ull;
                wv[q] = in ? w[(uint64_t)ENT_IDX(en[q]) * J + col] : 0.0;
            }
#pragma unroll
            for (int q = 0; q < LANE_AHEAD; q++) {
                if (i + q >= end) continue;
                const uint32_t a = ENT_ALT(en[q]), r = ENT_REF(en[q]);
                const double pa = wv[q] * (double)a, pt = wv[q] * (double)(a + r);
                A = A + pa;
                T = T + pt;
            }
        }
        if (!have) continue;
        const double th = used ? fmin(fmax((A + 1.0) / (T + 2.0), floor), ceil_) : 0.5;
        if (A_out) A_out[l * J + col] = A;
        if (T_out) T_out[l * J + col] = T;
        theta[l * J + col] = th;
    }
}

// the by-cell CSR as (locus key, cell | counts) pairs, one wave per row
__global__ __launch_bounds__(LANE_THREADS) void k_cluster_split(uint64_t n_rows, const uint64_t *__restrict__ row_ptr,
                                                                const uint64_t *__restrict__ ent, uint32_t *__restrict__ key,
                                                                uint64_t *__restrict__ val)
{
    const int lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t)blockIdx.x * LANE_WAVES + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * LANE_WAVES;
    for (uint64_t row = wave0; row < n_rows; row += n_waves) {
        const uint64_t beg = row_ptr[row], end = row_ptr[row + 1];
        for (uint64_t i = beg + lane; i < end; i += 64) {
            const uint64_t en = ent[i];
            key[i] = ENT_IDX(en);
            val[i] = (en & ~0xffffffffull) | row;
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
namespace {

// the scratch of one call; alloc() makes all of it (and the by-locus list) before anything is launched
struct ClusterRun {
    cellector_ctx *c;
    uint32_t K, R, J;
    uint64_t n, L;
    DevBuf<uint64_t> bl;        // [nnz] by locus, ascending cell: cell | alt << 32 | ref << 48; its pointers are the ctx's csc_ptr
    DevBuf<double> theta, A, T; // [L][J]
    DevBuf<double2> tab;        // [L][J]
    DevBuf<double> s, w;        // [n][J]
    DevBuf<double> o, obj;      // [n][R], [R]
    DevBuf<double> temp;        // [n] a caller's temperatures
    DevBuf<unsigned long long> depth;  // [n]
    DevBuf<uint32_t> cnt;       // [n]
    LociMask mask;              // [L]
    // CELLECTOR_TIMING=1: the GPU time of the E and M kernels of a cellector_cluster call (events 0, 1 around the E launches, 2, 3 around
    // the M launch, read after the iteration's own synchronisation) and the wall time of the by-locus list, one stderr line per call
    EventMarks<4> ev;
    double ms_e = 0.0, ms_m = 0.0, s_list = 0.0;
    unsigned n_e = 0, n_m = 0;
    bool open_e = false, open_m = false;
    void collect()  // (the stream is idle)
    {
        float ms = 0.f;
        if (open_e && ev.ms(0, 1, &ms)) { ms_e += ms; n_e++; }
        if (open_m && ev.ms(2, 3, &ms)) { ms_m += ms; n_m++; }
        open_e = open_m = false;
    }

    cellector_status alloc(bool e_side, bool m_side, bool at, bool temps)
    {
        const uint64_t LJ = L * J, nJ = n * J;
        CHK(dev_alloc(c, &mask.buf, L));
        CHK(dev_alloc(c, &tab, LJ));
        CHK(dev_alloc(c, &w, nJ));
        if (m_side) {
            CHK(dev_alloc(c, &theta, LJ));
            if (at) { CHK(dev_alloc(c, &A, LJ)); CHK(dev_alloc(c, &T, LJ)); }
        }
        if (e_side) {
            CHK(dev_alloc(c, &s, nJ));
            CHK(dev_alloc(c, &o, n * R));
            CHK(dev_alloc(c, &obj, R));
            CHK(dev_alloc(c, &depth, n));
            CHK(dev_alloc(c, &cnt, n));
            if (temps) CHK(dev_alloc(c, &temp, n));
        }
        if (m_side) CHK(build_by_locus());
        return CELLECTOR_OK;
    }

    // stable sort of the CSR's entries by locus: the temporaries go when it returns, the list stays with the call
    cellector_status build_by_locus()
    {
        const uint64_t nnz = c->nnz;
        DevBuf<uint32_t> key, key_o;
        DevBuf<uint64_t> val;
        CHK(dev_alloc(c, &bl, nnz));
        CHK(dev_alloc(c, &key, nnz)); CHK(dev_alloc(c, &key_o, nnz)); CHK(dev_alloc(c, &val, nnz));
        if (!nnz || !n) return CELLECTOR_OK;
        LapTimer t;
        hipLaunchKernelGGL(k_cluster_split, dim3(lane_grid(n, LANE_WAVES, 1u << 16)), dim3(LANE_THREADS), 0, c->stream, n, c->csr_ptr.get(),
                           c->csr_ent.get(), key.get(), val.get());
        HIPCHK(c, hipGetLastError());
        int bits = 1;
        while (bits < 32 && (1ull << bits) < L) bits++;
        CHK(dev_sort_pairs_u32_u64(c, key, key_o, val, bl, nnz, bits));  // (synchronises)
        s_list = t.lap();
        return CELLECTOR_OK;
    }

    cellector_status tables()
    {
        if (!(L * J)) return CELLECTOR_OK;
        hipLaunchKernelGGL(k_cluster_tables, dim3(lane_grid(L * J, LANE_THREADS, 0x7fffffffu)), dim3(LANE_THREADS), 0, c->stream, L * J, J,
                           theta.get(), mask.get(), tab.get());
        HIPCHK(c, hipGetLastError());
        return CELLECTOR_OK;
    }

    cellector_status e_step(const double *d_temp, double div)
    {
        const int jp = lane_width(J, 2);
        ev.mark(0, c->stream);
        if (n)
            lane_dispatch<2, 64>(jp, [&](auto JP) {
                hipLaunchKernelGGL(k_cluster_e<JP>, dim3(lane_walk_grid(n, jp, c->n_cu)), dim3(LANE_THREADS), 0, c->stream, n, J, K,
                                   c->csr_ptr.get(), c->csr_ent.get(), tab.get(), mask.get(), d_temp, div, s.get(), w.get(), o.get(),
                                   depth.get(), cnt.get());
            });
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(k_cluster_objective, dim3(R), dim3(LANE_THREADS), 0, c->stream, n, R, o.get(), obj.get());
        HIPCHK(c, hipGetLastError());
        ev.mark(1, c->stream);
        open_e = ev.on;
        return CELLECTOR_OK;
    }

    cellector_status m_step(double floor, bool at)
    {
        const int jp = lane_width(J, 2);
        ev.mark(2, c->stream);
        if (L)
            lane_dispatch<2, 64>(jp, [&](auto JP) {
                hipLaunchKernelGGL(k_cluster_m<JP>, dim3(lane_walk_grid(L, jp, c->n_cu)), dim3(LANE_THREADS), 0, c->stream, L, J,
                                   c->csc_ptr.get(), bl.get(), w.get(), mask.get(), floor, at ? A.get() : (double *)nullptr,
                                   at ? T.get() : (double *)nullptr, theta.get());
            });
        HIPCHK(c, hipGetLastError());
        ev.mark(3, c->stream);
        open_m = ev.on;
        return CELLECTOR_OK;
    }
};

// K columns from column j0 of a device [rows][J] array into out [K][rows] on the host
cellector_status take_columns(cellector_ctx *c, const double *d, uint64_t rows, uint32_t J, uint32_t j0, uint32_t K, double *out)
{
    if (!out || !rows) return CELLECTOR_OK;
    std::vector<double> h(rows * K);
    HIPCHK(c, hipMemcpy2DAsync(h.data(), (size_t)K * 8, d + j0, (size_t)J * 8, (size_t)K * 8, rows, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (uint64_t i = 0; i < rows; i++)
        for (uint32_t k = 0; k < K; k++) out[(uint64_t)k * rows + i] = h[i * K + k];
    return CELLECTOR_OK;
}

}  // namespace

// one M step and the tables from its theta: w [cells][J] host; A, T, theta [J][L], tab [L][J][2] host, any may be null
cellector_status cluster_m_step_run(cellector_ctx *c, const double *w, uint32_t J, const uint8_t *mask, double floor, double *A, double *T,
                                    double *theta, double *tab)
{
    ClusterRun r{c, J, 1, J, c->nloc, c->L};
    CHK(r.alloc(false, true, A || T, false));
    invalidate_cell_ll_state(c);
    CHK(r.mask.set(c, mask, r.L));
    if (r.n) HIPCHK(c, hipMemcpyAsync(r.w, w, r.n * J * 8, hipMemcpyHostToDevice, c->stream));
    cellector_status st = r.m_step(floor, A || T);
    if (st == CELLECTOR_OK) st = r.tables();
    if (st == CELLECTOR_OK && (A || T)) {
        st = take_columns(c, r.A, r.L, J, 0, J, A);
        if (st == CELLECTOR_OK) st = take_columns(c, r.T, r.L, J, 0, J, T);
    }
    if (st == CELLECTOR_OK) st = take_columns(c, r.theta, r.L, J, 0, J, theta);
    if (st == CELLECTOR_OK && tab) st = d2h(c, tab, r.tab, r.L * J * 16);
    (void)hipStreamSynchronize(c->stream);  // (nothing of the scratch may be in use when it goes)
    return st;
}

// one E step on the caller's tables: tab [L][J][2], temp [cells] or null host; s, w [cells][J], objective [R] host, any may be null
cellector_status cluster_e_step_run(cellector_ctx *c, const double *tab, uint32_t K, uint32_t R, const double *temp, const uint8_t *mask,
                                    double *s, double *w, double *objective)
{
    const uint32_t J = K * R;
    ClusterRun r{c, K, R, J, c->nloc, c->L};
    CHK(r.alloc(true, false, false, temp != nullptr));
    invalidate_cell_ll_state(c);
    CHK(r.mask.set(c, mask, r.L));
    if (r.L) HIPCHK(c, hipMemcpyAsync(r.tab, tab, r.L * J * 16, hipMemcpyHostToDevice, c->stream));
    if (temp && r.n) HIPCHK(c, hipMemcpyAsync(r.temp, temp, r.n * 8, hipMemcpyHostToDevice, c->stream));
    cellector_status st = r.e_step(temp ? r.temp.get() : nullptr, 0.0);
    if (st == CELLECTOR_OK && s) st = d2h(c, s, r.s, r.n * J * 8);
    if (st == CELLECTOR_OK && w) st = d2h(c, w, r.w, r.n * J * 8);
    if (st == CELLECTOR_OK && objective) st = d2h(c, objective, r.obj, (uint64_t)R * 8);
    (void)hipStreamSynchronize(c->stream);
    if (r.ev.on && st == CELLECTOR_OK) {
        r.collect();
        fprintf(stderr, "[timing]   cluster_e_step: J %u E step %.3f ms\n", J, r.ms_e);
    }
    return st;
}

// the annealed soft EM over R restarts: validated arguments; host outputs, any may be null
cellector_status cluster_run(cellector_ctx *c, uint32_t K, uint32_t R, uint64_t seed, const cellector_cluster_params *p, const uint8_t *mask,
                             uint8_t *labels, double *ll, double *posterior, double *theta, double *objective,
                             cellector_cluster_summary *out)
{
    const uint32_t J = K * R;
    LapTimer whole;
    ClusterRun r{c, K, R, J, c->nloc, c->L};
    const uint64_t n = r.n, L = r.L;
    CHK(r.alloc(true, true, false, false));
    invalidate_cell_ll_state(c);
    CHK(r.mask.set(c, mask, r.L));
    cellector_cluster_summary sum = {};
    std::vector<double> obj(R), prev(R);
    cellector_status st = CELLECTOR_OK;
    if (L * J) {
        hipLaunchKernelGGL(k_cluster_start, dim3(lane_grid(L * J, LANE_THREADS, 0x7fffffffu)), dim3(LANE_THREADS), 0, c->stream, L * J,
                           mix64(seed * GOLD + GOLD), p->theta_floor, r.theta.get());
        if (hipGetLastError() != hipSuccess) st = ctx_fail(c, CELLECTOR_EDEVICE, "cluster: start launch failed");
    }
    // the stage loop: no allocation inside, one stream, one read of R doubles per iteration
    for (uint32_t stage = 0; stage < p->anneal_steps && st == CELLECTOR_OK; stage++) {
        const double div = stage + 1 < p->anneal_steps ? std::ldexp(p->anneal_base, (int)stage) : 0.0;  // the last stage: T = 1
        for (uint32_t it = 0; it < p->max_iter; it++) {
            if ((st = r.tables()) != CELLECTOR_OK) break;
            if ((st = r.e_step(nullptr, div)) != CELLECTOR_OK) break;
            if ((st = r.m_step(p->theta_floor, false)) != CELLECTOR_OK) break;
            if ((st = d2h(c, obj.data(), r.obj, (uint64_t)R * 8)) != CELLECTOR_OK) break;
            r.collect();
            sum.iterations++;
            sum.iterations_per_stage[stage]++;
            bool still = it > 0;
            for (uint32_t q = 0; q < R && still; q++) still = std::fabs(obj[q] - prev[q]) < p->tol;
            prev = obj;
            if (still) break;
        }
        sum.stages++;
    }
    // the result: the tables of the final theta and one E step at T = 1
    if (st == CELLECTOR_OK) st = r.tables();
    if (st == CELLECTOR_OK) st = r.e_step(nullptr, 0.0);
    if (st == CELLECTOR_OK) st = d2h(c, obj.data(), r.obj, (uint64_t)R * 8);
    if (st != CELLECTOR_OK) {
        (void)hipStreamSynchronize(c->stream);
        return st;
    }
    r.collect();
    if (r.ev.on)
        fprintf(stderr, "[timing]   cluster: K %u R %u by-locus list %.4f s, E step %.3f ms x %u, M step %.3f ms x %u, whole call %.4f s\n", K, R,
                r.s_list, r.n_e ? r.ms_e / r.n_e : 0.0, r.n_e, r.n_m ? r.ms_m / r.n_m : 0.0, r.n_m, whole.lap());
    const double shift = (double)n * std::log((double)K);
    uint32_t best = 0;
    for (uint32_t q = 0; q < R; q++) {
        obj[q] = obj[q] - shift;
        if (obj[q] > obj[best]) best = q;
    }
    sum.best_restart = best;
    std::vector<double> hs((uint64_t)K * n);
    std::vector<uint32_t> cnt(n);
    st = take_columns(c, r.s, n, J, best * K, K, hs.data());
    if (st == CELLECTOR_OK && n) st = d2h(c, cnt.data(), r.cnt, n * 4);
    if (st == CELLECTOR_OK) st = take_columns(c, r.w, n, J, best * K, K, posterior);
    if (st == CELLECTOR_OK) st = take_columns(c, r.theta, L, J, best * K, K, theta);
    (void)hipStreamSynchronize(c->stream);
    if (st != CELLECTOR_OK) return st;
    for (uint64_t i = 0; i < n; i++) {
        uint32_t b = 0;
        for (uint32_t k = 1; k < K; k++)
            if (hs[(uint64_t)k * n + i] > hs[(uint64_t)b * n + i]) b = k;
        const bool lab = (uint64_t)cnt[i] >= p->min_loci;
        if (lab) sum.cluster_cells[b]++;
        else sum.n_unlabelled++;
        if (labels) labels[i] = lab ? (uint8_t)b : (uint8_t)255;
    }
    if (ll) memcpy(ll, hs.data(), hs.size() * 8);
    if (objective) memcpy(objective, obj.data(), (uint64_t)R * 8);
    if (out) *out = sum;
    return CELLECTOR_OK;
}
