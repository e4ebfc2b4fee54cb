// Ambient fraction estimation (cellector_ambient_tables, cellector_ambient_profile, cellector_estimate_ambient): the profile
// log-likelihood of the pool over a grid of G ambient fractions rho, every cell scored under the genotypes of the source it is
// assigned to.  include/cellector_ffi.h states the model completely; cellector_amd/ambient.py is its twin.
//
// The genotypes are packed as the donor calls pack them (k_donor_pack of kernels_donors.hip: 2 bits per source and locus), and a
// locus has four table rows of G grid points each: tab [L][4][G] double2, 64 G bytes per locus.
//   k_ambient_tables  one thread per (l, g, j): theta = ((1 - rho_j) e_g) + (rho_j soup), (log theta, log(1 - theta))
//   k_ambient_e       rows = cells of the by-cell CSR, lane = grid point j, in the shape lane_rows.h states; the tail finds the
//                     cell's own maximum over the grid and the vertex of the parabola through the three points around it
//   k_ambient_fold    block s < S: the cells of source s, block S: every cell that takes part; G ordered sums of the cells' rows
// All scratch belongs to the call.  Nothing of the ctx is written: the EM state, its tables and its outputs stay.
#include "lane_rows.h"
#include "vertex.h"

#include <cmath>

#define AM_NONE 255
#define AM_MIN_GP 4  // the lane width of the smallest grid: the tail reads three points of it
#define AM_MAX_G 32
// (AM_FLAT and am_vertex, the vertex rule of the tail and of the host folds: vertex.h, shared with kernels_pair_fraction.hip)

// thread (l, g, j) of tab [L][4][G]: soup and e_g as k_donor_tables makes them; a masked locus carries (0, 0)
__global__ __launch_bounds__(LANE_THREADS) void k_ambient_tables(uint64_t n /*4 L G*/, uint32_t G, const double *__restrict__ s_alt,
                                                                 const double *__restrict__ s_ref, const uint8_t *__restrict__ mask /*or null*/,
                                                                 double err, const double *__restrict__ rho /*[G]*/, double2 *__restrict__ tab)
{
    const uint64_t i = (uint64_t)blockIdx.x * LANE_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t j = (uint32_t)(i % G);
    const uint64_t lg = i / G, l = lg >> 2;
    const uint32_t g = (uint32_t)lg & 3u;
    double2 out = make_double2(0.0, 0.0);
    if (!mask || mask[l] != 0) {
        const double A = s_alt[l], R = s_ref[l];
        const double num = A + 1.0, tot = A + R, den = tot + 2.0;
        const double soup = num / den;
        const double r = rho[j];
        const double keep = 1.0 - r, amb = r * soup;
        const double e2 = 1.0 - err;
        const double e = g == 0 ? err : g == 1 ? 0.5 : g == 2 ? e2 : soup;
        const double p = keep * e;
        const double th = p + amb;
        const double rest = 1.0 - th;
        out = make_double2(log(th), log(rest));
    }
    tab[i] = out;
}

// The cell pass.  A group of GP lanes per cell, lane = grid point j.  acc = the ordered sum of (alt la + ref lb) over the row's
// entries at unmasked loci, (la, lb) = tab[l][g][j], g = the genotype of the cell's source at l.  A cell whose assign is 255 walks
// nothing.  The tail: j* = the smallest j of the largest sum, jj = min(max(j*, 1), G - 2), the vertex through jj - 1, jj, jj + 1.
template <int GP>
__global__ __launch_bounds__(LANE_THREADS) void k_ambient_e(uint64_t n_rows, uint32_t G, uint32_t W, const uint64_t *__restrict__ row_ptr,
                                                            const uint64_t *__restrict__ ent, const uint64_t *__restrict__ packed,
                                                            const double2 *__restrict__ tab, const uint8_t *__restrict__ mask /*or null*/,
                                                            const uint8_t *__restrict__ assign, const double *__restrict__ rho, uint64_t min_loci,
                                                            double *__restrict__ ll /*[rows][G]*/, uint32_t *__restrict__ cnt_out /*or null*/,
                                                            double *__restrict__ cell_rho /*or null*/, double *__restrict__ cell_se /*or null*/)
{
    const LaneGeom<GP> geo(n_rows, G);
    const int col = geo.col, base = geo.base;
    const bool col_ok = geo.ok;
    for (uint64_t grp = geo.wave0; grp < geo.n_groups; grp += geo.n_waves) {
        const uint64_t row = geo.row(grp);
        const bool have = row < n_rows;
        const uint32_t src = have ? assign[row] : AM_NONE;
        const bool part = src != AM_NONE && src < 32u * W;  // (the host checks that any other value is below S)
        const uint64_t beg = part ? row_ptr[row] : 0, end = part ? row_ptr[row + 1] : 0;
        const uint32_t s_word = part ? src >> 5 : 0u, s_shift = 2u * (src & 31u);
        double acc = 0.0;
        uint32_t cnt = 0;
        // the entry loop of lane_rows.h: a fix here belongs in k_cluster_e, k_donor_e, k_donor_fit, k_pair_fraction_e and k_donor_match as well
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
                t[q] = make_double2(0.0, 0.0);
                if (use[q] && col_ok) {
                    const uint32_t g = (uint32_t)(packed[l * W + s_word] >> s_shift) & 3u;
                    t[q] = tab[(l * 4 + g) * G + (uint32_t)col];
                }
            }
#pragma unroll
            for (int q = 0; q < LANE_AHEAD; q++) {
                if (!use[q]) continue;
                const uint32_t al = ENT_ALT(en[q]), re = ENT_REF(en[q]);
                const double pa = (double)al * t[q].x, pb = (double)re * t[q].y;
                const double term = pa + pb;
                acc = acc + term;
                cnt++;
            }
        }
        // the tail
        double v = col_ok ? acc : -INFINITY;
        int js = col_ok ? col : 0x7fff;
        lane_argmax<GP>(v, js);
        const int hi = (int)G - 2;
        int jj = js < 1 ? 1 : js;
        if (jj > hi) jj = hi;
        const double y0 = __shfl(acc, (base + jj - 1) & 63, 64);
        const double y1 = __shfl(acc, (base + jj) & 63, 64);
        const double y2 = __shfl(acc, (base + jj + 1) & 63, 64);
        if (have && col_ok) ll[row * G + (uint32_t)col] = acc;
        if (have && col == 0) {
            if (cnt_out) cnt_out[row] = cnt;
            if (cell_rho || cell_se) {
                double est, se, curv;
                am_vertex(rho[jj - 1], rho[jj], rho[jj + 1], y0, y1, y2, rho[js], &est, &se, &curv);
                if (!part || (uint64_t)cnt < min_loci) est = se = NAN;
                if (cell_rho) cell_rho[row] = est;
                if (cell_se) cell_se[row] = se;
            }
        }
    }
}

// Block b < S: the cells of source b; block S: every cell whose assign is not 255.  Thread t adds the rows of its cells t, t + 256,
// ... in ascending order, one sum per grid point; the 256 partial sums of a grid point are folded pairwise (h = 128 ... 1), as
// k_cluster_objective folds.  cells[b] = how many cells the block summed.
template <int GP>
__global__ __launch_bounds__(LANE_THREADS) void k_ambient_fold(uint64_t n, uint32_t G, uint32_t S, const double *__restrict__ ll /*[n][G]*/,
                                                               const uint8_t *__restrict__ assign, double *__restrict__ tot /*[S + 1][G]*/,
                                                               unsigned long long *__restrict__ cells /*[S + 1]*/)
{
    __shared__ double sh[LANE_THREADS];
    __shared__ unsigned long long shn[LANE_THREADS];
    const uint32_t b = blockIdx.x;
    double a[GP];
#pragma unroll
    for (int j = 0; j < GP; j++) a[j] = 0.0;
    unsigned long long m = 0;
    for (uint64_t i = threadIdx.x; i < n; i += LANE_THREADS) {
        const uint32_t src = assign[i];
        if (b < S ? src != b : src == AM_NONE) continue;
        const double *row = ll + i * G;
#pragma unroll
        for (int j = 0; j < GP; j++)
            if ((uint32_t)j < G) a[j] = a[j] + row[j];
        m++;
    }
    shn[threadIdx.x] = m;
    __syncthreads();
    for (int h = LANE_THREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) shn[threadIdx.x] += shn[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) cells[b] = shn[0];
#pragma unroll
    for (int j = 0; j < GP; j++) {  // (the columns j >= G fold zeros and are not stored)
        __syncthreads();
        sh[threadIdx.x] = a[j];
        __syncthreads();
        for (int h = LANE_THREADS / 2; h > 0; h >>= 1) {
            if ((int)threadIdx.x < h) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + h];
            __syncthreads();
        }
        if (threadIdx.x == 0 && (uint32_t)j < G) tot[(uint64_t)b * G + j] = sh[0];
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
namespace {

// the scratch of one call; alloc() makes all of it before anything is launched
struct AmbientRun {
    cellector_ctx *c;
    uint32_t S, W, G;
    uint64_t n, L, TL;
    DevBuf<uint8_t> gt, assign;        // [S][TL], [n]
    LociMask mask;                     // [L]
    DevBuf<uint64_t> packed;           // [L][W]
    DevBuf<double2> tab;               // [L][4][G]
    DevBuf<double> rho, ll, tot;       // [G], [n][G], [S + 1][G]
    DevBuf<double> cell_rho, cell_se;  // [n]
    DevBuf<uint32_t> cnt;              // [n]
    DevBuf<unsigned long long> cells;  // [S + 1]
    EventMarks<2> ev;                  // around the cell pass and the folds of a profile

    cellector_status alloc(bool cell_pass)
    {
        CHK(dev_alloc(c, &mask.buf, L));
        CHK(dev_alloc(c, &rho, G));
        CHK(dev_alloc(c, &tab, L * 4 * G));
        if (cell_pass) {
            CHK(dev_alloc(c, &gt, (uint64_t)S * TL));
            CHK(dev_alloc(c, &packed, L * W));
            CHK(dev_alloc(c, &assign, n));
            CHK(dev_alloc(c, &ll, n * G));
            CHK(dev_alloc(c, &cell_rho, n)); CHK(dev_alloc(c, &cell_se, n));
            CHK(dev_alloc(c, &cnt, n));
            CHK(dev_alloc(c, &tot, (uint64_t)(S + 1) * G));
            CHK(dev_alloc(c, &cells, S + 1));
        }
        return CELLECTOR_OK;
    }

    // one upload of the mask, of gt and of assign, and the packing
    cellector_status prepare(const uint8_t *host_gt, const uint8_t *host_assign, const uint8_t *host_mask)
    {
        CHK(mask.set(c, host_mask, L));
        if (host_assign && n) HIPCHK(c, hipMemcpyAsync(assign, host_assign, n, hipMemcpyHostToDevice, c->stream));
        if (!host_gt || !L) return CELLECTOR_OK;
        HIPCHK(c, hipMemcpyAsync(gt, host_gt, (uint64_t)S * TL, hipMemcpyHostToDevice, c->stream));
        return donor_pack_launch(c, S, gt.get(), packed.get());
    }

    // the tables of one grid (the host's rho is consumed before this returns)
    cellector_status tables(const double *host_rho, double err)
    {
        HIPCHK(c, hipMemcpyAsync(rho, host_rho, (uint64_t)G * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (!L) return CELLECTOR_OK;
        hipLaunchKernelGGL(k_ambient_tables, dim3(lane_grid(L * 4 * G, LANE_THREADS, 0x7fffffffu)), dim3(LANE_THREADS), 0, c->stream,
                           L * 4 * G, G, c->s_alt.get(), c->s_ref.get(), mask.get(), err, rho.get(), tab.get());
        HIPCHK(c, hipGetLastError());
        return CELLECTOR_OK;
    }

    // the cell pass and the folds; cells == false: the per-cell outputs of an earlier pass stay
    cellector_status pass(uint64_t min_loci, bool cells_out)
    {
        const int gp = lane_width(G, AM_MIN_GP);
        if (n) {
            lane_dispatch<AM_MIN_GP, AM_MAX_G>(gp, [&](auto GP) {
                hipLaunchKernelGGL(k_ambient_e<GP>, dim3(lane_walk_grid(n, gp, c->n_cu)), dim3(LANE_THREADS), 0, c->stream, n, G, W,
                                   c->csr_ptr.get(), c->csr_ent.get(), packed.get(), tab.get(), mask.get(), assign.get(), rho.get(), min_loci,
                                   ll.get(), cells_out ? cnt.get() : nullptr, cells_out ? cell_rho.get() : nullptr,
                                   cells_out ? cell_se.get() : nullptr);
            });
            HIPCHK(c, hipGetLastError());
        }
        lane_dispatch<AM_MIN_GP, AM_MAX_G>(gp, [&](auto GP) {
            hipLaunchKernelGGL(k_ambient_fold<GP>, dim3(S + 1), dim3(LANE_THREADS), 0, c->stream, n, G, S, ll.get(), assign.get(), tot.get(),
                               cells.get());
        });
        HIPCHK(c, hipGetLastError());
        return CELLECTOR_OK;
    }
};

// the vertex rule of the header's step 4 on G totals
void am_host_vertex(const double *rho, const double *y, uint32_t G, uint32_t *j_star, double *est, double *se, double *curv)
{
    uint32_t js = 0;
    for (uint32_t j = 1; j < G; j++)
        if (y[j] > y[js]) js = j;
    uint32_t jj = js < 1 ? 1 : js;
    if (jj > G - 2) jj = G - 2;
    am_vertex(rho[jj - 1], rho[jj], rho[jj + 1], y[jj - 1], y[jj], y[jj + 1], rho[js], est, se, curv);
    *j_star = js;
}

}  // namespace

// cellector_ambient_tables: validated arguments; tab [L][4][G][2] host
cellector_status ambient_tables_run(cellector_ctx *c, const double *rho, uint32_t G, double err, const uint8_t *mask, double *tab)
{
    AmbientRun r{c, 0, 0, G, c->nloc, c->L, c->total_loci};
    CHK(r.alloc(false));
    invalidate_cell_ll_state(c);
    cellector_status st = r.prepare(nullptr, nullptr, mask);
    if (st == CELLECTOR_OK) st = r.tables(rho, err);
    if (st == CELLECTOR_OK && tab) st = d2h(c, tab, r.tab, r.L * 4 * G * 16);
    (void)hipStreamSynchronize(c->stream);  // (nothing of the scratch may be in use when it goes)
    return st;
}

// cellector_ambient_profile: validated arguments; host outputs, any may be null
cellector_status ambient_profile_run(cellector_ctx *c, const uint8_t *gt, uint32_t S, const uint8_t *assign, const double *rho, uint32_t G,
                                     double err, uint64_t min_loci, const uint8_t *mask, double *ll, double *total, double *source_total,
                                     uint64_t *source_cells, uint32_t *n_entries, double *cell_rho, double *cell_se, double *tab)
{
    LapTimer whole;
    AmbientRun r{c, S, (S + 31) / 32, G, c->nloc, c->L, c->total_loci};
    const uint64_t n = r.n;
    CHK(r.alloc(true));
    invalidate_cell_ll_state(c);
    cellector_status st = r.prepare(gt, assign, mask);
    if (st == CELLECTOR_OK) st = r.tables(rho, err);
    r.ev.mark(0, c->stream);
    if (st == CELLECTOR_OK) st = r.pass(min_loci, true);
    r.ev.mark(1, c->stream);
    std::vector<double> h_tot((uint64_t)(S + 1) * G);
    std::vector<unsigned long long> h_cells(S + 1);
    if (st == CELLECTOR_OK) st = d2h(c, h_tot.data(), r.tot, h_tot.size() * 8);
    if (st == CELLECTOR_OK) st = d2h(c, h_cells.data(), r.cells, h_cells.size() * 8);
    if (st == CELLECTOR_OK && ll) st = d2h(c, ll, r.ll, n * G * 8);
    if (st == CELLECTOR_OK && n_entries) st = d2h(c, n_entries, r.cnt, n * 4);
    if (st == CELLECTOR_OK && cell_rho) st = d2h(c, cell_rho, r.cell_rho, n * 8);
    if (st == CELLECTOR_OK && cell_se) st = d2h(c, cell_se, r.cell_se, n * 8);
    if (st == CELLECTOR_OK && tab) st = d2h(c, tab, r.tab, r.L * 4 * G * 16);
    (void)hipStreamSynchronize(c->stream);
    float ms = 0.f;
    if (st == CELLECTOR_OK && r.ev.ms(0, 1, &ms))
        fprintf(stderr, "[timing]   ambient: S %u G %u cell pass and folds %.3f ms, whole call %.4f s\n", S, G, ms, whole.lap());
    if (st != CELLECTOR_OK) return st;
    if (total) memcpy(total, h_tot.data() + (uint64_t)S * G, (uint64_t)G * 8);
    if (source_total) memcpy(source_total, h_tot.data(), (uint64_t)S * G * 8);
    for (uint32_t s = 0; source_cells && s < S; s++) source_cells[s] = h_cells[s];
    return CELLECTOR_OK;
}

// cellector_estimate_ambient: validated arguments and parameters; host outputs, any may be null
cellector_status ambient_estimate_run(cellector_ctx *c, const uint8_t *gt, uint32_t S, const uint8_t *assign, const cellector_ambient_params *p,
                                      const uint8_t *mask, cellector_ambient_summary *out, double *cell_rho, double *cell_se,
                                      uint32_t *n_entries)
{
    LapTimer whole;
    const uint32_t G = p->grid;
    AmbientRun r{c, S, (S + 31) / 32, G, c->nloc, c->L, c->total_loci};
    const uint64_t n = r.n;
    CHK(r.alloc(true));
    invalidate_cell_ll_state(c);
    std::vector<double> h_tot((uint64_t)(S + 1) * G);
    std::vector<unsigned long long> h_cells(S + 1);
    double rho[AM_MAX_G];
    double lo = p->lo, hi = p->hi;
    uint32_t js = 0;
    cellector_status st = r.prepare(gt, assign, mask);
    for (uint32_t round = 0; st == CELLECTOR_OK && round < p->rounds; round++) {
        if (round) {
            lo = rho[js < 1 ? 0 : js - 1];
            hi = rho[js + 1 > G - 1 ? G - 1 : js + 1];
        }
        const double span = hi - lo;
        const double step = span / (double)(G - 1);
        for (uint32_t j = 0; j < G; j++) {
            const double off = (double)j * step;
            rho[j] = lo + off;
        }
        st = r.tables(rho, p->err);
        if (st == CELLECTOR_OK) st = r.pass(p->min_loci, round == 0);
        if (st == CELLECTOR_OK) st = d2h(c, h_tot.data(), r.tot, h_tot.size() * 8);
        if (st == CELLECTOR_OK && round == 0) {
            st = d2h(c, h_cells.data(), r.cells, h_cells.size() * 8);
            if (st == CELLECTOR_OK && cell_rho) st = d2h(c, cell_rho, r.cell_rho, n * 8);
            if (st == CELLECTOR_OK && cell_se) st = d2h(c, cell_se, r.cell_se, n * 8);
            if (st == CELLECTOR_OK && n_entries) st = d2h(c, n_entries, r.cnt, n * 4);
        }
        if (st != CELLECTOR_OK) break;
        const double *tot = h_tot.data() + (uint64_t)S * G;
        js = 0;
        for (uint32_t j = 1; j < G; j++)
            if (tot[j] > tot[js]) js = j;
    }
    (void)hipStreamSynchronize(c->stream);
    if (st != CELLECTOR_OK) return st;
    if (r.ev.on) fprintf(stderr, "[timing]   ambient: S %u G %u rounds %u, whole call %.4f s\n", S, G, p->rounds, whole.lap());
    if (!out) return CELLECTOR_OK;
    cellector_ambient_summary sum = {};
    const double *tot = h_tot.data() + (uint64_t)S * G;
    uint32_t j_star = 0;
    am_host_vertex(rho, tot, G, &j_star, &sum.rho, &sum.se, &sum.curvature);
    if (sum.rho < p->lo) sum.rho = p->lo;
    if (sum.rho > p->hi) sum.rho = p->hi;
    sum.log_likelihood = tot[j_star];
    sum.lo = lo;
    sum.hi = hi;
    sum.j_star = j_star;
    sum.at_boundary = sum.rho <= p->lo || sum.rho >= p->hi;
    sum.rounds = p->rounds;
    sum.n_cells_used = h_cells[S];
    for (uint32_t s = 0; s < 64; s++) {
        sum.source_rho[s] = sum.source_se[s] = NAN;
        if (s >= S) continue;
        sum.source_cells[s] = h_cells[s];
        if (!h_cells[s]) continue;
        uint32_t jsrc;
        double curv;
        am_host_vertex(rho, h_tot.data() + (uint64_t)s * G, G, &jsrc, &sum.source_rho[s], &sum.source_se[s], &curv);
        if (sum.source_rho[s] < p->lo) sum.source_rho[s] = p->lo;
        if (sum.source_rho[s] > p->hi) sum.source_rho[s] = p->hi;
    }
    *out = sum;
    return CELLECTOR_OK;
}
