// Donor pair fractions (cellector_pair_fraction_tables, cellector_donor_pair_fractions): the share f of a cell's reads that come from
// donor a of the pair (a, b) it is scored under, profiled over a grid of G values of f.  include/cellector_ffi.h states the model
// completely; cellector_amd/pair_fraction.py is its twin.
//
// The genotypes are packed as the donor calls pack them (k_donor_pack of kernels_donors.hip: 2 bits per donor and locus), and a locus
// has sixteen table rows of G grid points each, one per (genotype of a, genotype of b): tab [L][16][G] double2, 256 G bytes per locus,
// of which an entry reads one row of 16 G bytes, as the ambient pass does.
//   k_pair_fraction_tables  one thread per (l, 4 ga + gb, j): theta_ga, theta_gb by k_donor_tables' own operations, then
//                           theta = (f_j theta_ga) + ((1 - f_j) theta_gb), (log theta, log(1 - theta))
//   k_pair_fraction_e       rows = cells of the by-cell CSR, lane = grid point j, in the shape lane_rows.h states; two genotype
//                           extractions per entry; the tail finds the cell's own maximum over the grid, the vertex of the parabola
//                           through the three points around it (vertex.h: the ambient pass's own rule) and the cell's kind
// All scratch belongs to the call.  Nothing of the ctx is written: the EM state, its tables and its outputs stay.
#include "lane_rows.h"
#include "vertex.h"

#include <cmath>

#define PF_NONE 255
#define PF_MIN_GP 4  // the lane width of the smallest grid: the tail reads three points of it
#define PF_MAX_G 32

// thread (l, 4 ga + gb, j) of tab [L][16][G]: soup, theta_ga and theta_gb as k_donor_tables makes them; a masked locus carries (0, 0)
__global__ __launch_bounds__(LANE_THREADS) void k_pair_fraction_tables(uint64_t n /*16 L G*/, uint32_t G, const double *__restrict__ s_alt,
                                                                       const double *__restrict__ s_ref,
                                                                       const uint8_t *__restrict__ mask /*or null*/, double err, double ambient,
                                                                       const double *__restrict__ frac /*[G]*/, double2 *__restrict__ tab)
{
    const uint64_t i = (uint64_t)blockIdx.x * LANE_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t j = (uint32_t)(i % G);
    const uint64_t lg = i / G, l = lg >> 4;
    const uint32_t ga = (uint32_t)(lg >> 2) & 3u, gb = (uint32_t)lg & 3u;
    double2 out = make_double2(0.0, 0.0);
    if (!mask || mask[l] != 0) {
        const double A = s_alt[l], R = s_ref[l];
        const double num = A + 1.0, tot = A + R, den = tot + 2.0;
        const double soup = num / den;
        const double keep = 1.0 - ambient, amb = ambient * soup;
        const double e2 = 1.0 - err;
        const double ea = ga == 0 ? err : ga == 1 ? 0.5 : ga == 2 ? e2 : soup;
        const double eb = gb == 0 ? err : gb == 1 ? 0.5 : gb == 2 ? e2 : soup;
        const double pa = keep * ea, pb = keep * eb;
        const double ta = pa + amb, tb = pb + amb;
        const double f = frac[j];
        const double fb = 1.0 - f;
        const double wa = f * ta, wb = fb * tb;
        const double th = wa + wb;
        const double rest = 1.0 - th;
        out = make_double2(log(th), log(rest));
    }
    tab[i] = out;
}

// The cell pass.  A group of GP lanes per cell, lane = grid point j.  acc = the ordered sum of (alt la + ref lb) over the row's
// entries at unmasked loci, (la, lb) = tab[l][4 ga + gb][j], ga and gb = the genotypes of the cell's two donors at l.  A cell whose
// pair_a is 255 walks nothing.  The tail: j* = the smallest j of the largest sum, jj = min(max(j*, 1), G - 2), the vertex through
// jj - 1, jj, jj + 1, then the kind.
template <int GP>
__global__ __launch_bounds__(LANE_THREADS) void k_pair_fraction_e(uint64_t n_rows, uint32_t G, uint32_t W, const uint64_t *__restrict__ row_ptr,
                                                                  const uint64_t *__restrict__ ent, const uint64_t *__restrict__ packed,
                                                                  const double2 *__restrict__ tab, const uint8_t *__restrict__ mask /*or null*/,
                                                                  const uint8_t *__restrict__ pair_a, const uint8_t *__restrict__ pair_b,
                                                                  const double *__restrict__ frac, uint64_t min_loci, double min_fraction,
                                                                  double *__restrict__ ll /*[rows][G]*/, uint32_t *__restrict__ cnt_out,
                                                                  double *__restrict__ cell_frac, double *__restrict__ cell_se,
                                                                  uint8_t *__restrict__ j_star, uint8_t *__restrict__ kind)
{
    const LaneGeom<GP> geo(n_rows, G);
    const int col = geo.col, base = geo.base;
    const bool col_ok = geo.ok;
    for (uint64_t grp = geo.wave0; grp < geo.n_groups; grp += geo.n_waves) {
        const uint64_t row = geo.row(grp);
        const bool have = row < n_rows;
        const uint32_t a = have ? pair_a[row] : PF_NONE, b = have ? pair_b[row] : PF_NONE;
        const bool part = a != PF_NONE && a < 32u * W && b < 32u * W;  // (the host checks that both are donors, and two)
        const uint64_t beg = part ? row_ptr[row] : 0, end = part ? row_ptr[row + 1] : 0;
        const uint32_t a_word = part ? a >> 5 : 0u, a_shift = 2u * (a & 31u);
        const uint32_t b_word = part ? b >> 5 : 0u, b_shift = 2u * (b & 31u);
        double acc = 0.0;
        uint32_t cnt = 0;
        // the entry loop of lane_rows.h: a fix here belongs in k_cluster_e, k_donor_e, k_donor_fit, k_ambient_e and k_donor_match as well
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
                    const uint32_t ga = (uint32_t)(packed[l * W + a_word] >> a_shift) & 3u;
                    const uint32_t gb = (uint32_t)(packed[l * W + b_word] >> b_shift) & 3u;
                    t[q] = tab[(l * 16 + 4 * ga + gb) * G + (uint32_t)col];
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
        // the tail: every lane of the wave takes part in the shuffles, whatever its row and column
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
            double est, se, curv;
            am_vertex(frac[jj - 1], frac[jj], frac[jj + 1], y0, y1, y2, frac[js], &est, &se, &curv);
            const double top = 1.0 - min_fraction;
            uint8_t k = se == INFINITY ? (uint8_t)3 : est > top ? (uint8_t)1 : est < min_fraction ? (uint8_t)2 : (uint8_t)0;
            if (!part || (uint64_t)cnt < min_loci) {
                est = se = NAN;
                k = (uint8_t)PF_NONE;
            }
            cnt_out[row] = cnt;
            cell_frac[row] = est;
            cell_se[row] = se;
            j_star[row] = (uint8_t)js;
            kind[row] = k;
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
namespace {

// the scratch of one call; alloc() makes all of it before anything is launched
struct PairFractionRun {
    cellector_ctx *c;
    uint32_t D, W, G;
    uint64_t n, L, TL;
    DevBuf<uint8_t> gt, pair_a, pair_b;  // [D][TL], [n], [n]
    LociMask mask;                       // [L]
    DevBuf<uint64_t> packed;             // [L][W]
    DevBuf<double2> tab;                 // [L][16][G]
    DevBuf<double> frac, ll;             // [G], [n][G]
    DevBuf<double> cell_frac, cell_se;   // [n]
    DevBuf<uint32_t> cnt;                // [n]
    DevBuf<uint8_t> j_star, kind;        // [n]
    EventMarks<2> ev;                    // around the cell pass

    cellector_status alloc(bool cell_pass)
    {
        CHK(dev_alloc(c, &mask.buf, L));
        CHK(dev_alloc(c, &frac, G));
        CHK(dev_alloc(c, &tab, L * 16 * G));
        if (cell_pass) {
            CHK(dev_alloc(c, &gt, (uint64_t)D * TL));
            CHK(dev_alloc(c, &packed, L * W));
            CHK(dev_alloc(c, &pair_a, n)); CHK(dev_alloc(c, &pair_b, n));
            CHK(dev_alloc(c, &ll, n * G));
            CHK(dev_alloc(c, &cell_frac, n)); CHK(dev_alloc(c, &cell_se, n));
            CHK(dev_alloc(c, &cnt, n));
            CHK(dev_alloc(c, &j_star, n)); CHK(dev_alloc(c, &kind, n));
        }
        return CELLECTOR_OK;
    }

    // one upload of the mask, of the grid, of gt and of the pairs; the packing and the tables
    cellector_status prepare(const uint8_t *host_gt, const uint8_t *host_a, const uint8_t *host_b, const double *host_frac,
                             const uint8_t *host_mask, const cellector_donor_params *prm)
    {
        CHK(mask.set(c, host_mask, L));
        HIPCHK(c, hipMemcpyAsync(frac, host_frac, (uint64_t)G * 8, hipMemcpyHostToDevice, c->stream));
        if (host_a && n) {
            HIPCHK(c, hipMemcpyAsync(pair_a, host_a, n, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(pair_b, host_b, n, hipMemcpyHostToDevice, c->stream));
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));  // (the host's grid may live on the caller's stack)
        if (!L) return CELLECTOR_OK;
        if (host_gt) {
            HIPCHK(c, hipMemcpyAsync(gt, host_gt, (uint64_t)D * TL, hipMemcpyHostToDevice, c->stream));
            CHK(donor_pack_launch(c, D, gt.get(), packed.get()));
        }
        hipLaunchKernelGGL(k_pair_fraction_tables, dim3(lane_grid(L * 16 * G, LANE_THREADS, 0x7fffffffu)), dim3(LANE_THREADS), 0, c->stream,
                           L * 16 * G, G, c->s_alt.get(), c->s_ref.get(), mask.get(), prm->err, prm->ambient, frac.get(), tab.get());
        HIPCHK(c, hipGetLastError());
        return CELLECTOR_OK;
    }

    cellector_status pass(const cellector_pair_fraction_params *fp)
    {
        if (!n) return CELLECTOR_OK;
        const int gp = lane_width(G, PF_MIN_GP);
        lane_dispatch<PF_MIN_GP, PF_MAX_G>(gp, [&](auto GP) {
            hipLaunchKernelGGL(k_pair_fraction_e<GP>, dim3(lane_walk_grid(n, gp, c->n_cu)), dim3(LANE_THREADS), 0, c->stream, n, G, W,
                               c->csr_ptr.get(), c->csr_ent.get(), packed.get(), tab.get(), mask.get(), pair_a.get(), pair_b.get(), frac.get(),
                               fp->min_loci, fp->min_fraction, ll.get(), cnt.get(), cell_frac.get(), cell_se.get(), j_star.get(), kind.get());
        });
        HIPCHK(c, hipGetLastError());
        return CELLECTOR_OK;
    }
};

}  // namespace

// cellector_pair_fraction_tables: validated arguments; tab [L][16][G][2] host
cellector_status pair_fraction_tables_run(cellector_ctx *c, const cellector_donor_params *prm, const double *frac, uint32_t G,
                                          const uint8_t *mask, double *tab)
{
    PairFractionRun r{c, 0, 0, G, c->nloc, c->L, c->total_loci};
    CHK(r.alloc(false));
    invalidate_cell_ll_state(c);
    cellector_status st = r.prepare(nullptr, nullptr, nullptr, frac, mask, prm);
    if (st == CELLECTOR_OK && tab) st = d2h(c, tab, r.tab, r.L * 16 * G * 16);
    (void)hipStreamSynchronize(c->stream);  // (nothing of the scratch may be in use when it goes)
    return st;
}

// cellector_donor_pair_fractions: validated arguments and parameters; host outputs, any may be null
cellector_status pair_fractions_run(cellector_ctx *c, const uint8_t *gt, uint32_t D, const cellector_donor_params *prm,
                                    const cellector_pair_fraction_params *fp, const uint8_t *pair_a, const uint8_t *pair_b, const double *frac,
                                    uint32_t G, const uint8_t *mask, double *ll, uint32_t *n_entries, double *cell_frac, double *cell_se,
                                    uint8_t *j_star, uint8_t *kind, cellector_pair_fraction_summary *out, double *tab)
{
    LapTimer whole;
    PairFractionRun r{c, D, (D + 31) / 32, G, c->nloc, c->L, c->total_loci};
    const uint64_t n = r.n;
    CHK(r.alloc(true));
    std::vector<uint8_t> h_kind(n);
    invalidate_cell_ll_state(c);
    cellector_status st = r.prepare(gt, pair_a, pair_b, frac, mask, prm);
    r.ev.mark(0, c->stream);
    if (st == CELLECTOR_OK) st = r.pass(fp);
    r.ev.mark(1, c->stream);
    if (st == CELLECTOR_OK && ll) st = d2h(c, ll, r.ll, n * G * 8);
    if (st == CELLECTOR_OK && n_entries) st = d2h(c, n_entries, r.cnt, n * 4);
    if (st == CELLECTOR_OK && cell_frac) st = d2h(c, cell_frac, r.cell_frac, n * 8);
    if (st == CELLECTOR_OK && cell_se) st = d2h(c, cell_se, r.cell_se, n * 8);
    if (st == CELLECTOR_OK && j_star) st = d2h(c, j_star, r.j_star, n);
    if (st == CELLECTOR_OK) st = d2h(c, h_kind.data(), r.kind, n);
    if (st == CELLECTOR_OK && tab) st = d2h(c, tab, r.tab, r.L * 16 * G * 16);
    (void)hipStreamSynchronize(c->stream);
    float ms = 0.f;
    if (st == CELLECTOR_OK && r.ev.ms(0, 1, &ms))
        fprintf(stderr, "[timing]   pair fractions: D %u G %u cell pass %.3f ms, whole call %.4f s\n", D, G, ms, whole.lap());
    if (st != CELLECTOR_OK) return st;
    cellector_pair_fraction_summary sum = {};
    for (uint64_t i = 0; i < n; i++) {
        switch (h_kind[i]) {
        case 0: sum.n_balanced++; break;
        case 1: sum.n_toward_a++; sum.donor_cells[pair_a[i] < 64 ? pair_a[i] : 0]++; break;
        case 2: sum.n_toward_b++; sum.donor_cells[pair_b[i] < 64 ? pair_b[i] : 0]++; break;
        case 3: sum.n_flat++; break;
        default: sum.n_none++; break;
        }
    }
    if (kind && n) memcpy(kind, h_kind.data(), n);
    if (out) *out = sum;
    return CELLECTOR_OK;
}
