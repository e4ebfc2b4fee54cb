// Donor demultiplexing (cellector_donor_posteriors, cellector_donor_tables, cellector_match_donors): every cell, and every class of
// a labelling, scored against D donors whose genotypes are known.  include/cellector_ffi.h states the model completely;
// cellector_amd/donors.py is its twin.
//
// A donor's genotype at a locus is 2 bits.  The D genotypes of a used locus are packed into W = ceil(D / 32) u64 words (donor d at
// bits 2 (d & 31) of word d >> 5), and a locus has FOUR table rows, one per genotype value, whatever D is: 64 B of singlet table
// and 256 B of pair table per locus, against the 16 D bytes of a table with a column per donor.
//   k_donor_pack    gt [D][total_loci] u8 -> packed [L][W], over the used loci
//   k_donor_tables  tab1 [L][4] and tab2 [L][16] double2 from the locus' alt / ref totals
//   k_donor_e       rows = cells of the by-cell CSR, lane = donor, in the shape lane_rows.h states.  <DP, false>: the singlet sums,
//                   best, second and the anchor; <DP, true>: the pair sums (anchor, d) and the posterior chain over the 2 D - 1
//                   hypotheses
//   k_donor_match   a lane per (class, donor): the class' tallies over ascending loci, the same terms in the same order
// The same calls from genotype probabilities (three weights per donor and locus in place of a code) are the section behind
// k_donor_match; the fit of the called hypothesis (cellector_donor_fit: k_donor_moments, k_donor_fit) is the one behind that.  All
// scratch belongs to the call.  Nothing of the ctx is written: the EM state, its tables and its outputs stay.
#include "lane_rows.h"

#include <cmath>

#define DN_NONE 255

// packed[l][w]: donor d = 32 w + i at bits 2 i, from gt[d][locus_ids[l]]; the bits of donors >= D are 0
__global__ __launch_bounds__(LANE_THREADS) void k_donor_pack(uint64_t n /*L W*/, uint32_t D, uint32_t W, uint64_t TL,
                                                             const uint64_t *__restrict__ locus_ids, const uint8_t *__restrict__ gt,
                                                             uint64_t *__restrict__ packed)
{
    const uint64_t i = (uint64_t)blockIdx.x * LANE_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint64_t l = i / W, t = locus_ids[l];
    const uint32_t w = (uint32_t)(i % W);
    uint64_t word = 0;
    if (t < TL)
        for (uint32_t b = 0; b < 32 && 32 * w + b < D; b++) word |= (uint64_t)(gt[(uint64_t)(32 * w + b) * TL + t] & 3u) << (2 * b);
    packed[i] = word;
}

// theta_g = (1 - ambient) e_g + ambient soup, e = {err, 0.5, 1 - err, soup}, soup = (A + 1) / ((A + R) + 2) from the locus' totals
// (whole numbers below 2^53 held as doubles: their sum is exact).  Thread (l, 4 ga + gb): tab2 from 0.5 (theta_ga + theta_gb); the
// diagonal is tab1 ((x + x) 0.5 == x).  A masked locus carries (0, 0).
__global__ __launch_bounds__(LANE_THREADS) void k_donor_tables(uint64_t n /*16 L*/, const double *__restrict__ s_alt, const double *__restrict__ s_ref,
                                                               const uint8_t *__restrict__ mask /*or null*/, double err, double ambient,
                                                               double2 *__restrict__ tab1, double2 *__restrict__ tab2)
{
    const uint64_t i = (uint64_t)blockIdx.x * LANE_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint64_t l = i >> 4;
    const uint32_t ga = (uint32_t)(i >> 2) & 3u, gb = (uint32_t)i & 3u;
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
        const double sum = ta + tb;
        const double th = 0.5 * sum;
        const double rest = 1.0 - th;
        out = make_double2(log(th), log(rest));
    }
    tab2[i] = out;
    if (ga == gb) tab1[l * 4 + ga] = out;
}

struct DonorTail {
    double log_singlet, log_pair, threshold;
    uint64_t min_loci;
};

// The tail of a cell pass, shared by the hard and the soft kernels: acc = the lane's ordered sum, cnt = the row's entries.  Every lane of
// the wave takes part in the shuffles, whatever its row and donor.
// !PAIR: s = acc; u_d = s_d + lp_d; best = argmax u, second = argmax over d != best (smallest d on ties); the anchor, unless given
//  PAIR: p = acc; x_d = (s_d + lp_d) + log_singlet, y_d = p_d + log_pair (d != anchor), one softmax over the 2 D - 1 terms
template <int DP, bool PAIR>
__device__ __forceinline__ void dn_tail(uint64_t row, bool have, int col, bool col_ok, int base, uint32_t D, uint32_t a, double acc, uint32_t cnt,
                                        const double *__restrict__ lp, const DonorTail &tail, bool anchor_given, uint8_t *__restrict__ anchor,
                                        double *__restrict__ s, uint8_t *__restrict__ best, uint8_t *__restrict__ second,
                                        uint32_t *__restrict__ cnt_out, double *__restrict__ p_out, double *__restrict__ post,
                                        double *__restrict__ ppost, double *__restrict__ dp_out, uint8_t *__restrict__ best_pair,
                                        uint8_t *__restrict__ status)
{
    const double prior = col_ok ? lp[col] : 0.0;
    if (!PAIR) {
        double v = col_ok ? acc + prior : -INFINITY;
        int b = col_ok ? col : 0x7fff;
        const double u = v;
        lane_argmax<DP>(v, b);
        double v2 = col_ok && col != b ? u : -INFINITY;
        int b2 = col_ok && col != b ? col : 0x7fff;
        lane_argmax<DP>(v2, b2);
        if (have && col_ok) s[row * D + col] = acc;
        if (have && col == 0) {
            best[row] = (uint8_t)b;
            second[row] = D > 1 ? (uint8_t)b2 : (uint8_t)DN_NONE;
            if (!anchor_given) anchor[row] = (uint8_t)b;
            cnt_out[row] = cnt;
        }
    } else {
        const bool pair_ok = col_ok && (uint32_t)col != a;
        double x = -INFINITY, y = -INFINITY;
        if (have && col_ok) {
            const double u = s[row * D + col] + prior;
            x = u + tail.log_singlet;
        }
        if (pair_ok) y = acc + tail.log_pair;
        double m = fmax(x, y);
        int dummy = 0;
        lane_argmax<DP>(m, dummy);
        if (!have) m = 0.0;
        const double ex = exp(x - m), ey = exp(y - m);  // a lane that is no hypothesis: exp(-inf) = 0, and den + 0 is den
        double den = 0.0;
        for (uint32_t d = 0; d < D; d++) den = den + __shfl(ex, (base + (int)d) & 63, 64);
        for (uint32_t d = 0; d < D; d++) den = den + __shfl(ey, (base + (int)d) & 63, 64);
        const double w = ex / den, wp = ey / den;
        double dp = 0.0;
        for (uint32_t d = 0; d < D; d++) dp = dp + __shfl(wp, (base + (int)d) & 63, 64);
        double vy = y;
        int bp = pair_ok ? col : 0x7fff;
        lane_argmax<DP>(vy, bp);
        const int b = have ? (int)best[row] : 0;
        const double wb = __shfl(w, (base + b) & 63, 64);
        if (have && col_ok) {
            p_out[row * D + col] = acc;
            post[row * D + col] = w;
            ppost[row * D + col] = wp;
        }
        if (have && col == 0) {
            dp_out[row] = dp;
            best_pair[row] = D > 1 ? (uint8_t)bp : (uint8_t)DN_NONE;
            status[row] = (uint64_t)cnt < tail.min_loci ?(uint8_t)DN_NONE : dp > 0.5 ? (uint8_t)1 : wb >= tail.threshold ? (uint8_t)0 : (uint8_t)2;
        }
    }
}

// The cell pass.  A group of DP lanes per cell, lane = donor d.  acc = the ordered sum of (alt la + ref lb) over the row's entries at
// unmasked loci, (la, lb) = the table row of the donor's genotype (PAIR: of the anchor's and the donor's); then dn_tail.
template <int DP, bool PAIR>
__global__ __launch_bounds__(LANE_THREADS) void k_donor_e(uint64_t n_rows, uint32_t D, uint32_t W, const uint64_t *__restrict__ row_ptr,
                                                          const uint64_t *__restrict__ ent, const uint64_t *__restrict__ packed,
                                                          const double2 *__restrict__ tab, const uint8_t *__restrict__ mask /*or null*/,
                                                          const double *__restrict__ lp /*[D]*/, DonorTail tail, bool anchor_given,
                                                          uint8_t *__restrict__ anchor, double *__restrict__ s /*[rows][D]: !PAIR out, PAIR in*/,
                                                          uint8_t *__restrict__ best, uint8_t *__restrict__ second, uint32_t *__restrict__ cnt_out,
                                                          double *__restrict__ p_out, double *__restrict__ post, double *__restrict__ ppost,
                                                          double *__restrict__ dp_out, uint8_t *__restrict__ best_pair, uint8_t *__restrict__ status)
{
    const LaneGeom<DP> geo(n_rows, D);
    const int col = geo.col;
    const bool col_ok = geo.ok;
    const uint32_t my_word = col_ok ? (uint32_t)col >> 5 : 0u, my_shift = 2u * ((uint32_t)col & 31u);
    for (uint64_t g = geo.wave0; g < geo.n_groups; g += geo.n_waves) {
        const uint64_t row = geo.row(g);
        const bool have = row < n_rows;
        const uint64_t beg = have ? row_ptr[row] : 0, end = have ? row_ptr[row + 1] : 0;
        uint32_t a = 0;
        if (PAIR && have) a = anchor[row];
        if (a >= D) a = 0;  // (never: the host checks a given anchor, the singlet pass writes a donor)
        const uint32_t a_word = a >> 5, a_shift = 2u * (a & 31u);
        double acc = 0.0;
        uint32_t cnt = 0;
        // the entry loop of lane_rows.h: a fix here belongs in k_cluster_e, k_ambient_e, k_donor_fit, k_pair_fraction_e and k_donor_match as well
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
                    const uint32_t gd = (uint32_t)(packed[l * W + my_word] >> my_shift) & 3u;
                    if (PAIR) {
                        const uint32_t ga = (uint32_t)(packed[l * W + a_word] >> a_shift) & 3u;
                        t[q] = tab[l * 16 + 4 * ga + gd];
                    } else {
                        t[q] = tab[l * 4 + gd];
                    }
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
        dn_tail<DP, PAIR>(row, have, col, col_ok, geo.base, D, a, acc, cnt, lp, tail, anchor_given, anchor, s, best, second, cnt_out,
                          p_out, post, ppost, dp_out, best_pair, status);
    }
}

// ll[k][d] = the ordered sum over ascending unmasked loci of ((a la) + (r lb)), (a, r) the class' tallies, (la, lb) the singlet row of
// the donor's genotype.  Block k, lane d.
__global__ __launch_bounds__(64) void k_donor_match(uint64_t L, uint32_t D, uint32_t W, const unsigned long long *__restrict__ alt /*[K][L]*/,
                                                    const unsigned long long *__restrict__ ref, const uint64_t *__restrict__ packed,
                                                    const double2 *__restrict__ tab1, const uint8_t *__restrict__ mask /*or null*/,
                                                    double *__restrict__ ll /*[K][D]*/)
{
    const uint32_t k = blockIdx.x, d = threadIdx.x;
    if (d >= D) return;
    const uint32_t my_word = d >> 5, my_shift = 2u * (d & 31u);
    const unsigned long long *const ak = alt + (uint64_t)k * L, *const rk = ref + (uint64_t)k * L;
    double acc = 0.0;
    // the entry loop of lane_rows.h over loci: a fix here belongs in k_cluster_e, k_donor_e, k_donor_fit, k_ambient_e and k_pair_fraction_e as well
    for (uint64_t l0 = 0; l0 < L; l0 += LANE_AHEAD) {
        double av[LANE_AHEAD], rv[LANE_AHEAD];
        double2 t[LANE_AHEAD];
        bool use[LANE_AHEAD];
#pragma unroll
        for (int q = 0; q < LANE_AHEAD; q++) {
            const uint64_t l = l0 + q;
            use[q] = l < L && (!mask || mask[l] != 0);
            av[q] = rv[q] = 0.0;
            t[q] = make_double2(0.0, 0.0);
            if (use[q]) {
                av[q] = (double)ak[l];
                rv[q] = (double)rk[l];
                t[q] = tab1[l * 4 + ((uint32_t)(packed[l * W + my_word] >> my_shift) & 3u)];
            }
        }
#pragma unroll
        for (int q = 0; q < LANE_AHEAD; q++) {
            if (!use[q]) continue;
            const double pa = av[q] * t[q].x, pb = rv[q] * t[q].y;
            const double term = pa + pb;
            acc = acc + term;
        }
    }
    ll[(uint64_t)k * D + d] = acc;
}

// ---- genotype probabilities (cellector_donor_posteriors_gp, cellector_donor_weights, cellector_match_donors_gp) ------------------
// A donor's genotype at a locus is three weights, not one code.  include/cellector_ffi.h states the model; donors.py (soft_*) is
// its twin.
//   k_donor_weights  gp [D][total_loci][3] f32 -> w [L][D][3] f64 and kind [L][D] u8 over the used loci: kind 0, 1, 2 = the one-hot row
//                    of that genotype, 3 = no call, 4 = a soft row
//   k_donor_gp_e     k_donor_e's geometry and tail around a loop in three phases.  A lane's entry is a lookup (kind < 4:
//                    the hard call's bits) or the mixture over the genotypes of positive weight, m + log(sum w exp(t - m)).  The terms
//                    of LANE_AHEAD entries are formed first, the lookups of all four in flight together, then exp / log and all where
//                    a row is soft: they depend on nothing of the sum.  Then they are added in order.
//   k_donor_gp_match a lane per (class, donor), the same term from the class' tallies
#define DN_SOFT 4

// thread (l, d).  The host has validated every row; a row it should have refused is counted in bad and held as a no-call.
__global__ __launch_bounds__(LANE_THREADS) void k_donor_weights(uint64_t n /*L D*/, uint32_t D, uint64_t TL, const uint64_t *__restrict__ locus_ids,
                                                                const float *__restrict__ gp, double *__restrict__ w, uint8_t *__restrict__ kind,
                                                                uint32_t *__restrict__ bad)
{
    const uint64_t i = (uint64_t)blockIdx.x * LANE_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint64_t l = i / D, t = locus_ids[l];
    const uint32_t d = (uint32_t)(i % D);
    double w0 = 0.0, w1 = 0.0, w2 = 0.0;
    uint8_t k = 3;
    if (t < TL) {
        const float *row = gp + ((uint64_t)d * TL + t) * 3;
        const float f0 = row[0], f1 = row[1], f2 = row[2];
        const bool none = f0 != f0 && f1 != f1 && f2 != f2;
        const bool fine = f0 >= 0.f && f1 >= 0.f && f2 >= 0.f && f0 < INFINITY && f1 < INFINITY && f2 < INFINITY && (f0 > 0.f || f1 > 0.f || f2 > 0.f);
        if (fine) {
            const double x0 = (double)f0, x1 = (double)f1, x2 = (double)f2;
            const double s01 = x0 + x1;
            const double sum = s01 + x2;
            w0 = x0 / sum; w1 = x1 / sum; w2 = x2 / sum;
            const int pos = (f0 > 0.f) + (f1 > 0.f) + (f2 > 0.f);
            k = pos > 1 ? (uint8_t)DN_SOFT : f0 > 0.f ? (uint8_t)0 : f1 > 0.f ? (uint8_t)1 : (uint8_t)2;  // (one positive: x / x is 1.0)
        } else if (!none) {
            atomicAdd(bad, 1u);
        }
    }
    w[i * 3] = w0; w[i * 3 + 1] = w1; w[i * 3 + 2] = w2;
    kind[i] = k;
}

// the weights of a row over the four table rows: a one-hot row or a no-call is weight 1.0 on its own row
__device__ __forceinline__ void dn_row_weights(uint32_t k, const double *__restrict__ w3, double (&out)[4])
{
#pragma unroll
    for (uint32_t g = 0; g < 4; g++) out[g] = k < DN_SOFT ? (k == g ? 1.0 : 0.0) : g < 3 ? w3[g] : 0.0;
}

// the table row a lookup reads: of the donor's kind (PAIR: of the anchor's and the donor's); a soft row reads row 3 and its term is
// replaced by dn_gp_soft's
template <bool PAIR>
__device__ __forceinline__ uint64_t dn_gp_row(uint64_t l, uint32_t ka, uint32_t kd)
{
    const uint32_t ga = ka < 3u ? ka : 3u, gd = kd < 3u ? kd : 3u;
    return PAIR ? l * 16 + 4 * ga + gd : l * 4 + gd;
}

// one entry's mixture term for donor d of kind kd (PAIR: with anchor a of kind ka; one of the two is soft) at locus l under the counts
// (al, re)
template <bool PAIR>
__device__ __forceinline__ double dn_gp_soft(uint64_t l, uint32_t D, uint32_t d, uint32_t a, uint32_t ka, uint32_t kd,
                                             const double *__restrict__ w, const double2 *__restrict__ tab, double al, double re)
{
    if (!PAIR) {
        const double *w3 = w + (l * D + d) * 3;
        double wg[3], tg[3], m = -INFINITY;
#pragma unroll
        for (int g = 0; g < 3; g++) {
            wg[g] = w3[g];
            const double2 t = tab[l * 4 + g];
            const double pa = al * t.x, pb = re * t.y;
            tg[g] = pa + pb;
            if (wg[g] > 0.0 && tg[g] > m) m = tg[g];
        }
        double z = 0.0;
#pragma unroll
        for (int g = 0; g < 3; g++) {
            if (!(wg[g] > 0.0)) continue;
            const double dg = tg[g] - m;
            const double e = exp(dg);
            const double we = wg[g] * e;
            z = z + we;
        }
        const double lz = log(z);
        return m + lz;
    } else {
        double wa[4], wd[4], tt[16], m = -INFINITY;
        dn_row_weights(ka, w + (l * D + a) * 3, wa);
        dn_row_weights(kd, w + (l * D + d) * 3, wd);
#pragma unroll
        for (int g = 0; g < 4; g++)
#pragma unroll
            for (int h = 0; h < 4; h++) {
                tt[4 * g + h] = 0.0;
                if (!(wa[g] > 0.0 && wd[h] > 0.0)) continue;
                const double2 t = tab[l * 16 + 4 * g + h];
                const double pa = al * t.x, pb = re * t.y;
                tt[4 * g + h] = pa + pb;
                if (tt[4 * g + h] > m) m = tt[4 * g + h];
            }
        double z = 0.0;
#pragma unroll
        for (int g = 0; g < 4; g++)
#pragma unroll
            for (int h = 0; h < 4; h++) {
                if (!(wa[g] > 0.0 && wd[h] > 0.0)) continue;
                const double ww = wa[g] * wd[h];
                const double dg = tt[4 * g + h] - m;
                const double e = exp(dg);
                const double we = ww * e;
                z = z + we;
            }
        const double lz = log(z);
        return m + lz;
    }
}

template <int DP, bool PAIR>
__global__ __launch_bounds__(LANE_THREADS) void k_donor_gp_e(uint64_t n_rows, uint32_t D, const uint64_t *__restrict__ row_ptr,
                                                             const uint64_t *__restrict__ ent, const double *__restrict__ w /*[L][D][3]*/,
                                                             const uint8_t *__restrict__ kind /*[L][D]*/, const double2 *__restrict__ tab,
                                                             const uint8_t *__restrict__ mask /*or null*/, const double *__restrict__ lp /*[D]*/,
                                                             DonorTail tail, bool anchor_given, uint8_t *__restrict__ anchor,
                                                             double *__restrict__ s /*[rows][D]: !PAIR out, PAIR in*/, uint8_t *__restrict__ best,
                                                             uint8_t *__restrict__ second, uint32_t *__restrict__ cnt_out, double *__restrict__ p_out,
                                                             double *__restrict__ post, double *__restrict__ ppost, double *__restrict__ dp_out,
                                                             uint8_t *__restrict__ best_pair, uint8_t *__restrict__ status)
{
    const LaneGeom<DP> geo(n_rows, D);
    const int col = geo.col;
    const bool col_ok = geo.ok;
    for (uint64_t g = geo.wave0; g < geo.n_groups; g += geo.n_waves) {
        const uint64_t row = geo.row(g);
        const bool have = row < n_rows;
        const uint64_t beg = have ? row_ptr[row] : 0, end = have ? row_ptr[row + 1] : 0;
        uint32_t a = 0;
        if (PAIR && have) a = anchor[row];
        if (a >= D) a = 0;  // (never: the host checks a given anchor, the singlet pass writes a donor)
        const bool mine = PAIR && col_ok && (uint32_t)col == a;  // the anchor's own column: a copy of its singlet sum, no pair
        double acc = 0.0;
        uint32_t cnt = 0;
        for (uint64_t i = beg; i < end; i += LANE_AHEAD) {
            uint64_t en[LANE_AHEAD];
            uint32_t ka[LANE_AHEAD], kd[LANE_AHEAD];
            double term[LANE_AHEAD];
            bool use[LANE_AHEAD], live[LANE_AHEAD];
            // the kinds, then the lookups of all four entries (k_donor_e's loads, in flight together), then the mixtures where a row is soft
#pragma unroll
            for (int q = 0; q < LANE_AHEAD; q++) {
                const bool in = i + q < end;
                en[q] = in ? ent[i + q] : 0ull;
                const uint64_t l = ENT_IDX(en[q]);
                use[q] = in && (!mask || mask[l] != 0);
                live[q] = use[q] && col_ok && !mine;
                kd[q] = live[q] ? kind[l * D + (uint32_t)col] : 0u;
                ka[q] = PAIR && live[q] ? kind[l * D + a] : 0u;
            }
#pragma unroll
            for (int q = 0; q < LANE_AHEAD; q++) {
                double2 t = make_double2(0.0, 0.0);
                if (live[q]) t = tab[dn_gp_row<PAIR>(ENT_IDX(en[q]), ka[q], kd[q])];
                const double pa = (double)ENT_ALT(en[q]) * t.x, pb = (double)ENT_REF(en[q]) * t.y;
                term[q] = pa + pb;
            }
#pragma unroll
            for (int q = 0; q < LANE_AHEAD; q++)
                if (live[q] && (kd[q] == DN_SOFT || ka[q] == DN_SOFT))
                    term[q] = dn_gp_soft<PAIR>(ENT_IDX(en[q]), D, (uint32_t)col, a, ka[q], kd[q], w, tab, (double)ENT_ALT(en[q]), (double)ENT_REF(en[q]));
#pragma unroll
            for (int q = 0; q < LANE_AHEAD; q++) {
                if (!use[q]) continue;
                acc = acc + term[q];
                cnt++;
            }
        }
        if (mine && have) acc = s[row * D + col];
        dn_tail<DP, PAIR>(row, have, col, col_ok, geo.base, D, a, acc, cnt, lp, tail, anchor_given, anchor, s, best, second, cnt_out,
                          p_out, post, ppost, dp_out, best_pair, status);
    }
}

// ll[k][d] = the ordered sum over ascending unmasked loci of the singlet term under the class' tallies.  Block k, lane d.
__global__ __launch_bounds__(64) void k_donor_gp_match(uint64_t L, uint32_t D, const unsigned long long *__restrict__ alt /*[K][L]*/,
                                                       const unsigned long long *__restrict__ ref, const double *__restrict__ w,
                                                       const uint8_t *__restrict__ kind, const double2 *__restrict__ tab1,
                                                       const uint8_t *__restrict__ mask /*or null*/, double *__restrict__ ll /*[K][D]*/)
{
    const uint32_t k = blockIdx.x, d = threadIdx.x;
    if (d >= D) return;
    const unsigned long long *const ak = alt + (uint64_t)k * L, *const rk = ref + (uint64_t)k * L;
    double acc = 0.0;
    for (uint64_t l0 = 0; l0 < L; l0 += LANE_AHEAD) {
        double av[LANE_AHEAD], rv[LANE_AHEAD], term[LANE_AHEAD];
        uint32_t kd[LANE_AHEAD];
        bool use[LANE_AHEAD];
#pragma unroll
        for (int q = 0; q < LANE_AHEAD; q++) {
            const uint64_t l = l0 + q;
            use[q] = l < L && (!mask || mask[l] != 0);
            av[q] = use[q] ? (double)ak[l] : 0.0;
            rv[q] = use[q] ? (double)rk[l] : 0.0;
            kd[q] = use[q] ? kind[l * D + d] : 0u;
        }
#pragma unroll
        for (int q = 0; q < LANE_AHEAD; q++) {
            double2 t = make_double2(0.0, 0.0);
            if (use[q]) t = tab1[dn_gp_row<false>(l0 + q, 0u, kd[q])];
            const double pa = av[q] * t.x, pb = rv[q] * t.y;
            term[q] = pa + pb;
        }
#pragma unroll
        for (int q = 0; q < LANE_AHEAD; q++)
            if (use[q] && kd[q] == DN_SOFT) term[q] = dn_gp_soft<false>(l0 + q, D, d, 0u, 0u, kd[q], w, tab1, av[q], rv[q]);
#pragma unroll
        for (int q = 0; q < LANE_AHEAD; q++) {
            if (!use[q]) continue;
            acc = acc + term[q];
        }
    }
    ll[(uint64_t)k * D + d] = acc;
}

// ---- the fit of the called hypothesis (cellector_donor_fit, cellector_donor_moment_tables) -----------------------------------------
// The softmax of the donor call sums to 1 whoever the cell is: a cell of a donor nobody genotyped gets a confident call for something
// else.  Under its called hypothesis an entry's term (a log theta + r log(1 - theta)) is n = a + r times a per-(locus, genotype)
// constant in its mean and in its variance, so the expected sum and its variance are two more table rows and two more ordered sums
// per lane.  include/cellector_ffi.h states the model; donors.py (moment_tables, fit_sums, fit) is its twin.
//   k_donor_moments  mom1 [L][4] and mom2 [L][16] double2 = (h, v), thread (l, 4 ga + gb) as k_donor_tables
//   k_donor_fit      one walk of the row, lane = donor: E, V from mom1, PE, PV from mom2 under the donor call's anchor; the tail forms
//                    z, pz from the donor call's own s and p, the called hypothesis and its z

// theta and rest by k_donor_tables' own operations; la = log(th), lb = log(rest); h = (th la) + (rest lb); d = la - lb;
// v = (th rest) (d d).  The diagonal is mom1.  A masked locus carries (0, 0).
__global__ __launch_bounds__(LANE_THREADS) void k_donor_moments(uint64_t n /*16 L*/, const double *__restrict__ s_alt, const double *__restrict__ s_ref,
                                                                const uint8_t *__restrict__ mask /*or null*/, double err, double ambient,
                                                                double2 *__restrict__ mom1, double2 *__restrict__ mom2)
{
    const uint64_t i = (uint64_t)blockIdx.x * LANE_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint64_t l = i >> 4;
    const uint32_t ga = (uint32_t)(i >> 2) & 3u, gb = (uint32_t)i & 3u;
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
        const double sum = ta + tb;
        const double th = 0.5 * sum;
        const double rest = 1.0 - th;
        const double la = log(th), lb = log(rest);
        const double ha = th * la, hb = rest * lb;
        const double h = ha + hb;
        const double d = la - lb;
        const double tr = th * rest, dd = d * d;
        out = make_double2(h, tr * dd);
    }
    mom2[i] = out;
    if (ga == gb) mom1[l * 4 + ga] = out;
}

// The fit pass.  k_donor_e's geometry: a group of DP lanes per cell, lane = donor d.  Four ordered sums per lane over the row's entries
// at unmasked loci, n = (double)(alt + ref): E += n h, V += n v from mom1's row of the donor's genotype, PE, PV likewise from mom2's row
// of (the anchor's, the donor's).  Tail: z = (s - E) / sqrt(V), pz = (p - PE) / sqrt(PV), 0.0 where the variance is 0.0; the called
// hypothesis is (anchor, best_pair) under status 1 and (best, none) otherwise, its z is shuffled from the lane that holds it.
template <int DP>
__global__ __launch_bounds__(LANE_THREADS) void k_donor_fit(uint64_t n_rows, uint32_t D, uint32_t W, const uint64_t *__restrict__ row_ptr,
                                                            const uint64_t *__restrict__ ent, const uint64_t *__restrict__ packed,
                                                            const double2 *__restrict__ mom1, const double2 *__restrict__ mom2,
                                                            const uint8_t *__restrict__ mask /*or null*/, const uint8_t *__restrict__ anchor,
                                                            const double *__restrict__ s, const double *__restrict__ p,
                                                            const uint8_t *__restrict__ best, const uint8_t *__restrict__ best_pair,
                                                            const uint8_t *__restrict__ status, double *__restrict__ e_out,
                                                            double *__restrict__ v_out, double *__restrict__ pe_out, double *__restrict__ pv_out,
                                                            double *__restrict__ z_out, double *__restrict__ pz_out, double *__restrict__ call_z,
                                                            uint8_t *__restrict__ hyp_a, uint8_t *__restrict__ hyp_b)
{
    const LaneGeom<DP> geo(n_rows, D);
    const int col = geo.col;
    const bool col_ok = geo.ok;
    const uint32_t my_word = col_ok ? (uint32_t)col >> 5 : 0u, my_shift = 2u * ((uint32_t)col & 31u);
    for (uint64_t g = geo.wave0; g < geo.n_groups; g += geo.n_waves) {
        const uint64_t row = geo.row(g);
        const bool have = row < n_rows;
        const uint64_t beg = have ? row_ptr[row] : 0, end = have ? row_ptr[row + 1] : 0;
        uint32_t a = have ? anchor[row] : 0u;
        if (a >= D) a = 0;  // (never: the donor call checked a given anchor, or wrote a donor)
        const uint32_t a_word = a >> 5, a_shift = 2u * (a & 31u);
        double E = 0.0, V = 0.0, PE = 0.0, PV = 0.0;
        // the entry loop of lane_rows.h: a fix here belongs in k_donor_e, k_cluster_e, k_ambient_e, k_pair_fraction_e and k_donor_match as well
        for (uint64_t i = beg; i < end; i += LANE_AHEAD) {
            uint64_t en[LANE_AHEAD];
            double2 t1[LANE_AHEAD], t2[LANE_AHEAD];
            bool use[LANE_AHEAD];
#pragma unroll
            for (int q = 0; q < LANE_AHEAD; q++) {
                const bool in = i + q < end;
                en[q] = in ? ent[i + q] : 0ull;
                const uint64_t l = ENT_IDX(en[q]);
                use[q] = in && (!mask || mask[l] != 0);
                t1[q] = t2[q] = make_double2(0.0, 0.0);
                if (use[q] && col_ok) {
                    const uint32_t gd = (uint32_t)(packed[l * W + my_word] >> my_shift) & 3u;
                    const uint32_t ga = (uint32_t)(packed[l * W + a_word] >> a_shift) & 3u;
                    t1[q] = mom1[l * 4 + gd];
                    t2[q] = mom2[l * 16 + 4 * ga + gd];
                }
            }
#pragma unroll
            for (int q = 0; q < LANE_AHEAD; q++) {
                if (!use[q]) continue;
                const double n = (double)(ENT_ALT(en[q]) + ENT_REF(en[q]));
                const double eh = n * t1[q].x, ev = n * t1[q].y, ph = n * t2[q].x, pv = n * t2[q].y;
                E = E + eh;
                V = V + ev;
                PE = PE + ph;
                PV = PV + pv;
            }
        }
        // the tail: every lane of the wave takes part in the shuffles; a lane without a row or a column carries 0.0
        double z = 0.0, pz = 0.0;
        if (have && col_ok) {
            const uint64_t at = row * D + col;
            if (V != 0.0) {
                const double diff = s[at] - E, sd = sqrt(V);
                z = diff / sd;
            }
            if (PV != 0.0) {
                const double diff = p[at] - PE, sd = sqrt(PV);
                pz = diff / sd;
            }
            e_out[at] = E; v_out[at] = V; pe_out[at] = PE; pv_out[at] = PV;
            z_out[at] = z; pz_out[at] = pz;
        }
        const uint32_t st = have ? status[row] : (uint32_t)DN_NONE;
        uint32_t b = have ? best[row] : 0u, bp = have ? best_pair[row] : 0u;
        if (b >= D) b = 0;
        if (bp >= D) bp = 0;  // (D = 1 has no pair and never status 1)
        const double zb = __shfl(z, (geo.base + (int)b) & 63, 64), zp = __shfl(pz, (geo.base + (int)bp) & 63, 64);
        if (have && col == 0) {
            const bool pair = st == 1u;
            call_z[row] = st == (uint32_t)DN_NONE ? 0.0 : pair ? zp : zb;
            hyp_a[row] = pair ? (uint8_t)a : (uint8_t)b;
            hyp_b[row] = pair ? (uint8_t)bp : (uint8_t)DN_NONE;
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
namespace {

// the scratch of one call; alloc() makes all of it before anything is launched
struct DonorRun {
    cellector_ctx *c;
    uint32_t D, W;
    uint64_t n, L, TL;
    DevBuf<uint8_t> gt;             // [D][TL]
    LociMask mask;                  // [L]
    DevBuf<uint64_t> packed;        // [L][W]
    DevBuf<double2> tab1, tab2;     // [L][4], [L][16]
    DevBuf<double> lp;              // [D]
    DevBuf<double> s, p, post, ppost;  // [n][D]
    DevBuf<double> dp;              // [n]
    DevBuf<uint8_t> anchor, best, second, best_pair, status;  // [n]
    DevBuf<uint32_t> cnt;           // [n]
    DevBuf<unsigned long long> alt, ref;  // [K][L] the class tallies (match)
    DevBuf<double> ll;              // [K][D]
    DevBuf<float> gp;               // [D][TL][3] the soft calls: in place of gt and packed
    DevBuf<double> w;               // [L][D][3]
    DevBuf<uint8_t> kind;           // [L][D]
    DevBuf<uint32_t> bad;           // [1]
    bool soft = false;
    EventMarks<3> ev;               // before the singlet pass, between the two passes, behind the pair pass

    cellector_status alloc(bool cells, uint32_t K, bool soft_calls = false)
    {
        soft = soft_calls;
        if (soft) {
            CHK(dev_alloc(c, &gp, (uint64_t)D * TL * 3));
            CHK(dev_alloc(c, &w, L * D * 3));
            CHK(dev_alloc(c, &kind, L * D));
            CHK(dev_alloc(c, &bad, 1));
        } else {
            CHK(dev_alloc(c, &gt, (uint64_t)D * TL));
            CHK(dev_alloc(c, &packed, L * W));
        }
        CHK(dev_alloc(c, &mask.buf, L));
        CHK(dev_alloc(c, &tab1, L * 4));
        CHK(dev_alloc(c, &tab2, L * 16));
        if (cells) {
            const uint64_t nD = n * D;
            CHK(dev_alloc(c, &lp, D));
            CHK(dev_alloc(c, &s, nD)); CHK(dev_alloc(c, &p, nD)); CHK(dev_alloc(c, &post, nD)); CHK(dev_alloc(c, &ppost, nD));
            CHK(dev_alloc(c, &dp, n));
            CHK(dev_alloc(c, &anchor, n)); CHK(dev_alloc(c, &best, n)); CHK(dev_alloc(c, &second, n));
            CHK(dev_alloc(c, &best_pair, n)); CHK(dev_alloc(c, &status, n));
            CHK(dev_alloc(c, &cnt, n));
        }
        if (K) {
            CHK(dev_alloc(c, &alt, (uint64_t)K * L)); CHK(dev_alloc(c, &ref, (uint64_t)K * L));
            CHK(dev_alloc(c, &ll, (uint64_t)K * D));
        }
        return CELLECTOR_OK;
    }

    // one upload of the calls (gt [D][TL] u8, or gp [D][TL][3] f32 of a soft run), the packing or the weights, and the tables
    cellector_status prepare(const void *host_calls, const uint8_t *host_mask, const cellector_donor_params *prm)
    {
        CHK(mask.set(c, host_mask, L));
        if (soft) HIPCHK(c, hipMemsetAsync(bad, 0, 4, c->stream));
        if (!L) return CELLECTOR_OK;
        if (soft) {
            HIPCHK(c, hipMemcpyAsync(gp, host_calls, (uint64_t)D * TL * 12, hipMemcpyHostToDevice, c->stream));
            hipLaunchKernelGGL(k_donor_weights, dim3(lane_grid(L * D, LANE_THREADS, 0x7fffffffu)), dim3(LANE_THREADS), 0, c->stream, L * D, D, TL,
                               c->locus_ids.get(), gp.get(), w.get(), kind.get(), bad.get());
        } else {
            HIPCHK(c, hipMemcpyAsync(gt, host_calls, (uint64_t)D * TL, hipMemcpyHostToDevice, c->stream));
            hipLaunchKernelGGL(k_donor_pack, dim3(lane_grid(L * W, LANE_THREADS, 0x7fffffffu)), dim3(LANE_THREADS), 0, c->stream, L * W, D, W, TL,
                               c->locus_ids.get(), gt.get(), packed.get());
        }
        HIPCHK(c, hipGetLastError());
        return donor_tables_launch(c, mask.get(), prm, tab1.get(), tab2.get());
    }

    cellector_status pass(bool pair, bool anchor_given, const DonorTail &tail)
    {
        if (!n) return CELLECTOR_OK;
        if (pair) launch_pass(std::true_type(), anchor_given, tail);
        else launch_pass(std::false_type(), anchor_given, tail);
        HIPCHK(c, hipGetLastError());
        return CELLECTOR_OK;
    }

    // the one launch of a pass: the hard or the soft kernel at the run's width
    template <typename Pair>
    void launch_pass(Pair, bool anchor_given, const DonorTail &tail)
    {
        constexpr bool PAIR = Pair::value;
        const int dpw = lane_width(D, 2);
        const dim3 grid(lane_walk_grid(n, dpw, c->n_cu)), block(LANE_THREADS);
        const double2 *tab = PAIR ? tab2.get() : tab1.get();
        lane_dispatch<2, 64>(dpw, [&](auto DP) {
            if (soft)
                hipLaunchKernelGGL((k_donor_gp_e<DP, PAIR>), grid, block, 0, c->stream, n, D, c->csr_ptr.get(), c->csr_ent.get(), w.get(),
                                   kind.get(), tab, mask.get(), lp.get(), tail, anchor_given, anchor.get(), s.get(), best.get(), second.get(),
                                   cnt.get(), p.get(), post.get(), ppost.get(), dp.get(), best_pair.get(), status.get());
            else
                hipLaunchKernelGGL((k_donor_e<DP, PAIR>), grid, block, 0, c->stream, n, D, W, c->csr_ptr.get(), c->csr_ent.get(), packed.get(),
                                   tab, mask.get(), lp.get(), tail, anchor_given, anchor.get(), s.get(), best.get(), second.get(), cnt.get(),
                                   p.get(), post.get(), ppost.get(), dp.get(), best_pair.get(), status.get());
        });
    }

    // the donor call on the device: the uploads, the tables and the two passes; everything stays in the run's buffers
    cellector_status cells(const void *host_calls, const cellector_donor_params *prm, const double *log_prior, const uint8_t *host_anchor,
                           const uint8_t *host_mask, double log_singlet, double log_pair)
    {
        const DonorTail tail = {log_singlet, log_pair, prm->posterior_threshold, prm->min_loci};
        cellector_status st = prepare(host_calls, host_mask, prm);
        if (st == CELLECTOR_OK && hipMemcpyAsync(lp, log_prior, (uint64_t)D * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess)
            st = ctx_fail(c, CELLECTOR_EDEVICE, "donor_posteriors: the upload of the priors failed");
        if (st == CELLECTOR_OK && host_anchor && n && hipMemcpyAsync(anchor, host_anchor, n, hipMemcpyHostToDevice, c->stream) != hipSuccess)
            st = ctx_fail(c, CELLECTOR_EDEVICE, "donor_posteriors: the upload of the anchors failed");
        ev.mark(0, c->stream);
        if (st == CELLECTOR_OK) st = pass(false, host_anchor != nullptr, tail);
        ev.mark(1, c->stream);
        if (st == CELLECTOR_OK) st = pass(true, host_anchor != nullptr, tail);
        ev.mark(2, c->stream);
        return st;
    }

    // a soft run: the weights as the device holds them, and the kernel's own count of rows the host's check should have refused
    cellector_status fetch_weights(double *h_w, uint8_t *h_kind)
    {
        uint32_t h_bad = 0;
        CHK(d2h(c, &h_bad, bad, 4));
        if (h_w) CHK(d2h(c, h_w, w, L * D * 3 * 8));
        if (h_kind) CHK(d2h(c, h_kind, kind, L * D));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (h_bad) return ctx_fail(c, CELLECTOR_EDEVICE, "donor weights: %u rows of gp are invalid on the device", h_bad);
        return CELLECTOR_OK;
    }

    cellector_status fetch_tables(double *h_tab1, double *h_tab2, uint64_t *h_packed)
    {
        if (h_tab1) CHK(d2h(c, h_tab1, tab1, L * 4 * 16));
        if (h_tab2) CHK(d2h(c, h_tab2, tab2, L * 16 * 16));
        if (h_packed) CHK(d2h(c, h_packed, packed, L * W * 8));
        return CELLECTOR_OK;
    }
};

}  // namespace

// the packing alone, for the calls of other files that score cells against packed genotypes (kernels_ambient.hip): d_gt [D][TL] and
// d_packed [L][W] on the device
cellector_status donor_pack_launch(cellector_ctx *c, uint32_t D, const uint8_t *d_gt, uint64_t *d_packed)
{
    const uint32_t W = (D + 31) / 32;
    if (!c->L) return CELLECTOR_OK;
    hipLaunchKernelGGL(k_donor_pack, dim3(lane_grid(c->L * W, LANE_THREADS, 0x7fffffffu)), dim3(LANE_THREADS), 0, c->stream, c->L * W, D, W,
                       c->total_loci, c->locus_ids.get(), d_gt, d_packed);
    HIPCHK(c, hipGetLastError());
    return CELLECTOR_OK;
}

// the tables alone, for the donor panel (kernels_donor_panel.hip): d_mask [L] or null, d_tab1 [L][4] and d_tab2 [L][16] on the device
cellector_status donor_tables_launch(cellector_ctx *c, const uint8_t *d_mask, const cellector_donor_params *prm, double2 *d_tab1, double2 *d_tab2)
{
    if (!c->L) return CELLECTOR_OK;
    hipLaunchKernelGGL(k_donor_tables, dim3(lane_grid(c->L * 16, LANE_THREADS, 0x7fffffffu)), dim3(LANE_THREADS), 0, c->stream, c->L * 16,
                       c->s_alt.get(), c->s_ref.get(), d_mask, prm->err, prm->ambient, d_tab1, d_tab2);
    HIPCHK(c, hipGetLastError());
    return CELLECTOR_OK;
}

// cellector_donor_tables: validated arguments; host outputs, any may be null
cellector_status donor_tables_run(cellector_ctx *c, const uint8_t *gt, uint32_t D, const cellector_donor_params *prm, const uint8_t *mask,
                                  double *tab1, double *tab2, uint64_t *packed)
{
    DonorRun r{c, D, (D + 31) / 32, c->nloc, c->L, c->total_loci};
    CHK(r.alloc(false, 0));
    invalidate_cell_ll_state(c);
    cellector_status st = r.prepare(gt, mask, prm);
    if (st == CELLECTOR_OK) st = r.fetch_tables(tab1, tab2, packed);
    (void)hipStreamSynchronize(c->stream);  // (nothing of the scratch may be in use when it goes)
    return st;
}

// cellector_donor_weights: validated arguments; host outputs, any may be null
cellector_status donor_weights_run(cellector_ctx *c, const float *gp, uint32_t D, double *w, uint8_t *kind)
{
    DonorRun r{c, D, (D + 31) / 32, c->nloc, c->L, c->total_loci};
    CHK(r.alloc(false, 0, true));
    invalidate_cell_ll_state(c);
    cellector_donor_params prm;
    cellector_donor_default_params(&prm);
    cellector_status st = r.prepare(gp, nullptr, &prm);
    if (st == CELLECTOR_OK) st = r.fetch_weights(w, kind);
    (void)hipStreamSynchronize(c->stream);
    return st;
}

// cellector_donor_posteriors: validated arguments (log_prior never null: the caller's or zeros); host outputs, any may be null
// (gp: the soft calls, then gt is not read and packed stays null)
cellector_status donor_posteriors_run(cellector_ctx *c, const uint8_t *gt, const float *gp, uint32_t D, const cellector_donor_params *prm, const double *log_prior,
                                      const uint8_t *anchor, const uint8_t *mask, double log_singlet, double log_pair, double *ll,
                                      double *pair_ll, double *posterior, double *pair_posterior, double *doublet_posterior, uint8_t *best,
                                      uint8_t *second, uint8_t *best_pair, uint32_t *n_entries, uint8_t *status, uint8_t *anchor_out,
                                      cellector_donor_summary *out, double *tab1, double *tab2, uint64_t *packed)
{
    LapTimer whole;
    DonorRun r{c, D, (D + 31) / 32, c->nloc, c->L, c->total_loci};
    const uint64_t n = r.n;
    CHK(r.alloc(true, 0, gp != nullptr));
    std::vector<uint8_t> h_status(n), h_best(n);
    invalidate_cell_ll_state(c);
    cellector_status st = r.cells(gp ? (const void *)gp : (const void *)gt, prm, log_prior, anchor, mask, log_singlet, log_pair);
    const uint64_t nD = n * D;
    if (st == CELLECTOR_OK && ll) st = d2h(c, ll, r.s, nD * 8);
    if (st == CELLECTOR_OK && pair_ll) st = d2h(c, pair_ll, r.p, nD * 8);
    if (st == CELLECTOR_OK && posterior) st = d2h(c, posterior, r.post, nD * 8);
    if (st == CELLECTOR_OK && pair_posterior) st = d2h(c, pair_posterior, r.ppost, nD * 8);
    if (st == CELLECTOR_OK && doublet_posterior) st = d2h(c, doublet_posterior, r.dp, n * 8);
    if (st == CELLECTOR_OK) st = d2h(c, h_best.data(), r.best, n);
    if (st == CELLECTOR_OK && second) st = d2h(c, second, r.second, n);
    if (st == CELLECTOR_OK && best_pair) st = d2h(c, best_pair, r.best_pair, n);
    if (st == CELLECTOR_OK && n_entries) st = d2h(c, n_entries, r.cnt, n * 4);
    if (st == CELLECTOR_OK) st = d2h(c, h_status.data(), r.status, n);
    if (st == CELLECTOR_OK && anchor_out) st = d2h(c, anchor_out, r.anchor, n);
    if (st == CELLECTOR_OK) st = r.fetch_tables(tab1, tab2, gp ? nullptr : packed);
    if (st == CELLECTOR_OK && gp) st = r.fetch_weights(nullptr, nullptr);
    (void)hipStreamSynchronize(c->stream);
    float ms1 = 0.f, ms2 = 0.f;
    if (st == CELLECTOR_OK && r.ev.ms(0, 1, &ms1) && r.ev.ms(1, 2, &ms2))
        fprintf(stderr, "[timing]   donors%s: D %u singlet pass %.3f ms, pair pass %.3f ms, whole call %.4f s\n", gp ? " (gp)" : "", D, ms1, ms2, whole.lap());
    if (st != CELLECTOR_OK) return st;
    cellector_donor_summary sum = {};
    for (uint64_t i = 0; i < n; i++) {
        switch (h_status[i]) {
        case 0: sum.n_singlet++; sum.donor_cells[h_best[i] < 64 ? h_best[i] : 0]++; break;
        case 1: sum.n_doublet++; break;
        case 2: sum.n_ambiguous++; break;
        default: sum.n_unassigned++; break;
        }
    }
    if (best && n) memcpy(best, h_best.data(), n);
    if (status && n) memcpy(status, h_status.data(), n);
    if (out) *out = sum;
    return CELLECTOR_OK;
}

// cellector_match_donors: validated arguments; the tallies are cellector_class_tallies' own; host outputs, any may be null
cellector_status donor_match_run(cellector_ctx *c, const uint8_t *labels, uint32_t K, const uint8_t *gt, const float *gp, uint32_t D,
                                 const cellector_donor_params *prm, const uint8_t *mask, double *ll, uint8_t *best, double *margin,
                                 uint64_t *cells)
{
    DonorRun r{c, D, (D + 31) / 32, c->nloc, c->L, c->total_loci};
    const uint64_t L = r.L;
    CHK(r.alloc(false, K, gp != nullptr));
    std::vector<uint64_t> h_alt((uint64_t)K * L), h_ref((uint64_t)K * L), h_cells(K);
    std::vector<double> h_ll((uint64_t)K * D, 0.0);
    CHK(classes_tallies_run(c, labels, K, nullptr, h_cells.data(), h_alt.data(), h_ref.data(), nullptr, nullptr));
    invalidate_cell_ll_state(c);
    cellector_status st = r.prepare(gp ? (const void *)gp : (const void *)gt, mask, prm);
    if (st == CELLECTOR_OK && L) {
        if (hipMemcpyAsync(r.alt, h_alt.data(), (uint64_t)K * L * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            hipMemcpyAsync(r.ref, h_ref.data(), (uint64_t)K * L * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess)
            st = ctx_fail(c, CELLECTOR_EDEVICE, "match_donors: the upload of the tallies failed");
    }
    if (st == CELLECTOR_OK) {
        if (gp)
            hipLaunchKernelGGL(k_donor_gp_match, dim3(K), dim3(64), 0, c->stream, L, D, r.alt.get(), r.ref.get(), r.w.get(), r.kind.get(),
                               r.tab1.get(), r.mask.get(), r.ll.get());
        else
            hipLaunchKernelGGL(k_donor_match, dim3(K), dim3(64), 0, c->stream, L, D, r.W, r.alt.get(), r.ref.get(), r.packed.get(),
                               r.tab1.get(), r.mask.get(), r.ll.get());
        if (hipGetLastError() != hipSuccess) st = ctx_fail(c, CELLECTOR_EDEVICE, "match_donors: launch failed");
    }
    if (st == CELLECTOR_OK) st = d2h(c, h_ll.data(), r.ll, (uint64_t)K * D * 8);
    if (st == CELLECTOR_OK && gp) st = r.fetch_weights(nullptr, nullptr);
    (void)hipStreamSynchronize(c->stream);
    if (st != CELLECTOR_OK) return st;
    for (uint32_t k = 0; k < K; k++) {
        const double *row = h_ll.data() + (uint64_t)k * D;
        uint32_t b = 0, b2 = DN_NONE;
        for (uint32_t d = 1; d < D; d++)
            if (row[d] > row[b]) b = d;
        for (uint32_t d = 0; d < D; d++)
            if (d != b && (b2 == DN_NONE || row[d] > row[b2])) b2 = d;
        const bool live = h_cells[k] > 0;
        if (best) best[k] = live ? (uint8_t)b : (uint8_t)DN_NONE;
        if (margin) margin[k] = !live ? 0.0 : b2 == DN_NONE ? INFINITY : row[b] - row[b2];
        if (cells) cells[k] = h_cells[k];
    }
    if (ll) memcpy(ll, h_ll.data(), h_ll.size() * 8);
    return CELLECTOR_OK;
}

// ---- cellector_donor_fit, cellector_donor_moment_tables ----------------------------------------------------------------------------
namespace {

// the scratch of a fit beside the donor run's; alloc() makes all of it before anything is launched
struct FitRun {
    DevBuf<double2> mom1, mom2;         // [L][4], [L][16]
    DevBuf<double> e, v, pe, pv, z, pz; // [n][D]
    DevBuf<double> cz, keys;            // [n]
    DevBuf<uint8_t> ha, hb;             // [n]

    cellector_status alloc(cellector_ctx *c, uint64_t L, uint64_t n, uint32_t D, bool cells)
    {
        CHK(dev_alloc(c, &mom1, L * 4));
        CHK(dev_alloc(c, &mom2, L * 16));
        if (cells) {
            const uint64_t nD = n * D;
            CHK(dev_alloc(c, &e, nD)); CHK(dev_alloc(c, &v, nD)); CHK(dev_alloc(c, &pe, nD)); CHK(dev_alloc(c, &pv, nD));
            CHK(dev_alloc(c, &z, nD)); CHK(dev_alloc(c, &pz, nD));
            CHK(dev_alloc(c, &cz, n)); CHK(dev_alloc(c, &keys, n));
            CHK(dev_alloc(c, &ha, n)); CHK(dev_alloc(c, &hb, n));
            if (c->sel_list_cap < n) {  // (what select_threshold would grow behind the launches)
                c->sel_list_cap = 0;
                CHK(dev_alloc(c, &c->sel_list, n));
                c->sel_list_cap = n;
            }
        }
        return CELLECTOR_OK;
    }

    cellector_status moments(cellector_ctx *c, uint64_t L, const uint8_t *d_mask, const cellector_donor_params *prm)
    {
        if (!L) return CELLECTOR_OK;
        hipLaunchKernelGGL(k_donor_moments, dim3(lane_grid(L * 16, LANE_THREADS, 0x7fffffffu)), dim3(LANE_THREADS), 0, c->stream, L * 16,
                           c->s_alt.get(), c->s_ref.get(), d_mask, prm->err, prm->ambient, mom1.get(), mom2.get());
        HIPCHK(c, hipGetLastError());
        return CELLECTOR_OK;
    }
};

}  // namespace

// cellector_donor_moment_tables: validated arguments; host outputs, any may be null
cellector_status donor_moment_tables_run(cellector_ctx *c, const cellector_donor_params *prm, const uint8_t *mask, double *mom1, double *mom2)
{
    const uint64_t L = c->L;
    LociMask m;
    FitRun f;
    CHK(dev_alloc(c, &m.buf, L));
    CHK(f.alloc(c, L, 0, 0, false));
    invalidate_cell_ll_state(c);
    cellector_status st = m.set(c, mask, L);
    if (st == CELLECTOR_OK) st = f.moments(c, L, m.get(), prm);
    if (st == CELLECTOR_OK && mom1) st = d2h(c, mom1, f.mom1, L * 4 * 16);
    if (st == CELLECTOR_OK && mom2) st = d2h(c, mom2, f.mom2, L * 16 * 16);
    (void)hipStreamSynchronize(c->stream);  // (nothing of the scratch may be in use when it goes)
    return st;
}

// cellector_donor_fit: validated arguments (log_prior never null); the donor call into the run's scratch, then the moment tables and
// the fit pass over the same packed genotypes, anchors, sums and calls; the threshold and the flags on the host over the copied keys
cellector_status donor_fit_run(cellector_ctx *c, const uint8_t *gt, uint32_t D, const cellector_donor_params *prm, const cellector_donor_fit_params *fp,
                               const double *log_prior, const uint8_t *anchor, const uint8_t *mask, double log_singlet, double log_pair,
                               double *fit_e, double *fit_v, double *pair_e, double *pair_v, double *z, double *pair_z, double *call_z,
                               uint8_t *hyp_a, uint8_t *hyp_b, uint8_t *status, uint8_t *unmatched, cellector_donor_fit_summary *out,
                               double *mom1, double *mom2)
{
    LapTimer whole;
    DonorRun r{c, D, (D + 31) / 32, c->nloc, c->L, c->total_loci};
    FitRun f;
    const uint64_t n = r.n, L = r.L, nD = n * D;
    CHK(r.alloc(true, 0));
    CHK(f.alloc(c, L, n, D, true));
    std::vector<uint8_t> h_status(n), h_best(n), h_flag(n, 0);
    std::vector<double> h_cz(n), h_keys;
    h_keys.reserve(n);
    invalidate_cell_ll_state(c);
    cellector_status st = r.cells(gt, prm, log_prior, anchor, mask, log_singlet, log_pair);
    if (st == CELLECTOR_OK) st = f.moments(c, L, r.mask.get(), prm);
    EventMarks<2> ev;
    ev.mark(0, c->stream);
    if (st == CELLECTOR_OK && n) {
        const int dpw = lane_width(D, 2);
        const dim3 grid(lane_walk_grid(n, dpw, c->n_cu)), block(LANE_THREADS);
        lane_dispatch<2, 64>(dpw, [&](auto DP) {
            hipLaunchKernelGGL((k_donor_fit<DP>), grid, block, 0, c->stream, n, D, r.W, c->csr_ptr.get(), c->csr_ent.get(), r.packed.get(),
                               f.mom1.get(), f.mom2.get(), r.mask.get(), r.anchor.get(), r.s.get(), r.p.get(), r.best.get(), r.best_pair.get(),
                               r.status.get(), f.e.get(), f.v.get(), f.pe.get(), f.pv.get(), f.z.get(), f.pz.get(), f.cz.get(), f.ha.get(),
                               f.hb.get());
        });
        if (hipGetLastError() != hipSuccess) st = ctx_fail(c, CELLECTOR_EDEVICE, "donor_fit: launch failed");
    }
    ev.mark(1, c->stream);
    if (st == CELLECTOR_OK && fit_e) st = d2h(c, fit_e, f.e, nD * 8);
    if (st == CELLECTOR_OK && fit_v) st = d2h(c, fit_v, f.v, nD * 8);
    if (st == CELLECTOR_OK && pair_e) st = d2h(c, pair_e, f.pe, nD * 8);
    if (st == CELLECTOR_OK && pair_v) st = d2h(c, pair_v, f.pv, nD * 8);
    if (st == CELLECTOR_OK && z) st = d2h(c, z, f.z, nD * 8);
    if (st == CELLECTOR_OK && pair_z) st = d2h(c, pair_z, f.pz, nD * 8);
    if (st == CELLECTOR_OK) st = d2h(c, h_cz.data(), f.cz, n * 8);
    if (st == CELLECTOR_OK && hyp_a) st = d2h(c, hyp_a, f.ha, n);
    if (st == CELLECTOR_OK && hyp_b) st = d2h(c, hyp_b, f.hb, n);
    if (st == CELLECTOR_OK) st = d2h(c, h_status.data(), r.status, n);
    if (st == CELLECTOR_OK) st = d2h(c, h_best.data(), r.best, n);
    if (st == CELLECTOR_OK && mom1) st = d2h(c, mom1, f.mom1, L * 4 * 16);
    if (st == CELLECTOR_OK && mom2) st = d2h(c, mom2, f.mom2, L * 16 * 16);
    if (st == CELLECTOR_OK && hipStreamSynchronize(c->stream) != hipSuccess) st = ctx_fail(c, CELLECTOR_EDEVICE, "donor_fit: the device failed");
    // the keys: the called z of the status-0 cells in ascending cell order; the library's select gives the three statistics
    cellector_donor_fit_summary sum = {};
    sum.median = sum.iqr = NAN;
    sum.threshold = -INFINITY;
    if (st == CELLECTOR_OK) {
        for (uint64_t i = 0; i < n; i++)
            if (h_status[i] == 0) h_keys.push_back(h_cz[i]);
        sum.n_keys = h_keys.size();
        if (sum.n_keys >= fp->min_cells) {
            double out3[3] = {};
            if (hipMemcpyAsync(f.keys, h_keys.data(), sum.n_keys * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess)
                st = ctx_fail(c, CELLECTOR_EDEVICE, "donor_fit: the upload of the keys failed");
            if (st == CELLECTOR_OK) st = select_threshold(c, f.keys, sum.n_keys, fp->iqr_multiple);
            if (st == CELLECTOR_OK) st = d2h(c, out3, c->sel_out + 8, sizeof out3);
            sum.median = out3[0]; sum.iqr = out3[1]; sum.threshold = out3[2];
        }
    }
    (void)hipStreamSynchronize(c->stream);  // (nothing of the scratch may be in use when it goes)
    float ms = 0.f, ms1 = 0.f, ms2 = 0.f;
    if (st == CELLECTOR_OK && ev.ms(0, 1, &ms) && r.ev.ms(0, 1, &ms1) && r.ev.ms(1, 2, &ms2))
        fprintf(stderr, "[timing]   donor_fit: D %u singlet pass %.3f ms, pair pass %.3f ms, fit pass %.3f ms, whole call %.4f s\n", D, ms1, ms2,
                ms, whole.lap());
    if (st != CELLECTOR_OK) return st;
    for (uint64_t i = 0; i < n; i++) {
        if (h_status[i] == DN_NONE || !(h_cz[i] < sum.threshold)) continue;  // strict, main.rs:331
        h_flag[i] = 1;
        sum.n_unmatched++;
        (h_status[i] == 0 ? sum.n_unmatched_singlet : h_status[i] == 1 ? sum.n_unmatched_doublet : sum.n_unmatched_ambiguous)++;
        sum.donor_unmatched[h_best[i] < 64 ? h_best[i] : 0]++;
    }
    if (call_z && n) memcpy(call_z, h_cz.data(), n * 8);
    if (status && n) memcpy(status, h_status.data(), n);
    if (unmatched && n) memcpy(unmatched, h_flag.data(), n);
    if (out) *out = sum;
    return CELLECTOR_OK;
}
