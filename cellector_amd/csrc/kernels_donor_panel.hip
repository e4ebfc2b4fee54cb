// Donor panels (cellector_donor_panel, cellector_match_donors_panel): the donor calls of kernels_donors.hip for up to 4096 donors.
// include/cellector_ffi.h states the model completely; cellector_amd/donors.py (panel_shortlist, panel_posteriors) is its twin.
//
// k_donor_e gives a donor a lane and stops at 64.  Here a WAVE owns a cell and a lane owns Q = the power of two >= ceil(D / 64)
// donors, lane * Q ... lane * Q + Q - 1: their 2-bit codes are 2 Q adjacent bits of the packed row (one u64 word, two at Q = 64), and
// their Q ordered sums live in registers, indexed statically by full unrolling.  The four terms of an entry, one per genotype value,
// do not depend on the donor: they are formed once per entry from the wave-uniform table row, by the operations of k_donor_e, and a
// donor selects one by its code and adds it.  The entries of a row are fetched a chunk of 64 per wave, one per lane, and handed round
// by shuffles.
//   k_panel_pack         a slab of donors gt [DS][total_loci] u8 -> its words of packed [L][W]
//   k_donor_panel<Q>     per cell: the D singlet sums; u = s + log_prior; the shortlist (the first M donors by (u descending, d
//                        ascending), listed in ascending d) with best and second; the anchor; a second walk of the row with lane =
//                        shortlist slot for the pair sums (anchor, d) through tab2; one softmax over the D singlets in ascending d and
//                        the shortlisted pairs, its sum strictly sequential; the status
//   k_donor_panel_match  k_donor_match over a grid of (class, block of 64 donors)
// All scratch belongs to the call and none of it grows with cells x D unless ll is asked for.  Nothing of the ctx is written.
#include "lane_rows.h"

#include <cmath>
#include <vector>

#define PN_NONE 65535
#define PN_SLAB 256  // donors whose u8 genotypes are on the device at a time
#define PN_LAST 0x7fffffff

// words w_off ... w_off + WS - 1 of packed[l][W] from the slab's gt [DS][TL]: donor 32 w + b of the slab at bits 2 b of word w_off + w
__global__ __launch_bounds__(LANE_THREADS) void k_panel_pack(uint64_t n /*L WS*/, uint32_t DS, uint32_t WS, uint32_t W, uint32_t w_off, uint64_t TL,
                                                             const uint64_t *__restrict__ locus_ids, const uint8_t *__restrict__ gt,
                                                             uint64_t *__restrict__ packed)
{
    const uint64_t i = (uint64_t)blockIdx.x * LANE_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint64_t l = i / WS, t = locus_ids[l];
    const uint32_t w = (uint32_t)(i % WS);
    uint64_t word = 0;
    if (t < TL)
        for (uint32_t b = 0; b < 32 && 32 * w + b < DS; b++) word |= (uint64_t)(gt[(uint64_t)(32 * w + b) * TL + t] & 3u) << (2 * b);
    packed[l * W + w_off + w] = word;
}

struct PanelArgs {
    uint64_t n_rows;
    uint32_t D, W, M;
    double log_singlet, log_pair, threshold;
    uint64_t min_loci;
    const uint64_t *row_ptr, *ent, *packed;
    const double2 *tab1, *tab2;
    const uint8_t *mask;       // or null
    const double *lp;          // [D]
    const uint16_t *anchor_in; // [rows] or null
    double *ll;                // [rows][D] or null
    uint16_t *cand;            // [rows][M]
    double *cand_ll, *cand_pair_ll, *cand_post, *cand_ppost;  // [rows][M]
    double *dp, *best_post;    // [rows]
    uint16_t *best, *second, *best_pair, *anchor;  // [rows]
    uint32_t *cnt;             // [rows]
    uint8_t *status;           // [rows]
};

template <int Q>
__global__ __launch_bounds__(LANE_THREADS) void k_donor_panel(const PanelArgs A)
{
    constexpr int NW = Q > 32 ? Q / 32 : 1;  // packed words a lane reads per entry
    constexpr int QW = Q > 32 ? 32 : Q;      // donors of a lane per word
    const int lane = (int)(threadIdx.x & 63);
    const uint32_t D = A.D, W = A.W, M = A.M;
    const uint32_t d0 = (uint32_t)lane * Q;                    // this lane's first donor
    const uint32_t w0 = d0 >> 5, sh0 = 2u * (d0 & 31u);        // its word and its bit there
    const uint64_t wave0 = (uint64_t)blockIdx.x * LANE_WAVES + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * LANE_WAVES;
    for (uint64_t row = wave0; row < A.n_rows; row += n_waves) {
        const uint64_t beg = A.row_ptr[row], end = A.row_ptr[row + 1];
        // ---- the singlet sums: Q ordered accumulators per lane ----
        double acc[Q];
#pragma unroll
        for (int q = 0; q < Q; q++) acc[q] = 0.0;
        uint32_t cnt = 0;
        for (uint64_t c0 = beg; c0 < end; c0 += 64) {
            const uint64_t mine = c0 + (uint64_t)lane < end ? A.ent[c0 + lane] : 0ull;
            const int nc = end - c0 < 64 ? (int)(end - c0) : 64;
            for (int j = 0; j < nc; j += LANE_AHEAD) {
                uint64_t en[LANE_AHEAD], pw[LANE_AHEAD][NW];
                double2 t[LANE_AHEAD][4];
                bool use[LANE_AHEAD];
#pragma unroll
                for (int k = 0; k < LANE_AHEAD; k++) {
                    en[k] = __shfl(mine, j + k, 64);
                    const uint64_t l = ENT_IDX(en[k]);
                    use[k] = j + k < nc && (!A.mask || A.mask[l] != 0);
#pragma unroll
                    for (int g = 0; g < 4; g++) t[k][g] = use[k] ? A.tab1[l * 4 + g] : make_double2(0.0, 0.0);
#pragma unroll
                    for (int w = 0; w < NW; w++) pw[k][w] = use[k] && w0 + w < W ? A.packed[l * W + w0 + w] : 0ull;
                }
#pragma unroll
                for (int k = 0; k < LANE_AHEAD; k++) {
                    if (!use[k]) continue;
                    const double al = (double)ENT_ALT(en[k]), re = (double)ENT_REF(en[k]);
                    double term[4];
#pragma unroll
                    for (int g = 0; g < 4; g++) {
                        const double pa = al * t[k][g].x, pb = re * t[k][g].y;
                        term[g] = pa + pb;
                    }
#pragma unroll
                    for (int w = 0; w < NW; w++) {
                        const uint64_t bits = pw[k][w] >> (NW > 1 ? 0u : sh0);
#pragma unroll
                        for (int q = 0; q < QW; q++) {
                            const uint32_t code = (uint32_t)(bits >> (2 * q)) & 3u;
                            const double lo = code & 1u ? term[1] : term[0], hi = code & 1u ? term[3] : term[2];
                            acc[w * QW + q] = acc[w * QW + q] + (code & 2u ? hi : lo);
                        }
                    }
                    cnt++;
                }
            }
        }
        // ---- u = s + log_prior; a donor past D is no hypothesis ----
        double u[Q];
#pragma unroll
        for (int q = 0; q < Q; q++) {
            const uint32_t d = d0 + q;
            const bool ok = d < D;
            if (ok && A.ll) A.ll[row * D + d] = acc[q];
            u[q] = ok ? acc[q] + A.lp[d] : -INFINITY;
        }
        // ---- the shortlist: round r takes the first donor behind round r - 1's in (u descending, d ascending); lane r keeps it ----
        const uint32_t two = D < 2u ? D : 2u, rounds = M > two ? M : two;  // (second needs a round of its own at M = 1)
        double prev_u = 0.0, my_u = -INFINITY;
        int prev_d = -1, my_d = PN_LAST;
        uint32_t best = 0, second = PN_NONE;
        for (uint32_t r = 0; r < rounds; r++) {
            double v = -INFINITY;
            int idx = PN_LAST;
#pragma unroll
            for (int q = 0; q < Q; q++) {
                const int d = (int)d0 + q;
                const bool behind = r == 0 || u[q] < prev_u || (u[q] == prev_u && d > prev_d);
                const bool ok = (uint32_t)d < D && behind;
                if (ok && (idx == PN_LAST || u[q] > v)) { v = u[q]; idx = d; }
            }
            lane_argmax<64>(v, idx);
            prev_u = v; prev_d = idx;
            if (r == 0) best = (uint32_t)idx;
            if (r == 1) second = (uint32_t)idx;
            if (r < M && (uint32_t)lane == r) { my_u = v; my_d = idx; }
        }
        const double u_best = __shfl(my_u, 0, 64);  // (lane 0 holds round 0's)
        // in ascending d: slot = the number of shortlisted donors below this one
        int rank = 0;
        for (uint32_t k = 0; k < M; k++) rank += __shfl(my_d, (int)k, 64) < my_d ? 1 : 0;
        int cd = PN_LAST;
        double cu = -INFINITY;
        for (uint32_t k = 0; k < M; k++) {
            const int rk = __shfl(rank, (int)k, 64), dk = __shfl(my_d, (int)k, 64);
            const double uk = __shfl(my_u, (int)k, 64);
            if (rk == lane) { cd = dk; cu = uk; }
        }
        const bool slot = (uint32_t)lane < M && (uint32_t)cd < D;  // (M <= D: every slot is filled; no index leaves the row whatever u holds)
        // ---- the anchor, and the pair walk: lane = shortlist slot ----
        if (best >= D) best = 0;
        const uint32_t a_in = A.anchor_in ? A.anchor_in[row] : best;
        const uint32_t a = a_in < D ? a_in : 0u;  // (never: the host checks a given anchor)
        const uint32_t a_word = a >> 5, a_shift = 2u * (a & 31u);
        const uint32_t c_word = slot ? (uint32_t)cd >> 5 : 0u, c_shift = slot ? 2u * ((uint32_t)cd & 31u) : 0u;
        double sacc = 0.0, pacc = 0.0;
        for (uint64_t c0 = beg; c0 < end; c0 += 64) {
            const uint64_t mine = c0 + (uint64_t)lane < end ? A.ent[c0 + lane] : 0ull;
            const int nc = end - c0 < 64 ? (int)(end - c0) : 64;
            for (int j = 0; j < nc; j += LANE_AHEAD) {
                uint64_t en[LANE_AHEAD];
                double2 ts[LANE_AHEAD], tp[LANE_AHEAD];
                bool use[LANE_AHEAD];
#pragma unroll
                for (int k = 0; k < LANE_AHEAD; k++) {
                    en[k] = __shfl(mine, j + k, 64);
                    const uint64_t l = ENT_IDX(en[k]);
                    use[k] = j + k < nc && (!A.mask || A.mask[l] != 0);
                    ts[k] = tp[k] = make_double2(0.0, 0.0);
                    if (use[k] && slot) {
                        const uint32_t gd = (uint32_t)(A.packed[l * W + c_word] >> c_shift) & 3u;
                        const uint32_t ga = (uint32_t)(A.packed[l * W + a_word] >> a_shift) & 3u;
                        ts[k] = A.tab2[l * 16 + 5 * gd];  // (the diagonal carries tab1's bits)
                        tp[k] = A.tab2[l * 16 + 4 * ga + gd];
                    }
                }
#pragma unroll
                for (int k = 0; k < LANE_AHEAD; k++) {
                    if (!use[k]) continue;
                    const double al = (double)ENT_ALT(en[k]), re = (double)ENT_REF(en[k]);
                    const double sa = al * ts[k].x, sb = re * ts[k].y;
                    const double st = sa + sb;
                    sacc = sacc + st;
                    const double pa = al * tp[k].x, pb = re * tp[k].y;
                    const double pt = pa + pb;
                    pacc = pacc + pt;
                }
            }
        }
        // ---- the chain: the D singlets in ascending d, then the shortlisted pairs in ascending d ----
        const bool pair_ok = slot && (uint32_t)cd != a;
        const double y = pair_ok ? pacc + A.log_pair : -INFINITY;
        const double cx = slot ? cu + A.log_singlet : -INFINITY;
        double m = y;
#pragma unroll
        for (int q = 0; q < Q; q++) {
            u[q] = u[q] + A.log_singlet;  // x_d (-inf past D)
            m = fmax(m, u[q]);
        }
        int dummy = 0;
        lane_argmax<64>(m, dummy);
#pragma unroll
        for (int q = 0; q < Q; q++) u[q] = exp(u[q] - m);  // exp(-inf) = 0, and den + 0 is den
        const double ey = exp(y - m);
        double den = 0.0;
        const int n_lanes = (int)((D + Q - 1) / Q);
        for (int ln = 0; ln < n_lanes; ln++) {
#pragma unroll
            for (int q = 0; q < Q; q++) den = den + __shfl(u[q], ln, 64);
        }
        for (uint32_t k = 0; k < M; k++) den = den + __shfl(ey, (int)k, 64);
        const double w = exp(cx - m) / den, wp = ey / den;
        double dp = 0.0;
        for (uint32_t k = 0; k < M; k++) dp = dp + __shfl(wp, (int)k, 64);
        double vy = y;
        int bp = pair_ok ? cd : PN_LAST;
        lane_argmax<64>(vy, bp);
        const double xb = u_best + A.log_singlet;
        const double wb = exp(xb - m) / den;
        if (slot) {
            const uint64_t at = row * M + lane;
            A.cand[at] = (uint16_t)cd;
            A.cand_ll[at] = sacc;
            A.cand_pair_ll[at] = pacc;
            A.cand_post[at] = w;
            A.cand_ppost[at] = wp;
        }
        if (lane == 0) {
            A.dp[row] = dp;
            A.best_post[row] = wb;
            A.best[row] = (uint16_t)best;
            A.second[row] = D > 1 ? (uint16_t)second : (uint16_t)PN_NONE;
            A.best_pair[row] = bp == PN_LAST ? (uint16_t)PN_NONE : (uint16_t)bp;
            A.anchor[row] = (uint16_t)a;
            A.cnt[row] = cnt;
            A.status[row] = (uint64_t)cnt < A.min_loci ? (uint8_t)255 : dp > 0.5 ? (uint8_t)1 : wb >= A.threshold ? (uint8_t)0 : (uint8_t)2;
        }
    }
}

// ll[k][d] = the ordered sum over ascending unmasked loci of ((a la) + (r lb)): k_donor_match's sum.  Block (k, d / 64), lane d % 64.
__global__ __launch_bounds__(64) void k_donor_panel_match(uint64_t L, uint32_t D, uint32_t W, const unsigned long long *__restrict__ alt /*[K][L]*/,
                                                          const unsigned long long *__restrict__ ref, const uint64_t *__restrict__ packed,
                                                          const double2 *__restrict__ tab1, const uint8_t *__restrict__ mask /*or null*/,
                                                          double *__restrict__ ll /*[K][D]*/)
{
    const uint32_t k = blockIdx.x, d = blockIdx.y * 64 + threadIdx.x;
    if (d >= D) return;
    const uint32_t my_word = d >> 5, my_shift = 2u * (d & 31u);
    const unsigned long long *const ak = alt + (uint64_t)k * L, *const rk = ref + (uint64_t)k * L;
    double acc = 0.0;
    // the entry loop of lane_rows.h over loci, as k_donor_match has it
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

// ---- host side -----------------------------------------------------------------------------------------------------------------
namespace {

// the scratch of one call; alloc() makes all of it before anything is launched
struct PanelRun {
    cellector_ctx *c;
    uint32_t D, W, M;
    uint64_t n, L, TL;
    DevBuf<uint8_t> slab;           // [min(D, PN_SLAB)][TL]
    LociMask mask;                  // [L]
    DevBuf<uint64_t> packed;        // [L][W]
    DevBuf<double2> tab1, tab2;     // [L][4], [L][16]
    DevBuf<double> lp;              // [D]
    DevBuf<double> ll;              // [n][D], only where the caller asks for it; the match: [K][D]
    DevBuf<uint16_t> anchor_in, cand;
    DevBuf<double> cand_ll, cand_pair_ll, cand_post, cand_ppost;  // [n][M]
    DevBuf<double> dp, best_post;   // [n]
    DevBuf<uint16_t> best, second, best_pair, anchor;  // [n]
    DevBuf<uint32_t> cnt;           // [n]
    DevBuf<uint8_t> status;         // [n]
    DevBuf<unsigned long long> alt, ref;  // [K][L] the class tallies (match)
    EventMarks<3> ev;               // before the packing, before the cell pass, behind it

    cellector_status alloc(bool cells, bool want_ll, uint32_t K)
    {
        CHK(dev_alloc(c, &slab, (uint64_t)(D < PN_SLAB ? D : PN_SLAB) * TL));
        CHK(dev_alloc(c, &packed, L * W));
        CHK(dev_alloc(c, &mask.buf, L));
        CHK(dev_alloc(c, &tab1, L * 4));
        CHK(dev_alloc(c, &tab2, L * 16));
        if (cells) {
            const uint64_t nM = n * M;
            CHK(dev_alloc(c, &lp, D));
            if (want_ll) CHK(dev_alloc(c, &ll, n * D));
            CHK(dev_alloc(c, &anchor_in, n));
            CHK(dev_alloc(c, &cand, nM));
            CHK(dev_alloc(c, &cand_ll, nM)); CHK(dev_alloc(c, &cand_pair_ll, nM));
            CHK(dev_alloc(c, &cand_post, nM)); CHK(dev_alloc(c, &cand_ppost, nM));
            CHK(dev_alloc(c, &dp, n)); CHK(dev_alloc(c, &best_post, n));
            CHK(dev_alloc(c, &best, n)); CHK(dev_alloc(c, &second, n)); CHK(dev_alloc(c, &best_pair, n)); CHK(dev_alloc(c, &anchor, n));
            CHK(dev_alloc(c, &cnt, n));
            CHK(dev_alloc(c, &status, n));
        }
        if (K) {
            CHK(dev_alloc(c, &alt, (uint64_t)K * L)); CHK(dev_alloc(c, &ref, (uint64_t)K * L));
            CHK(dev_alloc(c, &ll, (uint64_t)K * D));
        }
        return CELLECTOR_OK;
    }

    // the genotypes slab by slab (upload, pack; the stream orders a slab's packing before the next upload), then the tables
    cellector_status prepare(const uint8_t *gt, const uint8_t *host_mask, const cellector_donor_params *prm)
    {
        CHK(mask.set(c, host_mask, L));
        if (!L) return CELLECTOR_OK;
        for (uint32_t s0 = 0; s0 < D; s0 += PN_SLAB) {
            const uint32_t DS = D - s0 < PN_SLAB ? D - s0 : PN_SLAB, WS = (DS + 31) / 32;
            HIPCHK(c, hipMemcpyAsync(slab, gt + (uint64_t)s0 * TL, (uint64_t)DS * TL, hipMemcpyHostToDevice, c->stream));
            hipLaunchKernelGGL(k_panel_pack, dim3(lane_grid(L * WS, LANE_THREADS, 0x7fffffffu)), dim3(LANE_THREADS), 0, c->stream, L * WS, DS, WS, W,
                               s0 / 32, TL, c->locus_ids.get(), slab.get(), packed.get());
            HIPCHK(c, hipGetLastError());
        }
        return donor_tables_launch(c, mask.get(), prm, tab1.get(), tab2.get());
    }
};

template <int Q>
void panel_launch(const PanelArgs &a, unsigned grid, hipStream_t stream)
{
    hipLaunchKernelGGL((k_donor_panel<Q>), dim3(grid), dim3(LANE_THREADS), 0, stream, a);
}

}  // namespace

// cellector_donor_panel: validated arguments (log_prior never null: the caller's or zeros); host outputs, any may be null
cellector_status donor_panel_run(cellector_ctx *c, const uint8_t *gt, uint32_t D, uint32_t M, const cellector_donor_params *prm,
                                 const double *log_prior, const uint16_t *anchor, const uint8_t *mask, double log_singlet, double log_pair,
                                 uint16_t *cand, double *cand_ll, double *cand_pair_ll, double *cand_posterior, double *cand_pair_posterior,
                                 double *doublet_posterior, double *best_posterior, uint16_t *best, uint16_t *second, uint16_t *best_pair,
                                 uint16_t *anchor_out, uint32_t *n_entries, uint8_t *status, uint64_t *donor_cells,
                                 cellector_donor_panel_summary *out, double *ll, uint64_t *packed, double *tab1, double *tab2)
{
    LapTimer whole;
    PanelRun r{c, D, (D + 31) / 32, M, c->nloc, c->L, c->total_loci};
    const uint64_t n = r.n, L = r.L, nM = n * M;
    CHK(r.alloc(true, ll != nullptr, 0));
    std::vector<uint8_t> h_status(n);
    std::vector<uint16_t> h_best(n);
    std::vector<uint64_t> h_cells(D, 0);
    invalidate_cell_ll_state(c);
    r.ev.mark(0, c->stream);
    cellector_status st = r.prepare(gt, mask, prm);
    if (st == CELLECTOR_OK && hipMemcpyAsync(r.lp, log_prior, (uint64_t)D * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess)
        st = ctx_fail(c, CELLECTOR_EDEVICE, "donor_panel: the upload of the priors failed");
    if (st == CELLECTOR_OK && anchor && n && hipMemcpyAsync(r.anchor_in, anchor, n * 2, hipMemcpyHostToDevice, c->stream) != hipSuccess)
        st = ctx_fail(c, CELLECTOR_EDEVICE, "donor_panel: the upload of the anchors failed");
    r.ev.mark(1, c->stream);
    if (st == CELLECTOR_OK && n) {
        PanelArgs a = {};
        a.n_rows = n; a.D = D; a.W = r.W; a.M = M;
        a.log_singlet = log_singlet; a.log_pair = log_pair; a.threshold = prm->posterior_threshold; a.min_loci = prm->min_loci;
        a.row_ptr = c->csr_ptr.get(); a.ent = c->csr_ent.get(); a.packed = r.packed.get();
        a.tab1 = r.tab1.get(); a.tab2 = r.tab2.get(); a.mask = r.mask.get(); a.lp = r.lp.get();
        a.anchor_in = anchor ? r.anchor_in.get() : nullptr;
        a.ll = ll ? r.ll.get() : nullptr;
        a.cand = r.cand.get(); a.cand_ll = r.cand_ll.get(); a.cand_pair_ll = r.cand_pair_ll.get();
        a.cand_post = r.cand_post.get(); a.cand_ppost = r.cand_ppost.get();
        a.dp = r.dp.get(); a.best_post = r.best_post.get();
        a.best = r.best.get(); a.second = r.second.get(); a.best_pair = r.best_pair.get(); a.anchor = r.anchor.get();
        a.cnt = r.cnt.get(); a.status = r.status.get();
        const unsigned grid = lane_grid(n, LANE_WAVES, (unsigned)c->n_cu * 8);
        const int q = lane_width((D + 63) / 64, 1);
        switch (q) {
        case 1: panel_launch<1>(a, grid, c->stream); break;
        case 2: panel_launch<2>(a, grid, c->stream); break;
        case 4: panel_launch<4>(a, grid, c->stream); break;
        case 8: panel_launch<8>(a, grid, c->stream); break;
        case 16: panel_launch<16>(a, grid, c->stream); break;
        case 32: panel_launch<32>(a, grid, c->stream); break;
        default: panel_launch<64>(a, grid, c->stream); break;
        }
        if (hipGetLastError() != hipSuccess) st = ctx_fail(c, CELLECTOR_EDEVICE, "donor_panel: launch failed");
    }
    r.ev.mark(2, c->stream);
    if (st == CELLECTOR_OK && cand) st = d2h(c, cand, r.cand, nM * 2);
    if (st == CELLECTOR_OK && cand_ll) st = d2h(c, cand_ll, r.cand_ll, nM * 8);
    if (st == CELLECTOR_OK && cand_pair_ll) st = d2h(c, cand_pair_ll, r.cand_pair_ll, nM * 8);
    if (st == CELLECTOR_OK && cand_posterior) st = d2h(c, cand_posterior, r.cand_post, nM * 8);
    if (st == CELLECTOR_OK && cand_pair_posterior) st = d2h(c, cand_pair_posterior, r.cand_ppost, nM * 8);
    if (st == CELLECTOR_OK && doublet_posterior) st = d2h(c, doublet_posterior, r.dp, n * 8);
    if (st == CELLECTOR_OK && best_posterior) st = d2h(c, best_posterior, r.best_post, n * 8);
    if (st == CELLECTOR_OK) st = d2h(c, h_best.data(), r.best, n * 2);
    if (st == CELLECTOR_OK && second) st = d2h(c, second, r.second, n * 2);
    if (st == CELLECTOR_OK && best_pair) st = d2h(c, best_pair, r.best_pair, n * 2);
    if (st == CELLECTOR_OK && anchor_out) st = d2h(c, anchor_out, r.anchor, n * 2);
    if (st == CELLECTOR_OK && n_entries) st = d2h(c, n_entries, r.cnt, n * 4);
    if (st == CELLECTOR_OK) st = d2h(c, h_status.data(), r.status, n);
    if (st == CELLECTOR_OK && ll) st = d2h(c, ll, r.ll, n * D * 8);
    if (st == CELLECTOR_OK && packed) st = d2h(c, packed, r.packed, L * r.W * 8);
    if (st == CELLECTOR_OK && tab1) st = d2h(c, tab1, r.tab1, L * 4 * 16);
    if (st == CELLECTOR_OK && tab2) st = d2h(c, tab2, r.tab2, L * 16 * 16);
    if (st == CELLECTOR_OK && hipStreamSynchronize(c->stream) != hipSuccess) st = ctx_fail(c, CELLECTOR_EDEVICE, "donor_panel: the device failed");
    (void)hipStreamSynchronize(c->stream);  // (nothing of the scratch may be in use when it goes)
    float ms0 = 0.f, ms1 = 0.f;
    if (st == CELLECTOR_OK && r.ev.ms(0, 1, &ms0) && r.ev.ms(1, 2, &ms1))
        fprintf(stderr, "[timing]   donor_panel: D %u M %u packing and tables %.3f ms, cell pass %.3f ms, whole call %.4f s\n", D, M, ms0, ms1,
                whole.lap());
    if (st != CELLECTOR_OK) return st;
    cellector_donor_panel_summary sum = {};
    for (uint64_t i = 0; i < n; i++) {
        switch (h_status[i]) {
        case 0: sum.n_singlet++; h_cells[h_best[i] < D ? h_best[i] : 0]++; break;
        case 1: sum.n_doublet++; break;
        case 2: sum.n_ambiguous++; break;
        default: sum.n_unassigned++; break;
        }
    }
    for (uint32_t d = 0; d < D; d++) sum.n_present += h_cells[d] > 0;
    if (best && n) memcpy(best, h_best.data(), n * 2);
    if (status && n) memcpy(status, h_status.data(), n);
    if (donor_cells) memcpy(donor_cells, h_cells.data(), (uint64_t)D * 8);
    if (out) *out = sum;
    return CELLECTOR_OK;
}

// cellector_match_donors_panel: validated arguments; the tallies are cellector_class_tallies' own; host outputs, any may be null
cellector_status donor_panel_match_run(cellector_ctx *c, const uint8_t *labels, uint32_t K, const uint8_t *gt, uint32_t D,
                                       const cellector_donor_params *prm, const uint8_t *mask, double *ll, uint16_t *best, double *margin,
                                       uint64_t *cells)
{
    PanelRun r{c, D, (D + 31) / 32, 0, c->nloc, c->L, c->total_loci};
    const uint64_t L = r.L;
    CHK(r.alloc(false, false, K));
    std::vector<uint64_t> h_alt((uint64_t)K * L), h_ref((uint64_t)K * L), h_cells(K);
    std::vector<double> h_ll((uint64_t)K * D, 0.0);
    CHK(classes_tallies_run(c, labels, K, nullptr, h_cells.data(), h_alt.data(), h_ref.data(), nullptr, nullptr));
    invalidate_cell_ll_state(c);
    cellector_status st = r.prepare(gt, mask, prm);
    if (st == CELLECTOR_OK && L) {
        if (hipMemcpyAsync(r.alt, h_alt.data(), (uint64_t)K * L * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            hipMemcpyAsync(r.ref, h_ref.data(), (uint64_t)K * L * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess)
            st = ctx_fail(c, CELLECTOR_EDEVICE, "match_donors_panel: the upload of the tallies failed");
    }
    if (st == CELLECTOR_OK) {
        hipLaunchKernelGGL(k_donor_panel_match, dim3(K, (D + 63) / 64), dim3(64), 0, c->stream, L, D, r.W, r.alt.get(), r.ref.get(),
                           r.packed.get(), r.tab1.get(), r.mask.get(), r.ll.get());
        if (hipGetLastError() != hipSuccess) st = ctx_fail(c, CELLECTOR_EDEVICE, "match_donors_panel: launch failed");
    }
    if (st == CELLECTOR_OK) st = d2h(c, h_ll.data(), r.ll, (uint64_t)K * D * 8);
    (void)hipStreamSynchronize(c->stream);
    if (st != CELLECTOR_OK) return st;
    for (uint32_t k = 0; k < K; k++) {
        const double *row = h_ll.data() + (uint64_t)k * D;
        uint32_t b = 0, b2 = PN_NONE;
        for (uint32_t d = 1; d < D; d++)
            if (row[d] > row[b]) b = d;
        for (uint32_t d = 0; d < D; d++)
            if (d != b && (b2 == PN_NONE || row[d] > row[b2])) b2 = d;
        const bool live = h_cells[k] > 0;
        if (best) best[k] = live ? (uint16_t)b : (uint16_t)PN_NONE;
        if (margin) margin[k] = !live ? 0.0 : b2 == PN_NONE ? INFINITY : row[b] - row[b2];
        if (cells) cells[k] = h_cells[k];
    }
    if (ll) memcpy(ll, h_ll.data(), h_ll.size() * 8);
    return CELLECTOR_OK;
}
