// K-genotype class scoring (cellector_class_tallies, _class_alpha_betas, _class_posteriors, cellector_refine_classes): the layer
// between the exact integer recount of a cell set (kernels_state.hip) and the per-cell sum under any alpha/beta (the cell pass).
//
// The model is cellector's own beta-binomial generalised from {minority, majority} to K classes (include/cellector_ffi.h states
// it completely): per class the per-locus allele tallies of its cells, alpha_k = alt_k * scale_k + 1 and beta_k = ref_k * scale_k
// + 1 the way init_alpha_betas forms two (main.rs:598-611), one cell pass per live class (get_cell_log_likelihoods,
// main.rs:541-591), the prior / logsumexp chain of main.rs:264-276 over K terms, and a hard-EM loop that moves every cell to its
// best class until nothing moves.  The doublet classes of the K (K - 1) / 2 unordered pairs are the second half of this file
// (cellector_class_pair_alpha_betas, _class_doublets, cellector_refine_class_doublets); the four calls above form none.
//
// Tallies are sums of integers added with 64-bit atomics: exact and independent of the order the hardware performs them in, so a
// recount, a delta update and numpy give the same integers.  A full recount never walks the class with the most cells: its planes
// are (locus totals - the sum of the others), the subtraction init_alpha_betas itself does.  Between two refine steps only the
// rows of the cells that moved are walked: each is subtracted from its old class and added to its new one (two's-complement
// 64-bit adds).
#include "ctx.h"

#include <cmath>
#include <utility>

#define CL_THREADS 256
#define CL_WAVES (CL_THREADS / 64)
#define CL_MAX 16                // classes
#define CL_NONE 255              // the label of an unlabelled cell
// the counter block of a step (u32): cells moved, then the new size of every class and of the unlabelled cells
// (the doublet refine: the sizes are those of the effective classes, and one more word counts the held cells)
enum { CLC_MOVED = 0, CLC_SIZE = 1, CLC_WORDS = 1 + CL_MAX + 1, CLC_HELD = CLC_WORDS, CLC_WORDS_DBL = CLC_WORDS + 1 };
#define CL_PAIRS (CL_MAX * (CL_MAX - 1) / 2)

struct ClassPriors { double lp[CL_MAX]; };

static inline unsigned cl_grid(uint64_t n, unsigned per_block, unsigned cap)
{
    uint64_t g = (n + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (unsigned)g;
}

// one wave per row of the by-cell CSR, lanes over the row's entries; acc = [K + 1][2][L] u64: alt, ref per class and locus, slot K
// the unlabelled cells and, with held flags, the held ones.  The rows of class `skip` are not walked (k_class_rest forms its planes).
__global__ __launch_bounds__(CL_THREADS) void k_class_tally(uint64_t n_rows, const uint8_t *__restrict__ lab,
                                                            const uint8_t *__restrict__ held /*or null*/, uint32_t K, uint32_t skip,
                                                            const uint64_t *__restrict__ row_ptr, const uint64_t *__restrict__ ent,
                                                            uint64_t L, unsigned long long *__restrict__ acc)
{
    const int lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t)blockIdx.x * CL_WAVES + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * CL_WAVES;
    for (uint64_t row = wave0; row < n_rows; row += nwaves) {
        const uint32_t lb = lab[row];
        const uint32_t k = (lb == CL_NONE || (held && held[row])) ? K : lb;
        if (k == skip) continue;
        unsigned long long *const pa = acc + (uint64_t)k * 2 * L, *const pr = pa + L;
        const uint64_t beg = row_ptr[row], end = row_ptr[row + 1];
        for (uint64_t i = beg + lane; i < end; i += 64) {
            const uint64_t en = ent[i];
            const uint64_t l = ENT_IDX(en);
            const uint32_t a = ENT_ALT(en), r = ENT_REF(en);
            if (a) atomicAdd(&pa[l], (unsigned long long)a);
            if (r) atomicAdd(&pr[l], (unsigned long long)r);
        }
    }
}

// the planes of the class that was not walked: the locus totals (whole numbers in doubles) minus every other slot, as integers
__global__ void k_class_rest(uint64_t L, uint32_t K, uint32_t skip, const double *__restrict__ s_alt, const double *__restrict__ s_ref,
                             unsigned long long *__restrict__ acc)
{
    const uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= L) return;
    unsigned long long a = (unsigned long long)s_alt[l], r = (unsigned long long)s_ref[l];
    for (uint32_t k = 0; k <= K; k++) {
        if (k == skip) continue;
        a -= acc[((uint64_t)k * 2) * L + l];
        r -= acc[((uint64_t)k * 2 + 1) * L + l];
    }
    acc[((uint64_t)skip * 2) * L + l] = a;
    acc[((uint64_t)skip * 2 + 1) * L + l] = r;
}

// the delta between two refine steps: one wave per moved cell, its row leaves the slot it had (was) and joins the one it has now.
// With held flags (the doublet refine) a cell's slot is its effective class: K when it is held, else its label; a cell that stays
// held under another label leaves and joins slot K, which adds up to nothing.
__global__ __launch_bounds__(CL_THREADS) void k_class_delta(uint32_t n_list, const uint32_t *__restrict__ list, const uint8_t *__restrict__ was,
                                                            const uint8_t *__restrict__ now, const uint8_t *__restrict__ held_was /*or null*/,
                                                            const uint8_t *__restrict__ held_now /*or null*/, uint32_t K,
                                                            const uint64_t *__restrict__ row_ptr, const uint64_t *__restrict__ ent, uint64_t L,
                                                            unsigned long long *__restrict__ acc)
{
    const int lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t)blockIdx.x * CL_WAVES + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * CL_WAVES;
    for (uint64_t j = wave0; j < n_list; j += nwaves) {
        const uint32_t row = list[j];
        // (a moved cell is labelled on both sides: an unlabelled cell keeps its label)
        const uint32_t s_was = held_was && held_was[row] ? K : was[row], s_now = held_now && held_now[row] ? K : now[row];
        unsigned long long *const from = acc + (uint64_t)s_was * 2 * L, *const to = acc + (uint64_t)s_now * 2 * L;
        const uint64_t beg = row_ptr[row], end = row_ptr[row + 1];
        for (uint64_t i = beg + lane; i < end; i += 64) {
            const uint64_t en = ent[i];
            const uint64_t l = ENT_IDX(en);
            const unsigned long long a = ENT_ALT(en), r = ENT_REF(en);
            if (a) { atomicAdd(&from[l], 0ull - a); atomicAdd(&to[l], a); }
            if (r) { atomicAdd(&from[L + l], 0ull - r); atomicAdd(&to[L + l], r); }
        }
    }
}

// the K distributions: a rounded product and a rounded sum (the library is built without contraction).  ab = [K][L]; a masked
// locus carries alpha < 0, the cell pass' mark.
struct ClassScales { double s[CL_MAX]; };
__global__ void k_class_ab(uint64_t L, uint32_t K, const unsigned long long *__restrict__ acc, ClassScales sc,
                           const uint8_t *__restrict__ mask /*or null*/, double2 *__restrict__ ab)
{
    const uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= L) return;
    const bool used = !mask || mask[l] != 0;
    for (uint32_t k = 0; k < K; k++) {
        const double a = (double)acc[((uint64_t)k * 2) * L + l] * sc.s[k] + 1.0;
        const double b = (double)acc[((uint64_t)k * 2 + 1) * L + l] * sc.s[k] + 1.0;
        ab[(uint64_t)k * L + l] = used ? make_double2(a, b) : make_double2(-1.0, -1.0);
    }
}

// a pass' result into its column: ll_k = the pass' sums (null: a dead class, -inf), nl = the cells' used-locus counts
__global__ void k_class_column(uint64_t n, const double *__restrict__ ll, const double *__restrict__ nloci, double *__restrict__ col,
                               double *__restrict__ nl /*or null*/)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    col[i] = ll ? ll[i] : -INFINITY;
    if (nl) nl[i] = nloci[i];
}

// One thread per cell: the posterior chain over the live classes in ascending k, then the move rule.
//   x_k = lp_k + ll_k, m = max x_k, best = the smallest k attaining m, den = m + log(sum_k exp(x_k - m)), posterior_k = exp(x_k - den),
//   rest = sum_{k != best} exp(x_k - den), qual = min(-10 log10(rest), 255) as an integer (rest == 0: 255).
// move: a labelled cell with at least min_loci entries at used loci takes the label best; every other cell keeps its own.  The
// moved cells go into a list and the step's counters with one atomic per wave and counter.
__global__ __launch_bounds__(CL_THREADS) void k_class_finalize(uint64_t n, uint32_t K, uint32_t live, ClassPriors pr, const double *__restrict__ ll,
                                                               const double *__restrict__ nl, const uint8_t *__restrict__ lab, uint64_t min_loci,
                                                               int move, double *__restrict__ post, uint8_t *__restrict__ best_out,
                                                               unsigned long long *__restrict__ qual, uint8_t *__restrict__ lab_new,
                                                               uint32_t *__restrict__ list, uint32_t *__restrict__ cnt)
{
    const uint64_t i = (uint64_t)blockIdx.x * CL_THREADS + threadIdx.x;  // (the grid covers n rounded up to whole waves)
    const int lane = threadIdx.x & 63;
    const bool ok = i < n;
    uint32_t newlab = CL_NONE;
    bool moved = false;
    if (ok) {
        double m = -INFINITY;
        uint32_t best = 0;
        bool first = true;
        for (uint32_t k = 0; k < K; k++) {
            if (!((live >> k) & 1u)) continue;
            const double x = pr.lp[k] + ll[(uint64_t)k * n + i];
            if (first || x > m) { m = x; best = k; first = false; }
        }
        double s = 0.0;
        for (uint32_t k = 0; k < K; k++)
            if ((live >> k) & 1u) s += exp((pr.lp[k] + ll[(uint64_t)k * n + i]) - m);
        const double den = m + log(s);
        double rest = 0.0;
        for (uint32_t k = 0; k < K; k++) {
            double p = 0.0;
            if ((live >> k) & 1u) {
                p = exp((pr.lp[k] + ll[(uint64_t)k * n + i]) - den);
                if (k != best) rest += p;
            }
            post[(uint64_t)k * n + i] = p;
        }
        const double q = fmin(-10.0 * log10(rest), 255.0);
        best_out[i] = (uint8_t)best;
        qual[i] = q > 0.0 ? (unsigned long long)q : 0ull;  // (a NaN or a negative value: 0)
        const uint32_t old = lab[i];
        newlab = old;
        if (move && old != CL_NONE && (uint64_t)nl[i] >= min_loci) newlab = best;
        moved = newlab != old;
        lab_new[i] = (uint8_t)newlab;
    }
    const unsigned long long mm = __ballot(moved);
    if (mm) {
        const int leader = __ffsll((long long)mm) - 1;
        uint32_t pos = 0;
        if (lane == leader) pos = atomicAdd(&cnt[CLC_MOVED], (uint32_t)__popcll(mm));
        pos = __shfl(pos, leader, 64);
        if (moved) list[pos + (uint32_t)__popcll(mm & ((1ull << lane) - 1ull))] = (uint32_t)i;
    }
    for (uint32_t k = 0; k <= K; k++) {
        const unsigned long long mk = __ballot(ok && newlab == (k == K ? (uint32_t)CL_NONE : k));
        if (mk && lane == 0) atomicAdd(&cnt[CLC_SIZE + k], (uint32_t)__popcll(mk));
    }
}

// ---- the host side ---------------------------------------------------------------------------------------------------------
namespace {
struct ClassRun {
    cellector_ctx *c;
    uint32_t K;
    uint64_t n, L;
    DevBuf<uint8_t> lab, lab_new, mask;
    DevBuf<unsigned long long> acc, qual;
    DevBuf<double2> ab;
    DevBuf<double> ll, nl, post;
    DevBuf<uint8_t> best;
    DevBuf<uint32_t> list, cnt, masked_cnt;
    uint64_t size[CL_MAX + 1];  // cells per class under the current labels, slot K the unlabelled (and the held) ones
    // the doublet calls: P pairs; held flags beside the labels, one pair's distribution, the pair columns and their outputs
    uint32_t P = 0;
    bool doublets = false;
    DevBuf<uint8_t> held, held_new, best_pair, call;
    DevBuf<double2> pab;
    DevBuf<double> llp, dpost;
    uint64_t n_held = 0;

    cellector_status alloc(bool passes)
    {
        if (doublets) {
            CHK(dev_alloc(c, &held, n));
            CHK(dev_alloc(c, &pab, L));
            if (passes) {
                CHK(dev_alloc(c, &held_new, n));
                CHK(dev_alloc(c, &llp, (uint64_t)P * n));
                CHK(dev_alloc(c, &dpost, n));
                CHK(dev_alloc(c, &best_pair, 2 * n));
                CHK(dev_alloc(c, &call, n));
            }
        }
        CHK(dev_alloc(c, &lab, n));
        CHK(dev_alloc(c, &acc, (uint64_t)(K + 1) * 2 * L));
        CHK(dev_alloc(c, &ab, (uint64_t)K * L));
        if (!passes) return CELLECTOR_OK;
        CHK(dev_alloc(c, &lab_new, n));
        CHK(dev_alloc(c, &mask, L));
        CHK(dev_alloc(c, &ll, (uint64_t)K * n));
        CHK(dev_alloc(c, &nl, n));
        CHK(dev_alloc(c, &post, (uint64_t)K * n));
        CHK(dev_alloc(c, &best, n));
        CHK(dev_alloc(c, &qual, n));
        CHK(dev_alloc(c, &list, n));
        CHK(dev_alloc(c, &cnt, CLC_WORDS_DBL));
        if (c->engine == 2) CHK(dev_alloc(c, &masked_cnt, n));
        return CELLECTOR_OK;
    }

    // the slot a full recount leaves out: the one with the most cells (the lowest on a tie)
    uint32_t largest() const
    {
        uint32_t s = 0;
        for (uint32_t k = 1; k <= K; k++)
            if (size[k] > size[s]) s = k;
        return s;
    }

    cellector_status recount()
    {
        const uint32_t skip = largest();
        HIPCHK(c, hipMemsetAsync(acc, 0, ((uint64_t)(K + 1) * 2 * L + (L ? 0 : 1)) * sizeof(unsigned long long), c->stream));
        if (n && L && size[skip] < n)
            hipLaunchKernelGGL(k_class_tally, dim3(cl_grid(n, CL_WAVES, 8192)), dim3(CL_THREADS), 0, c->stream, n, lab.get(),
                               doublets ? held.get() : (const uint8_t *)nullptr, K, skip, c->csr_ptr.get(), c->csr_ent.get(), L, acc.get());
        if (L)
            hipLaunchKernelGGL(k_class_rest, dim3(cl_grid(L, 256, 0x7fffffffu)), dim3(256), 0, c->stream, L, K, skip, c->s_alt.get(),
                               c->s_ref.get(), acc.get());
        HIPCHK(c, hipGetLastError());
        return CELLECTOR_OK;
    }

    cellector_status delta(uint32_t n_moved)
    {
        if (n_moved && L)  // lab_new (and held_new) still hold the state of the step before (the buffers were swapped)
            hipLaunchKernelGGL(k_class_delta, dim3(cl_grid(n_moved, CL_WAVES, 8192)), dim3(CL_THREADS), 0, c->stream, n_moved, list.get(),
                               lab_new.get(), lab.get(), doublets ? held_new.get() : (const uint8_t *)nullptr,
                               doublets ? held.get() : (const uint8_t *)nullptr, K, c->csr_ptr.get(), c->csr_ent.get(), L, acc.get());
        HIPCHK(c, hipGetLastError());
        return CELLECTOR_OK;
    }

    cellector_status alpha_betas(const double *scale, const uint8_t *d_mask)
    {
        ClassScales sc;
        for (uint32_t k = 0; k < CL_MAX; k++) sc.s[k] = scale && k < K ? scale[k] : 1.0;
        if (L)
            hipLaunchKernelGGL(k_class_ab, dim3(cl_grid(L, 256, 0x7fffffffu)), dim3(256), 0, c->stream, L, K, acc.get(), sc, d_mask, ab.get());
        HIPCHK(c, hipGetLastError());
        return CELLECTOR_OK;
    }
};
}  // namespace

static void class_sizes(const uint8_t *labels, uint64_t n, uint32_t K, uint64_t *size)
{
    for (uint32_t k = 0; k <= K; k++) size[k] = 0;
    for (uint64_t i = 0; i < n; i++) size[labels[i] == CL_NONE ? K : labels[i]]++;
}

// cellector_class_tallies / cellector_class_alpha_betas: validated arguments; any output may be null
cellector_status classes_tallies_run(cellector_ctx *c, const uint8_t *labels, uint32_t K, const double *scale, uint64_t *cells, uint64_t *alt,
                                     uint64_t *ref, double *alpha, double *beta)
{
    ClassRun r{c, K, c->nloc, c->L};
    CHK(r.alloc(false));
    class_sizes(labels, r.n, K, r.size);
    if (r.n) HIPCHK(c, hipMemcpyAsync(r.lab, labels, r.n, hipMemcpyHostToDevice, c->stream));
    CHK(r.recount());
    const uint64_t L = r.L;
    for (uint32_t k = 0; k < K; k++) {
        if (cells) cells[k] = r.size[k];
        if (alt && L) CHK(d2h(c, alt + (uint64_t)k * L, r.acc + ((uint64_t)k * 2) * L, L * 8));
        if (ref && L) CHK(d2h(c, ref + (uint64_t)k * L, r.acc + ((uint64_t)k * 2 + 1) * L, L * 8));
    }
    if ((alpha || beta) && L) {
        CHK(r.alpha_betas(scale, nullptr));
        std::vector<double2> h((uint64_t)K * L);
        CHK(d2h(c, h.data(), r.ab, h.size() * sizeof(double2)));
        for (uint64_t j = 0; j < h.size(); j++) {
            if (alpha) alpha[j] = h[j].x;
            if (beta) beta[j] = h[j].y;
        }
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (the scratch goes back to the cache on return; labels may go)
    return CELLECTOR_OK;
}

// cellector_class_posteriors (max_iter 0, labels_out null) and cellector_refine_classes: validated arguments.  Every device
// buffer is allocated before anything is written; the caller's labels are written once, at the end.
cellector_status classes_run(cellector_ctx *c, const uint8_t *labels, uint32_t K, const double *scale, const double *log_prior,
                             const uint8_t *mask, uint32_t max_iter, uint64_t min_loci, uint8_t *labels_out, cellector_refine_summary *sum,
                             double *ll, double *posterior, uint8_t *best, uint64_t *qual)
{
    ClassRun r{c, K, c->nloc, c->L};
    const uint64_t n = r.n, L = r.L;
    CHK(r.alloc(true));
    class_sizes(labels, n, K, r.size);
    // the engine-2 pass subtracts every cell's entries at the call's masked loci from its used-locus count (scratch: the ctx's own
    // counts belong to the loop's mask and stay)
    if (c->engine == 2) CHK(tiled_call_masked_count(c, mask, r.masked_cnt.get()));
    if (mask && L) HIPCHK(c, hipMemcpyAsync(r.mask, mask, L, hipMemcpyHostToDevice, c->stream));
    if (n) HIPCHK(c, hipMemcpyAsync(r.lab, labels, n, hipMemcpyHostToDevice, c->stream));
    c->tables_prebuilt = false;  // the passes overwrite the tables and their column counters, like cellector_cell_log_likelihoods
    c->work_zeroed = false;
    const bool expected = c->compute_expected;
    cellector_refine_summary s = {};
    uint32_t n_moved = 0;
    cellector_status st = CELLECTOR_OK;
    for (uint32_t step = 0;; step++) {
        // tallies of the current labels: a delta from the step before while fewer cells moved than a recount would walk
        if (step == 0 || !c->class_delta || (uint64_t)n_moved > n - r.size[r.largest()]) {
            if ((st = r.recount()) != CELLECTOR_OK) break;
            s.n_recounts++;
        } else if ((st = r.delta(n_moved)) != CELLECTOR_OK) break;
        if ((st = r.alpha_betas(scale, mask ? r.mask.get() : nullptr)) != CELLECTOR_OK) break;
        // a pass per live class (the expected column is not formed), its sums into the class' column
        ClassPriors pr;
        uint32_t live = 0, k_live = 0;
        uint64_t n_lab = 0;
        for (uint32_t k = 0; k < K; k++) {
            if (r.size[k]) { live |= 1u << k; k_live++; }
            n_lab += r.size[k];
        }
        for (uint32_t k = 0; k < CL_MAX; k++)
            pr.lp[k] = k >= K ? 0.0 : (log_prior ? log_prior[k] : std::log(((double)r.size[k] + 1.0) / ((double)n_lab + (double)k_live)));
        bool have_nl = false;
        c->compute_expected = false;
        for (uint32_t k = 0; k < K && st == CELLECTOR_OK; k++) {
            const bool alive = (live >> k) & 1u;
            if (alive && n) st = c->engine == 2 ? tiled_cell_pass(c, r.ab + (uint64_t)k * L, nullptr, false, r.masked_cnt.get())
                                                : launch_cell_ll(c, r.ab + (uint64_t)k * L, nullptr);
            if (st != CELLECTOR_OK || !n) continue;
            hipLaunchKernelGGL(k_class_column, dim3(cl_grid(n, 256, 0x7fffffffu)), dim3(256), 0, c->stream, n,
                               alive ? c->ll.get() : (const double *)nullptr, c->nloci.get(), r.ll + (uint64_t)k * n,
                               alive && !have_nl ? r.nl.get() : (double *)nullptr);
            have_nl = have_nl || alive;
        }
        c->compute_expected = expected;
        if (st != CELLECTOR_OK) break;
        if (hipMemsetAsync(r.cnt, 0, CLC_WORDS * sizeof(uint32_t), c->stream) != hipSuccess) { st = ctx_fail(c, CELLECTOR_EDEVICE, "hipMemsetAsync failed"); break; }
        if (n)
            hipLaunchKernelGGL(k_class_finalize, dim3(cl_grid(n, CL_THREADS, 0x7fffffffu)), dim3(CL_THREADS), 0, c->stream, n, K, live, pr,
                               r.ll.get(), r.nl.get(), r.lab.get(), min_loci, max_iter ? 1 : 0, r.post.get(), r.best.get(), r.qual.get(),
                               r.lab_new.get(), r.list.get(), r.cnt.get());
        if (hipGetLastError() != hipSuccess) { st = ctx_fail(c, CELLECTOR_EDEVICE, "class finalize launch failed"); break; }
        if (!max_iter) break;
        uint32_t h[CLC_WORDS];  // the step's one read-back: the stop test and the next step's default priors need it
        if ((st = d2h(c, h, r.cnt, sizeof h)) != CELLECTOR_OK) break;
        n_moved = h[CLC_MOVED];
        for (uint32_t k = 0; k <= K; k++) r.size[k] = h[CLC_SIZE + k];
        std::swap(r.lab, r.lab_new);
        s.iterations++;
        s.n_moved_last = n_moved;
        s.n_moved_total += n_moved;
        if (!n_moved) { s.converged = 1; break; }
        if (s.iterations == max_iter) break;
    }
    if (st == CELLECTOR_OK && hipStreamSynchronize(c->stream) != hipSuccess) st = ctx_fail(c, CELLECTOR_EDEVICE, "hipStreamSynchronize failed");
    if (st != CELLECTOR_OK) {
        c->compute_expected = expected;
        (void)hipStreamSynchronize(c->stream);  // (nothing of the scratch may be in use when it goes)
        return st;
    }
    for (uint32_t k = 0; k < K; k++) s.class_cells[k] = r.size[k];
    if (ll) CHK(d2h(c, ll, r.ll, (uint64_t)K * n * 8));
    if (posterior) CHK(d2h(c, posterior, r.post, (uint64_t)K * n * 8));
    if (best) CHK(d2h(c, best, r.best, n));
    if (qual) CHK(d2h(c, qual, r.qual, n * 8));
    if (labels_out) CHK(d2h(c, labels_out, r.lab, n));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (sum) *sum = s;
    return CELLECTOR_OK;
}

// ---- doublet classes: cellector_class_pair_alpha_betas, _class_doublets, cellector_refine_class_doublets ------------------------
// include/cellector_ffi.h states the model.  A pair (a, b), a < b, has the index p = a (2K - a - 1) / 2 + (b - a - 1); its
// distribution is the two classes' tallies brought to the weights ps_a, ps_b and added (main.rs:245-246 for K = 2), its prior the
// droplet doublet rate times the floored fraction of its smaller class (main.rs:259).  One pair's distribution exists at a time:
// k_class_pair_ab, the cell pass, k_class_column into the pair's column, then the next pair.  The finalize sweeps the K + P columns
// three times (max, sum, posteriors), re-reading ll[t][i], coalesced across the wave, and keeps no per-thread array.

// one pair's distribution: two rounded products, a rounded sum, then + 1.0 (no contraction); a masked locus carries alpha < 0
__global__ void k_class_pair_ab(uint64_t L, uint32_t a, uint32_t b, double ps_a, double ps_b, const unsigned long long *__restrict__ acc,
                                const uint8_t *__restrict__ mask /*or null*/, double2 *__restrict__ ab)
{
    const uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= L) return;
    const bool used = !mask || mask[l] != 0;
    const double al = ((double)acc[((uint64_t)a * 2) * L + l] * ps_a + (double)acc[((uint64_t)b * 2) * L + l] * ps_b) + 1.0;
    const double be = ((double)acc[((uint64_t)a * 2 + 1) * L + l] * ps_a + (double)acc[((uint64_t)b * 2 + 1) * L + l] * ps_b) + 1.0;
    ab[l] = used ? make_double2(al, be) : make_double2(-1.0, -1.0);
}

struct PairPriors { double lp[CL_PAIRS]; };

// One thread per cell: the chain over the live singlets in ascending k and then the live pairs in ascending p, the call, and the
// move rule of the held-out refine.
//   x_t = prior + ll, m = max, S = sum exp(x_t - m), den = m + log S, posterior_k = exp(x_k - den), q_p = exp(y_p - den),
//   doublet_posterior = sum_p q_p, best = the smallest k attaining the singlet maximum, best_pair = the smallest p attaining the pair
//   maximum (255, 255 without a live pair), call = doublet_posterior > 0.5, rest = call ? sum_k posterior_k : sum_{k != best}
//   posterior_k + doublet_posterior, qual as k_class_finalize.
// move: a labelled cell with at least min_loci entries at used loci takes label = best and held = doublet_posterior > threshold;
// every other cell keeps both.  The counters are those of the effective classes (a held cell counts in slot K) and the held cells.
__global__ __launch_bounds__(CL_THREADS) void k_class_dbl_finalize(uint64_t n, uint32_t K, uint32_t live, ClassPriors pr, PairPriors pp,
                                                                   const double *__restrict__ ll, const double *__restrict__ llp,
                                                                   const double *__restrict__ nl, const uint8_t *__restrict__ lab,
                                                                   const uint8_t *__restrict__ held, uint64_t min_loci, double threshold,
                                                                   int move, double *__restrict__ post, double *__restrict__ dpost,
                                                                   uint8_t *__restrict__ best_out, uint8_t *__restrict__ pair_out,
                                                                   uint8_t *__restrict__ call_out, unsigned long long *__restrict__ qual,
                                                                   uint8_t *__restrict__ lab_new, uint8_t *__restrict__ held_new,
                                                                   uint32_t *__restrict__ list, uint32_t *__restrict__ cnt)
{
    const uint64_t i = (uint64_t)blockIdx.x * CL_THREADS + threadIdx.x;  // (the grid covers n rounded up to whole waves)
    const int lane = threadIdx.x & 63;
    const bool ok = i < n;
    uint32_t newlab = CL_NONE, newheld = 0;
    bool moved = false;
    if (ok) {
        double m = -INFINITY, mp = -INFINITY;
        uint32_t best = 0, pa = CL_NONE, pb = CL_NONE;
        bool first = true;
        for (uint32_t k = 0; k < K; k++) {
            if (!((live >> k) & 1u)) continue;
            const double x = pr.lp[k] + ll[(uint64_t)k * n + i];
            if (first || x > m) { m = x; best = k; first = false; }
        }
        first = true;
        for (uint32_t a = 0, p = 0; a < K; a++)
            for (uint32_t b = a + 1; b < K; b++, p++) {
                if (!((live >> a) & (live >> b) & 1u)) continue;
                const double y = pp.lp[p] + llp[(uint64_t)p * n + i];
                if (first || y > mp) { mp = y; pa = a; pb = b; first = false; }
            }
        if (!first && mp > m) m = mp;
        double s = 0.0;
        for (uint32_t k = 0; k < K; k++)
            if ((live >> k) & 1u) s += exp((pr.lp[k] + ll[(uint64_t)k * n + i]) - m);
        for (uint32_t a = 0, p = 0; a < K; a++)
            for (uint32_t b = a + 1; b < K; b++, p++)
                if ((live >> a) & (live >> b) & 1u) s += exp((pp.lp[p] + llp[(uint64_t)p * n + i]) - m);
        const double den = m + log(s);
        double others = 0.0, all = 0.0;
        for (uint32_t k = 0; k < K; k++) {
            double p = 0.0;
            if ((live >> k) & 1u) {
                p = exp((pr.lp[k] + ll[(uint64_t)k * n + i]) - den);
                all += p;
                if (k != best) others += p;
            }
            post[(uint64_t)k * n + i] = p;
        }
        double dp = 0.0;
        for (uint32_t a = 0, p = 0; a < K; a++)
            for (uint32_t b = a + 1; b < K; b++, p++)
                if ((live >> a) & (live >> b) & 1u) dp += exp((pp.lp[p] + llp[(uint64_t)p * n + i]) - den);
        const bool dbl = dp > 0.5;  // (strict, main.rs:150)
        const double rest = dbl ? all : others + dp;
        const double q = fmin(-10.0 * log10(rest), 255.0);
        dpost[i] = dp;
        best_out[i] = (uint8_t)best;
        pair_out[2 * i] = (uint8_t)pa;
        pair_out[2 * i + 1] = (uint8_t)pb;
        call_out[i] = dbl ? 1 : 0;
        qual[i] = q > 0.0 ? (unsigned long long)q : 0ull;  // (a NaN or a negative value: 0)
        const uint32_t old = lab[i], oldheld = held[i];
        newlab = old;
        newheld = oldheld;
        if (move && old != CL_NONE && (uint64_t)nl[i] >= min_loci) { newlab = best; newheld = dp > threshold ? 1u : 0u; }
        moved = newlab != old || newheld != oldheld;
        lab_new[i] = (uint8_t)newlab;
        held_new[i] = (uint8_t)newheld;
    }
    const unsigned long long mm = __ballot(moved);
    if (mm) {
        const int leader = __ffsll((long long)mm) - 1;
        uint32_t pos = 0;
        if (lane == leader) pos = atomicAdd(&cnt[CLC_MOVED], (uint32_t)__popcll(mm));
        pos = __shfl(pos, leader, 64);
        if (moved) list[pos + (uint32_t)__popcll(mm & ((1ull << lane) - 1ull))] = (uint32_t)i;
    }
    const uint32_t slot = (newlab == CL_NONE || newheld) ? K : newlab;
    for (uint32_t k = 0; k <= K; k++) {
        const unsigned long long mk = __ballot(ok && slot == k);
        if (mk && lane == 0) atomicAdd(&cnt[CLC_SIZE + k], (uint32_t)__popcll(mk));
    }
    const unsigned long long mh = __ballot(ok && newheld && newlab != CL_NONE);
    if (mh && lane == 0) atomicAdd(&cnt[CLC_HELD], (uint32_t)__popcll(mh));
}

// the sizes of the effective classes (slot K: unlabelled or held) and the held labelled cells; hn = the flags as 0 / 1
static uint64_t doublet_sizes(const uint8_t *labels, const uint8_t *held, uint64_t n, uint32_t K, uint64_t *size, std::vector<uint8_t> &hn)
{
    uint64_t n_held = 0;
    hn.assign(n ? n : 1, 0);
    for (uint32_t k = 0; k <= K; k++) size[k] = 0;
    for (uint64_t i = 0; i < n; i++) {
        const bool h = held && held[i] != 0;
        hn[i] = h ? 1 : 0;
        if (h && labels[i] != CL_NONE) n_held++;
        size[(labels[i] == CL_NONE || h) ? K : labels[i]]++;
    }
    return n_held;
}

static inline uint32_t pair_index(uint32_t K, uint32_t a, uint32_t b) { return a * (2 * K - a - 1) / 2 + (b - a - 1); }

// ps_k: the caller's, else n_min / n_k over the live classes (a dead class: 0; its tallies are zero)
static void pair_scales(const double *pair_scale, const uint64_t *size, uint32_t K, double *ps)
{
    uint64_t n_min = 0;
    for (uint32_t k = 0; k < K; k++)
        if (size[k] && (!n_min || size[k] < n_min)) n_min = size[k];
    for (uint32_t k = 0; k < K; k++) ps[k] = pair_scale ? pair_scale[k] : (size[k] ? (double)n_min / (double)size[k] : 0.0);
}

// cellector_class_pair_alpha_betas: validated arguments; all P rows by the one formula, dead pairs included
cellector_status class_pairs_run(cellector_ctx *c, const uint8_t *labels, const uint8_t *held, uint32_t K, const double *pair_scale,
                                 double *alpha, double *beta)
{
    ClassRun r{c, K, c->nloc, c->L};
    r.P = K * (K - 1) / 2;
    r.doublets = true;
    const uint64_t L = r.L;
    CHK(r.alloc(false));
    std::vector<uint8_t> hn;
    r.n_held = doublet_sizes(labels, held, r.n, K, r.size, hn);
    if (r.n) {
        HIPCHK(c, hipMemcpyAsync(r.lab, labels, r.n, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(r.held, hn.data(), r.n, hipMemcpyHostToDevice, c->stream));
    }
    CHK(r.recount());
    double ps[CL_MAX];
    pair_scales(pair_scale, r.size, K, ps);
    std::vector<double2> h(L);
    for (uint32_t a = 0; a < K && L && (alpha || beta); a++)
        for (uint32_t b = a + 1; b < K; b++) {
            hipLaunchKernelGGL(k_class_pair_ab, dim3(cl_grid(L, 256, 0x7fffffffu)), dim3(256), 0, c->stream, L, a, b, ps[a], ps[b], r.acc.get(),
                               (const uint8_t *)nullptr, r.pab.get());
            HIPCHK(c, hipGetLastError());
            CHK(d2h(c, h.data(), r.pab, L * sizeof(double2)));
            const uint64_t o = (uint64_t)pair_index(K, a, b) * L;
            for (uint64_t l = 0; l < L; l++) {
                if (alpha) alpha[o + l] = h[l].x;
                if (beta) beta[o + l] = h[l].y;
            }
        }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CELLECTOR_OK;
}

// cellector_class_doublets (max_iter 0, labels_out / held_out null) and cellector_refine_class_doublets: validated arguments.  Every
// device buffer is allocated before anything is written; the caller's labels and held flags are written once, at the end.
cellector_status class_doublets_run(cellector_ctx *c, const uint8_t *labels, const uint8_t *held, uint32_t K, const double *scale,
                                    const double *pair_scale, const double *log_prior, const double *log_pair_prior, const uint8_t *mask,
                                    double threshold, uint32_t max_iter, uint64_t min_loci, uint8_t *labels_out, uint8_t *held_out,
                                    cellector_refine_doublets_summary *sum, double *ll, double *ll_pair, double *posterior,
                                    double *doublet_posterior, uint8_t *best, uint8_t *best_pair, uint8_t *call, uint64_t *qual)
{
    ClassRun r{c, K, c->nloc, c->L};
    r.P = K * (K - 1) / 2;
    r.doublets = true;
    const uint64_t n = r.n, L = r.L;
    const uint32_t P = r.P;
    CHK(r.alloc(true));
    std::vector<uint8_t> hn;
    r.n_held = doublet_sizes(labels, held, n, K, r.size, hn);
    if (c->engine == 2) CHK(tiled_call_masked_count(c, mask, r.masked_cnt.get()));
    if (mask && L) HIPCHK(c, hipMemcpyAsync(r.mask, mask, L, hipMemcpyHostToDevice, c->stream));
    if (n) {
        HIPCHK(c, hipMemcpyAsync(r.lab, labels, n, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(r.held, hn.data(), n, hipMemcpyHostToDevice, c->stream));
    }
    c->tables_prebuilt = false;  // as classes_run: the passes overwrite the tables and their column counters
    c->work_zeroed = false;
    const bool expected = c->compute_expected;
    const uint8_t *const d_mask = mask ? r.mask.get() : nullptr;
    cellector_refine_doublets_summary s = {};
    uint32_t n_moved = 0;
    cellector_status st = CELLECTOR_OK;
    const auto pass = [&](const double2 *ab) {
        return c->engine == 2 ? tiled_cell_pass(c, ab, nullptr, false, r.masked_cnt.get()) : launch_cell_ll(c, ab, nullptr);
    };
    for (uint32_t step = 0;; step++) {
        if (step == 0 || !c->class_delta || (uint64_t)n_moved > n - r.size[r.largest()]) {
            if ((st = r.recount()) != CELLECTOR_OK) break;
            s.n_recounts++;
        } else if ((st = r.delta(n_moved)) != CELLECTOR_OK) break;
        if ((st = r.alpha_betas(scale, d_mask)) != CELLECTOR_OK) break;
        ClassPriors pr;
        PairPriors pp;
        double f[CL_MAX], ps[CL_MAX];
        uint32_t live = 0, k_live = 0;
        uint64_t n_lab = 0;
        for (uint32_t k = 0; k < K; k++) {
            if (r.size[k]) { live |= 1u << k; k_live++; }
            n_lab += r.size[k];
        }
        if (!k_live) { st = ctx_fail(c, CELLECTOR_EINVAL, "class doublets: every labelled cell is held: all %u classes are dead", K); break; }
        for (uint32_t k = 0; k < CL_MAX; k++) {
            f[k] = k >= K ? 0.0 : ((double)r.size[k] + 1.0) / ((double)n_lab + (double)k_live);
            pr.lp[k] = k >= K ? 0.0 : (log_prior ? log_prior[k] : std::log(f[k]));
        }
        for (uint32_t p = 0; p < CL_PAIRS; p++) pp.lp[p] = 0.0;
        for (uint32_t a = 0; a < K; a++)
            for (uint32_t b = a + 1; b < K; b++) {
                const uint32_t p = pair_index(K, a, b);
                pp.lp[p] = log_pair_prior ? log_pair_prior[p] : std::log(((double)n / 1000.0 / 100.0) * std::fmax(std::fmin(f[a], f[b]), 0.1));
            }
        pair_scales(pair_scale, r.size, K, ps);
        bool have_nl = false;
        c->compute_expected = false;
        for (uint32_t k = 0; k < K && st == CELLECTOR_OK; k++) {
            const bool alive = (live >> k) & 1u;
            if (alive && n) st = pass(r.ab + (uint64_t)k * L);
            if (st != CELLECTOR_OK || !n) continue;
            hipLaunchKernelGGL(k_class_column, dim3(cl_grid(n, 256, 0x7fffffffu)), dim3(256), 0, c->stream, n,
                               alive ? c->ll.get() : (const double *)nullptr, c->nloci.get(), r.ll + (uint64_t)k * n,
                               alive && !have_nl ? r.nl.get() : (double *)nullptr);
            have_nl = have_nl || alive;
        }
        // a pass per live pair under its own distribution, formed just before it
        for (uint32_t a = 0; a < K && st == CELLECTOR_OK; a++)
            for (uint32_t b = a + 1; b < K && st == CELLECTOR_OK; b++) {
                const bool alive = (live >> a) & (live >> b) & 1u;
                if (!n) continue;
                if (alive) {
                    if (L)
                        hipLaunchKernelGGL(k_class_pair_ab, dim3(cl_grid(L, 256, 0x7fffffffu)), dim3(256), 0, c->stream, L, a, b, ps[a], ps[b],
                                           r.acc.get(), d_mask, r.pab.get());
                    if ((st = pass(r.pab.get())) != CELLECTOR_OK) break;
                }
                hipLaunchKernelGGL(k_class_column, dim3(cl_grid(n, 256, 0x7fffffffu)), dim3(256), 0, c->stream, n,
                                   alive ? c->ll.get() : (const double *)nullptr, c->nloci.get(), r.llp + (uint64_t)pair_index(K, a, b) * n,
                                   (double *)nullptr);
            }
        c->compute_expected = expected;
        if (st != CELLECTOR_OK) break;
        if (hipMemsetAsync(r.cnt, 0, CLC_WORDS_DBL * sizeof(uint32_t), c->stream) != hipSuccess) { st = ctx_fail(c, CELLECTOR_EDEVICE, "hipMemsetAsync failed"); break; }
        if (n)
            hipLaunchKernelGGL(k_class_dbl_finalize, dim3(cl_grid(n, CL_THREADS, 0x7fffffffu)), dim3(CL_THREADS), 0, c->stream, n, K, live, pr, pp,
                               r.ll.get(), r.llp.get(), r.nl.get(), r.lab.get(), r.held.get(), min_loci, threshold, max_iter ? 1 : 0,
                               r.post.get(), r.dpost.get(), r.best.get(), r.best_pair.get(), r.call.get(), r.qual.get(), r.lab_new.get(),
                               r.held_new.get(), r.list.get(), r.cnt.get());
        if (hipGetLastError() != hipSuccess) { st = ctx_fail(c, CELLECTOR_EDEVICE, "class doublet finalize launch failed"); break; }
        if (!max_iter) break;
        uint32_t h[CLC_WORDS_DBL];  // the step's one read-back
        if ((st = d2h(c, h, r.cnt, sizeof h)) != CELLECTOR_OK) break;
        n_moved = h[CLC_MOVED];
        for (uint32_t k = 0; k <= K; k++) r.size[k] = h[CLC_SIZE + k];
        r.n_held = h[CLC_HELD];
        std::swap(r.lab, r.lab_new);
        std::swap(r.held, r.held_new);
        s.iterations++;
        s.n_moved_last = n_moved;
        s.n_moved_total += n_moved;
        if (!n_moved) { s.converged = 1; break; }
        if (s.iterations == max_iter) break;
    }
    if (st == CELLECTOR_OK && hipStreamSynchronize(c->stream) != hipSuccess) st = ctx_fail(c, CELLECTOR_EDEVICE, "hipStreamSynchronize failed");
    if (st != CELLECTOR_OK) {
        c->compute_expected = expected;
        (void)hipStreamSynchronize(c->stream);  // (nothing of the scratch may be in use when it goes)
        return st;
    }
    for (uint32_t k = 0; k < K; k++) s.class_cells[k] = r.size[k];
    s.n_held = r.n_held;
    if (ll) CHK(d2h(c, ll, r.ll, (uint64_t)K * n * 8));
    if (ll_pair) CHK(d2h(c, ll_pair, r.llp, (uint64_t)P * n * 8));
    if (posterior) CHK(d2h(c, posterior, r.post, (uint64_t)K * n * 8));
    if (doublet_posterior) CHK(d2h(c, doublet_posterior, r.dpost, n * 8));
    if (best) CHK(d2h(c, best, r.best, n));
    if (best_pair) CHK(d2h(c, best_pair, r.best_pair, 2 * n));
    if (call) CHK(d2h(c, call, r.call, n));
    if (qual) CHK(d2h(c, qual, r.qual, n * 8));
    if (labels_out) CHK(d2h(c, labels_out, r.lab, n));
    if (held_out) CHK(d2h(c, held_out, r.held, n));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (sum) *sum = s;
    return CELLECTOR_OK;
}
