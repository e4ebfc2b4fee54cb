// cellector_donor_genotypes: the donors' genotypes from the reads of the cells called for them.  include/cellector_ffi.h states the
// model completely; cellector_amd/donor_genotypes.py is its twin.
//   k_dg_tallies    one pass over the staged COO: acc [D + 1][2][total_loci] u64, per slot the alt plane, then the ref plane (the
//                   layout of kernels_genotypes.hip); slot D collects the cells assigned 255
//   k_dg_tables     a thread per locus: the totals over the D + 1 slots, soup, theta_g and (log theta_g, log(1 - theta_g)), g < 3
//   k_dg_posterior  a thread per (donor, locus): the floored prior, q, gt_out and kind
// All scratch belongs to the call.  Nothing of the ctx is written: the EM state, its tables and its outputs stay.
#include "ctx.h"

#include <cmath>

#define DG_THREADS 256
#define DG_BATCH 4                                            // entries a thread has in flight
#define DG_ROUNDS 4                                           // batches per thread
#define DG_BLOCK_ENTRIES (DG_THREADS * DG_BATCH * DG_ROUNDS)  // 4096 entries per block
#define DG_PAIRS 4096                                         // (alt, ref) counter pairs of the LDS window: 32 KiB

// A counter pair is one u64 word, alt in the low u32 and ref in the high u32, so an entry is ONE LDS add.  A half receives at most
// one count of at most 65535 from each of the block's entries: DG_BLOCK_ENTRIES x 65535 = 268431360 < 2^32, so the low half never
// carries into the high one and the high one never wraps.  (The bound holds up to 65536 entries per block.)
static_assert((uint64_t)DG_BLOCK_ENTRIES * 65535ull < (1ull << 32), "a u32 LDS counter must not wrap");

// A block takes the contiguous run [blockIdx.x E, +E) of entries, E = DG_BLOCK_ENTRIES.  Its window is the WL loci from the locus of
// its first entry on, bin[slot][w] (slot-major: the flush walks consecutive loci of one slot, consecutive u64 of one plane; WL is odd,
// so the slots of one locus fall on different banks).  An entry inside the window is an LDS add; any other entry goes straight to
// the planes with global atomics.  Integer adds: exact in any order.  The call needs a READY ctx, and the build behind every way of
// staging (ingest_build sorts by locus whatever order cellector_ingest_coo was given; synth, parse, combine, join and restage end
// locus-major) leaves the staged COO locus-major: a block's loci ascend from its first entry's, and the direct path is taken exactly
// where a block's run spans more than WL loci (runs of sparse loci: more than 2047 at D = 1, more than 63 at D = 64).  The window test
// is one unsigned compare of l - base against WL; a locus below base, which a locus-major COO never has, would wrap to a large value
// and take the direct path too, so the sums do not depend on that order for their correctness, only for their speed.  A locus may
// straddle blocks, hence the flush adds too.  An entry with alt = ref = 0 adds nothing.
__global__ __launch_bounds__(DG_THREADS) void k_dg_tallies(uint64_t n, uint64_t total_loci, uint64_t n_cells, uint32_t D, uint32_t WL,
                                                           const uint32_t *__restrict__ locus, const uint32_t *__restrict__ cell,
                                                           const uint16_t *__restrict__ alt, const uint16_t *__restrict__ ref,
                                                           const uint8_t *__restrict__ assign, unsigned long long *__restrict__ acc)
{
    __shared__ unsigned long long bin[DG_PAIRS];
    const uint32_t S = D + 1, used = S * WL;  // (the host keeps S WL <= DG_PAIRS)
    const uint64_t beg = (uint64_t)blockIdx.x * DG_BLOCK_ENTRIES;
    const uint64_t end = beg + DG_BLOCK_ENTRIES < n ? beg + DG_BLOCK_ENTRIES : n;
    for (uint32_t i = threadIdx.x; i < used; i += DG_THREADS) bin[i] = 0ull;
    const uint64_t base = beg < n ? locus[beg] : 0;
    __syncthreads();
    for (uint64_t i0 = beg + threadIdx.x; i0 < end; i0 += DG_THREADS * DG_BATCH) {
        uint32_t l[DG_BATCH], c[DG_BATCH];
        uint64_t packed[DG_BATCH];
#pragma unroll
        for (int u = 0; u < DG_BATCH; u++) {
            const uint64_t i = i0 + (uint64_t)u * DG_THREADS;
            const bool ok = i < end;
            l[u] = ok ? locus[i] : 0u;
            c[u] = ok ? cell[i] : 0u;
            packed[u] = ok ? (uint64_t)alt[i] | (uint64_t)ref[i] << 32 : 0ull;
        }
#pragma unroll
        for (int u = 0; u < DG_BATCH; u++) {
            // (the staged COO holds no entry outside the matrix; nothing is written outside bin or acc in any case)
            if (packed[u] == 0ull || l[u] >= total_loci || c[u] >= n_cells) continue;
            const uint32_t a = assign[c[u]];
            const uint32_t slot = a < D ? a : D;
            const uint64_t w = (uint64_t)l[u] - base;  // (wraps to a large value below the window)
            if (w < WL) {
                atomicAdd(&bin[slot * WL + (uint32_t)w], (unsigned long long)packed[u]);
            } else {
                unsigned long long *const pa = acc + (uint64_t)slot * 2 * total_loci + l[u];
                const unsigned long long av = packed[u] & 0xffffffffull, rv = packed[u] >> 32;
                if (av) atomicAdd(pa, av);
                if (rv) atomicAdd(pa + total_loci, rv);
            }
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < used; i += DG_THREADS) {
        const unsigned long long v = bin[i];
        if (v == 0ull) continue;
        const uint32_t slot = i / WL, w = i % WL;
        // (a counter is non-zero only where an entry with base + w = its locus < total_loci has been added)
        unsigned long long *const pa = acc + (uint64_t)slot * 2 * total_loci + (base + w);
        const unsigned long long av = v & 0xffffffffull, rv = v >> 32;
        if (av) atomicAdd(pa, av);
        if (rv) atomicAdd(pa + total_loci, rv);
    }
}

// tab [total_loci][3][2] = (la_g, lb_g): steps 2 and 3 of the donor model from the totals over all D + 1 slots, in k_donor_tables'
// operations (its theta for the singlet rows is 0.5 (t + t) = t), so a used locus carries the bits of tab1[l][g]
__global__ __launch_bounds__(DG_THREADS) void k_dg_tables(uint64_t total_loci, uint32_t D, const unsigned long long *__restrict__ acc,
                                                          double err, double ambient, double *__restrict__ tab)
{
    const uint64_t t = (uint64_t)blockIdx.x * DG_THREADS + threadIdx.x;
    if (t >= total_loci) return;
    uint64_t Ai = 0, Ri = 0;
    for (uint32_t s = 0; s <= D; s++) {
        Ai += acc[(uint64_t)s * 2 * total_loci + t];
        Ri += acc[((uint64_t)s * 2 + 1) * total_loci + t];
    }
    const double A = (double)Ai;
    const double num = A + 1.0, tot = (double)(Ai + Ri), den = tot + 2.0;
    const double soup = num / den;
    const double keep = 1.0 - ambient, amb = ambient * soup;
    const double e2 = 1.0 - err;
#pragma unroll
    for (uint32_t g = 0; g < 3; g++) {
        const double e = g == 0 ? err : g == 1 ? 0.5 : e2;
        const double p = keep * e;
        const double th = p + amb;
        const double rest = 1.0 - th;
        tab[(t * 3 + g) * 2] = log(th);
        tab[(t * 3 + g) * 2 + 1] = log(rest);
    }
}

// thread (d, t), t the fast index.  The host has validated every row of the prior; a row it should have refused is counted in bad
// and held as a no-call.
__global__ __launch_bounds__(DG_THREADS) void k_dg_posterior(uint64_t n /*D total_loci*/, uint64_t total_loci,
                                                             const unsigned long long *__restrict__ acc, const double *__restrict__ tab,
                                                             const float *__restrict__ prior /*or null*/, double gt_threshold,
                                                             double prior_floor, double *__restrict__ q /*or null*/,
                                                             uint8_t *__restrict__ gt_out, uint8_t *__restrict__ kind,
                                                             uint32_t *__restrict__ bad)
{
    const uint64_t i = (uint64_t)blockIdx.x * DG_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint64_t d = i / total_loci, t = i % total_loci;
    const uint64_t a = acc[d * 2 * total_loci + t], r = acc[(d * 2 + 1) * total_loci + t];
    const double third = 1.0 / 3.0;
    double w[3] = {third, third, third};
    uint32_t prior_call = 3;
    if (prior) {
        const float f0 = prior[i * 3], f1 = prior[i * 3 + 1], f2 = prior[i * 3 + 2];
        const bool none = f0 != f0 && f1 != f1 && f2 != f2;
        const bool fine = f0 >= 0.f && f1 >= 0.f && f2 >= 0.f && f0 < INFINITY && f1 < INFINITY && f2 < INFINITY && (f0 > 0.f || f1 > 0.f || f2 > 0.f);
        if (fine) {
            const double x0 = (double)f0, x1 = (double)f1, x2 = (double)f2;
            const double s01 = x0 + x1;
            const double sum = s01 + x2;
            w[0] = x0 / sum; w[1] = x1 / sum; w[2] = x2 / sum;
            prior_call = w[1] > w[0] ? (w[2] > w[1] ? 2u : 1u) : (w[2] > w[0] ? 2u : 0u);
        } else if (!none) {
            atomicAdd(bad, 1u);
        }
    }
    const double keep = 1.0 - prior_floor, share = prior_floor / 3.0;
    const double ad = (double)a, rd = (double)r;
    double x[3];
    bool in[3];
    double m = -INFINITY;
#pragma unroll
    for (int g = 0; g < 3; g++) {
        const double la = tab[(t * 3 + g) * 2], lb = tab[(t * 3 + g) * 2 + 1];
        const double pa = ad * la, pr = rd * lb;
        const double lam = pa + pr;
        const double kw = keep * w[g];
        const double v = kw + share;
        in[g] = v != 0.0;
        x[g] = in[g] ? lam + log(v) : -INFINITY;
        if (in[g] && x[g] > m) m = x[g];
    }
    double e[3], den = 0.0;
#pragma unroll
    for (int g = 0; g < 3; g++) {
        e[g] = in[g] ? exp(x[g] - m) : 0.0;
        if (in[g]) den = den + e[g];
    }
    double qg[3];
#pragma unroll
    for (int g = 0; g < 3; g++) qg[g] = in[g] ? e[g] / den : 0.0;
    const uint32_t call = qg[1] > qg[0] ? (qg[2] > qg[1] ? 2u : 1u) : (qg[2] > qg[0] ? 2u : 0u);
    const uint32_t out = qg[call] > gt_threshold ? call : 3u;
    const uint32_t k = a + r == 0 ? 0u : out == 3u ? 4u : prior_call == 3u ? 2u : out == prior_call ? 1u : 3u;
    if (q) { q[i * 3] = qg[0]; q[i * 3 + 1] = qg[1]; q[i * 3 + 2] = qg[2]; }
    gt_out[i] = (uint8_t)out;
    kind[i] = (uint8_t)k;
}

// the odd window that fits the LDS: at most DG_PAIRS / (D + 1) loci
static uint32_t dg_window_loci(uint32_t D)
{
    const uint32_t wl = DG_PAIRS / (D + 1);
    return wl % 2 ? wl : wl - 1;  // (D <= 64: wl >= 63)
}

cellector_status launch_donor_genotype_tallies(cellector_ctx *c, const uint8_t *d_assign, uint32_t D, uint64_t *d_acc)
{
    const uint64_t n = c->coo.n;
    const uint64_t grid = (n + DG_BLOCK_ENTRIES - 1) / DG_BLOCK_ENTRIES;
    if (grid > 0x7fffffffull)
        return ctx_fail(c, CELLECTOR_EINVAL, "donor_genotypes: %llu staged entries, one launch covers below 2^43", (unsigned long long)n);
    HIPCHK(c, hipMemsetAsync(d_acc, 0, (uint64_t)(D + 1) * 2 * c->total_loci * 8, c->stream));
    if (n) {
        hipLaunchKernelGGL(k_dg_tallies, dim3((unsigned)grid), dim3(DG_THREADS), 0, c->stream, n, c->total_loci, c->nloc, D,
                           dg_window_loci(D), c->coo.locus.get(), c->coo.cell.get(), c->coo.alt.get(), c->coo.ref.get(), d_assign,
                           (unsigned long long *)d_acc);
    }
    HIPCHK(c, hipGetLastError());
    return CELLECTOR_OK;
}

cellector_status donor_genotypes_run(cellector_ctx *c, const uint8_t *assign, const float *prior, uint32_t D,
                                     const cellector_donor_genotypes_params *p, uint64_t *cells, uint64_t *alt, uint64_t *ref, double *q,
                                     uint8_t *gt_out, uint8_t *kind, cellector_donor_genotypes_summary *summary, double *tab, double *pass_ms)
{
    const uint64_t TL = c->total_loci, n = c->nloc, planes = (uint64_t)(D + 1) * 2, sites = (uint64_t)D * TL;
    const bool rule = q || gt_out || kind || summary || tab;
    // every buffer first: on CELLECTOR_ENOMEM nothing has been written
    DevBuf<uint64_t> d_acc;
    DevBuf<uint8_t> d_assign, d_gt, d_kind;
    DevBuf<float> d_prior;
    DevBuf<double> d_tab, d_q;
    DevBuf<uint32_t> d_bad;
    CHK(dev_alloc(c, &d_acc, planes * TL));
    CHK(dev_alloc(c, &d_assign, n));
    if (rule) {
        CHK(dev_alloc(c, &d_tab, TL * 6));
        CHK(dev_alloc(c, &d_gt, sites));
        CHK(dev_alloc(c, &d_kind, sites));
        CHK(dev_alloc(c, &d_bad, 1));
        if (q) CHK(dev_alloc(c, &d_q, sites * 3));
        if (prior) CHK(dev_alloc(c, &d_prior, sites * 3));
    }
    std::vector<uint8_t> h_kind;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    try {
        if (summary && !kind) h_kind.resize(sites);
    } catch (const std::bad_alloc &) {
        return ctx_fail(c, CELLECTOR_ENOMEM, "donor_genotypes: out of host memory");
    }
    struct EventGuard {
        hipEvent_t *ev;
        ~EventGuard() { for (int i = 0; i < 3; i++) if (ev[i]) (void)hipEventDestroy(ev[i]); }
    } guard{ev};
    if (pass_ms)
        for (auto &e : ev) HIPCHK(c, hipEventCreate(&e));

    if (n) HIPCHK(c, hipMemcpyAsync(d_assign, assign, n, hipMemcpyHostToDevice, c->stream));
    if (rule && prior && sites) HIPCHK(c, hipMemcpyAsync(d_prior, prior, sites * 12, hipMemcpyHostToDevice, c->stream));
    if (pass_ms) HIPCHK(c, hipEventRecord(ev[0], c->stream));
    CHK(launch_donor_genotype_tallies(c, d_assign, D, d_acc));
    if (pass_ms) HIPCHK(c, hipEventRecord(ev[1], c->stream));
    if (rule && TL) {
        HIPCHK(c, hipMemsetAsync(d_bad, 0, 4, c->stream));
        hipLaunchKernelGGL(k_dg_tables, dim3((unsigned)((TL + DG_THREADS - 1) / DG_THREADS)), dim3(DG_THREADS), 0, c->stream, TL, D,
                           (const unsigned long long *)d_acc.get(), p->err, p->ambient, d_tab.get());
        hipLaunchKernelGGL(k_dg_posterior, dim3((unsigned)((sites + DG_THREADS - 1) / DG_THREADS)), dim3(DG_THREADS), 0, c->stream, sites, TL,
                           (const unsigned long long *)d_acc.get(), d_tab.get(), prior ? d_prior.get() : nullptr, p->gt_threshold,
                           p->prior_floor, q ? d_q.get() : nullptr, d_gt.get(), d_kind.get(), d_bad.get());
        HIPCHK(c, hipGetLastError());
    }
    if (pass_ms) HIPCHK(c, hipEventRecord(ev[2], c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (the caller's assign and prior have been read)
    if (rule && TL) {
        uint32_t bad = 0;
        CHK(d2h(c, &bad, d_bad, 4));
        if (bad) return ctx_fail(c, CELLECTOR_EDEVICE, "donor_genotypes: the device refused %u rows of prior the host had passed", bad);
    }
    if (pass_ms) {
        float ms = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms, ev[0], ev[1]));
        pass_ms[0] = ms;
        HIPCHK(c, hipEventElapsedTime(&ms, ev[1], ev[2]));
        pass_ms[1] = ms;
    }
    for (uint32_t s = 0; s <= D && TL; s++) {
        if (alt) CHK(d2h(c, alt + (uint64_t)s * TL, d_acc + (uint64_t)s * 2 * TL, TL * 8));
        if (ref) CHK(d2h(c, ref + (uint64_t)s * TL, d_acc + ((uint64_t)s * 2 + 1) * TL, TL * 8));
    }
    if (tab) CHK(d2h(c, tab, d_tab, TL * 6 * 8));
    if (q) CHK(d2h(c, q, d_q, sites * 3 * 8));
    if (gt_out) CHK(d2h(c, gt_out, d_gt, sites));
    if (kind) CHK(d2h(c, kind, d_kind, sites));
    uint64_t n_cells[65] = {};
    for (uint64_t i = 0; i < n; i++) n_cells[assign[i] == 255 ? D : assign[i]]++;
    for (uint32_t s = 0; cells && s <= D; s++) cells[s] = n_cells[s];
    if (summary) {
        memset(summary, 0, sizeof *summary);
        if (!kind) CHK(d2h(c, h_kind.data(), d_kind, sites));
        const uint8_t *const hk = kind ? kind : h_kind.data();  // (the caller's copy, if one was asked for)
        for (uint32_t d = 0; d < D; d++) {
            summary->cells[d] = n_cells[d];
            for (uint64_t t = 0; t < TL; t++) {
                const uint8_t k = hk[(uint64_t)d * TL + t];
                summary->loci_with_reads[d] += k != 0;
                summary->confirmed[d] += k == 1;
                summary->filled[d] += k == 2;
                summary->changed[d] += k == 3;
                summary->withdrawn[d] += k == 4;
            }
        }
    }
    return CELLECTOR_OK;
}
