// The posterior phase of the C ABI: posterior_priors, posterior_alpha_betas, posteriors (kernels_assign.hip; kernels_tiled.hip on engine
// 2), cellector_assign and its host threading (kernels_resolve.hip, assign_host.h), final allele tallies (kernels_genotypes.hip).
#include <cmath>
#include <cstring>
#include <algorithm>
#include <system_error>
#include <thread>
#include <vector>

#include "api_checks.h"
#include "assign_host.h"

// ---- posteriors ---------------------------------------------------------------------------------------
// the minority fraction and the three log priors of calculate_posteriors, from the current exclusion set
struct PosteriorPriors { double mf0, lp_min, lp_maj, lp_dbl; };
static PosteriorPriors posterior_priors(const cellector_ctx *c)
{
    PosteriorPriors p;
    const double N = (double)c->total_cells;
    p.mf0 = ((double)c->n_excluded_global + 1.0) / (N + 1.0);             // main.rs:240
    const double mf = std::fmax(p.mf0, 0.01);                             // main.rs:250
    p.lp_dbl = std::log(N / 1000.0 / 100.0 * std::fmax(mf, 0.1));         // main.rs:259
    p.lp_min = std::log(mf);                                              // main.rs:264-265
    p.lp_maj = std::log(1.0 - mf);
    return p;
}

cellector_status cellector_posterior_alpha_betas(cellector_ctx *c, int which, double *alpha, double *beta)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) {  // per-locus state is replicated: shard 0 answers
        cellector_ctx *s0 = multi_shard0(c);
        const cellector_status st = cellector_posterior_alpha_betas(s0, which, alpha, beta);
        if (st != CELLECTOR_OK) c->err = s0->err;
        return st;
    }
    READY(c);
    REQUIRE(c, c->em_phase == 0, "posterior_alpha_betas: iteration in flight (finish it with cellector_em_finish)");
    REQUIRE(c, which >= 0 && which <= 2, "posterior_alpha_betas: which is 0 (minority), 1 (majority) or 2 (doublet)");
    SETDEV(c);
    const uint64_t L = c->L;
    DevBuf<double> ab6;  // the kernel's [8 L] layout: min, maj, dbl pairs and a pad per locus
    CHK(dev_alloc(c, &ab6, 8 * L));
    CHK(launch_ab_posterior_into(c, posterior_priors(c).mf0, ab6.get()));
    std::vector<double> h(8 * L);
    CHK(d2h(c, h.data(), ab6, 8 * L * sizeof(double)));
    for (uint64_t l = 0; l < L; l++) {
        if (alpha) alpha[l] = h[8 * l + 2 * (uint64_t)which];
        if (beta) beta[l] = h[8 * l + 2 * (uint64_t)which + 1];
    }
    return CELLECTOR_OK;
}

// the posterior phase of a single-device ctx; sdbl (device, [nloc] or null): the doublet set's per-cell sums as well
static cellector_status posteriors_run(cellector_ctx *c, double *posterior, double *doublet, double *ll_maj, double *ll_min,
                                       double *sdbl)
{
    READY(c);
    REQUIRE(c, c->em_phase == 0, "iteration in flight");
    SETDEV(c);
    const PosteriorPriors pr = posterior_priors(c);
    if (c->engine == 2) CHK(tiled_posteriors(c, pr.mf0, pr.lp_min, pr.lp_maj, pr.lp_dbl, sdbl));
    else CHK(launch_posteriors(c, pr.mf0, pr.lp_min, pr.lp_maj, pr.lp_dbl, sdbl));
    const size_t b = c->nloc * 8;
    if (posterior) CHK(d2h(c, posterior, c->post, b));
    if (doublet) CHK(d2h(c, doublet, c->post + c->nloc, b));
    if (ll_maj) CHK(d2h(c, ll_maj, c->post + 2 * c->nloc, b));
    if (ll_min) CHK(d2h(c, ll_min, c->post + 3 * c->nloc, b));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->timing) timer_collect(c);
    return CELLECTOR_OK;
}

cellector_status cellector_posteriors(cellector_ctx *c, double *posterior, double *doublet, double *ll_maj,
                                      double *ll_min)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return multi_posteriors(c, posterior, doublet, ll_maj, ll_min);
    return posteriors_run(c, posterior, doublet, ll_maj, ll_min, nullptr);
}

// ---- posteriors + the labelling rule ------------------------------------------------------------------
// The chain and the rule for the cells [lo, hi) of the list (option resolve_posteriors): per-cell independent, so any split
// over threads gives the same bits.
static void assign_finish_range(const uint32_t *ids, const double *ll3, size_t n_list, size_t lo, size_t hi, double lp_min, double lp_maj,
                                double lp_dbl, double thr, uint64_t min_loci, const uint32_t *ent, double *p, double *d, double *lmaj,
                                double *lmin, uint8_t *pa, uint64_t *q)
{
    for (size_t j = lo; j < hi; j++) {
        const uint32_t i = ids[j];
        const double s_min = ll3[j], s_maj = ll3[n_list + j], s_dbl = ll3[2 * n_list + j];
        assign_posterior(s_min, s_maj, s_dbl, lp_min, lp_maj, lp_dbl, &p[i], &d[i]);
        lmaj[i] = s_maj;
        lmin[i] = s_min;
        pa[i] = assign_label(p[i], d[i], ent[i], thr, min_loci);
        q[i] = assign_qual(p[i]);
    }
}

cellector_status cellector_assign(cellector_ctx *c, double posterior_threshold, uint64_t min_loci_used, double *posterior,
                                  double *doublet, double *ll_maj, double *ll_min, uint8_t *posterior_assignment,
                                  uint8_t *anomaly_assignment, uint64_t *qual)
{
    if (!c) return CELLECTOR_EINVAL;
    const int mode = c->multi ? 0 : c->resolve_posteriors;
    if (!c->multi) {
        READY(c);
        REQUIRE(c, c->em_phase == 0, "iteration in flight");
        REQUIRE(c, !mode || !comm_active(c->comm), "resolve_posteriors works on a single-device ctx");
        c->pa_last_mode = 0;
        c->pa_labels_changed = c->pa_qual_changed = 0;
        c->pa_ids.clear();
    }
    cellector_dims_t dm;
    CHK(cellector_dims(c, &dm));
    const size_t n = c->multi ? (size_t)dm.total_cells : (size_t)(dm.cell_end - dm.cell_begin);
    try {
        std::vector<double> &p = c->pa_host.p, &d = c->pa_host.d, &lmaj = c->pa_host.lmaj, &lmin = c->pa_host.lmin;
        std::vector<uint8_t> &excl = c->pa_host.excl, &pa = c->pa_host.pa;
        std::vector<uint32_t> &ent = c->pa_host.ent;
        std::vector<uint64_t> &q = c->pa_host.q;
        p.resize(n); d.resize(n); lmaj.resize(n); lmin.resize(n);
        excl.resize(n); pa.resize(n); ent.resize(n); q.resize(n);
        if (c->multi) CHK(cellector_posteriors(c, p.data(), d.data(), lmaj.data(), lmin.data()));
        else {
            if (mode == 1 && !c->pa_sdbl) {  // the mark kernel also reads the doublet set's sums
                SETDEV(c);
                CHK(dev_alloc(c, &c->pa_sdbl, c->nloc));
            }
            CHK(posteriors_run(c, p.data(), d.data(), lmaj.data(), lmin.data(), mode == 1 ? c->pa_sdbl.get() : nullptr));
        }
        CHK(cellector_excluded(c, excl.data()));
        CHK(cellector_entries_per_cell(c, ent.data()));
        for (size_t i = 0; i < n; i++) {  // the rule on the device's values
            pa[i] = assign_label(p[i], d[i], ent[i], posterior_threshold, min_loci_used);
            q[i] = assign_qual(p[i]);
        }
        if (mode) {
            SETDEV(c);
            const PosteriorPriors pr = posterior_priors(c);
            const double lp_min = pr.lp_min, lp_maj = pr.lp_maj, lp_dbl = pr.lp_dbl;
            std::vector<uint32_t> ids;
            std::vector<double> ll3;
            CHK(assign_resolve(c, mode, posterior_threshold, lp_min, lp_maj, lp_dbl, &ids, &ll3));
            const size_t m = ids.size();
            std::vector<uint8_t> pa_dev(m);
            std::vector<uint64_t> q_dev(m);
            for (size_t j = 0; j < m; j++) { pa_dev[j] = pa[ids[j]]; q_dev[j] = q[ids[j]]; }
            // ~10 C-library calls a cell: over up to 8 threads when the list is long (each writes its own cells only)
            size_t nt = m / 32768;
            if (nt > 8) nt = 8;
            if (nt < 1) nt = 1;
            std::vector<std::thread> th;
            th.reserve(8);
            size_t done = 0;
            for (size_t t = 1; t < nt; t++) {
                const size_t lo = m * t / nt, hi = m * (t + 1) / nt;
                try {
                    th.emplace_back(assign_finish_range, ids.data(), ll3.data(), m, lo, hi, lp_min, lp_maj, lp_dbl, posterior_threshold,
                                    min_loci_used, ent.data(), p.data(), d.data(), lmaj.data(), lmin.data(), pa.data(), q.data());
                    done = hi;
                } catch (const std::system_error &) {  // no more threads: this one takes the rest
                    break;
                }
            }
            // the first share, and whatever no thread could be made for
            assign_finish_range(ids.data(), ll3.data(), m, 0, m / nt, lp_min, lp_maj, lp_dbl, posterior_threshold, min_loci_used,
                                ent.data(), p.data(), d.data(), lmaj.data(), lmin.data(), pa.data(), q.data());
            if (nt > 1 && done < m)
                assign_finish_range(ids.data(), ll3.data(), m, std::max(done, m / nt), m, lp_min, lp_maj, lp_dbl, posterior_threshold,
                                    min_loci_used, ent.data(), p.data(), d.data(), lmaj.data(), lmin.data(), pa.data(), q.data());
            for (std::thread &t : th) t.join();
            for (size_t j = 0; j < m; j++) {
                c->pa_labels_changed += pa_dev[j] != pa[ids[j]] ? 1 : 0;
                c->pa_qual_changed += q_dev[j] != q[ids[j]] ? 1 : 0;
            }
            c->pa_ids.swap(ids);
            c->pa_last_mode = mode;
        }
        const size_t b = n * 8;
        if (posterior) memcpy(posterior, p.data(), b);
        if (doublet) memcpy(doublet, d.data(), b);
        if (ll_maj) memcpy(ll_maj, lmaj.data(), b);
        if (ll_min) memcpy(ll_min, lmin.data(), b);
        if (posterior_assignment) memcpy(posterior_assignment, pa.data(), n);
        if (anomaly_assignment)
            for (size_t i = 0; i < n; i++) anomaly_assignment[i] = excl[i] ? 0 : 1;  // main.rs:161-163
        if (qual) memcpy(qual, q.data(), b);
    } catch (const std::bad_alloc &) {
        return ctx_fail(c, CELLECTOR_ENOMEM, "cellector_assign: out of host memory");
    }
    return CELLECTOR_OK;
}

cellector_status cellector_assign_resolution(const cellector_ctx *c, cellector_assign_resolution_t *out)
{
    if (!c || !out) return CELLECTOR_EINVAL;
    memset(out, 0, sizeof *out);
    if (c->multi || !c->pa_last_mode) return CELLECTOR_OK;  // (the last cellector_assign resolved nothing)
    out->n_evaluated = c->pa_ids.size();
    out->n_labels_changed = c->pa_labels_changed;
    out->n_qual_changed = c->pa_qual_changed;
    out->mode = (uint32_t)c->pa_last_mode;
    return CELLECTOR_OK;
}

cellector_status cellector_assign_resolved_cells(const cellector_ctx *c, uint32_t *ids)
{
    if (!c || !ids) return CELLECTOR_EINVAL;
    if (c->multi || !c->pa_last_mode) return CELLECTOR_OK;
    if (!c->pa_ids.empty()) memcpy(ids, c->pa_ids.data(), c->pa_ids.size() * sizeof(uint32_t));
    return CELLECTOR_OK;
}

cellector_status cellector_final_allele_tallies(cellector_ctx *c, uint64_t *alt_min, uint64_t *ref_min,
                                                uint64_t *alt_maj, uint64_t *ref_maj)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return multi_final_allele_tallies(c, alt_min, ref_min, alt_maj, ref_maj);
    READY(c);
    REQUIRE(c, c->keep_coo, "final tallies need the staged COO (option keep_coo=1)");
    SETDEV(c);
    const uint64_t TL = c->total_loci;
    DevBuf<uint64_t> d;
    CHK(dev_alloc(c, &d, 4 * TL));
    CHK(launch_final_tallies(c, d));
    std::vector<uint64_t> h(4 * TL);
    CHK(d2h(c, h.data(), d, 4 * TL * 8));
    d.reset();
    if (alt_min) memcpy(alt_min, h.data(), TL * 8);
    if (ref_min) memcpy(ref_min, h.data() + TL, TL * 8);
    if (alt_maj) memcpy(alt_maj, h.data() + 2 * TL, TL * 8);
    if (ref_maj) memcpy(ref_maj, h.data() + 3 * TL, TL * 8);
    return CELLECTOR_OK;
}
