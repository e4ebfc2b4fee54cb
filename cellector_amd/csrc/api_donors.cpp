// The genotype models of the C ABI: donor calls from hard calls and from genotype probabilities and the donor fit
// (kernels_donors.hip), donor panels (kernels_donor_panel.hip), ambient fractions (kernels_ambient.hip), donor pair fractions (kernels_pair_fraction.hip) and donor genotype
// refinement (kernels_donor_genotypes.hip).  Every call opens with model_call_scope (api_checks.h), then its argument checks.
#include "api_checks.h"

#include <vector>

// ---- donor demultiplexing: kernels_donors.hip -------------------------------------------------------------------
cellector_status cellector_donor_default_params(cellector_donor_params *out)
{
    if (!out) return CELLECTOR_EINVAL;
    out->err = 0.01;
    out->ambient = 0.03;
    out->doublet_rate = 0.1;
    out->posterior_threshold = 0.999;
    out->min_loci = 1;
    return CELLECTOR_OK;
}

// gt [n, total_loci] of n donors or sources (noun: what the message calls them): every value is one of the four codes
static cellector_status gt_values_check(cellector_ctx *c, const char *what, const char *noun, const uint8_t *gt, uint32_t n)
{
    const uint64_t TL = c->total_loci;
    for (uint32_t d = 0; d < n; d++)
        for (uint64_t t = 0; t < TL; t++)
            if (gt[(uint64_t)d * TL + t] > 3)
                return ctx_fail(c, CELLECTOR_EINVAL, "%s: gt of %s %u at locus %llu is %u: 0 = 0/0, 1 = 0/1, 2 = 1/1, 3 = no call", what, noun, d,
                                (unsigned long long)t, (unsigned)gt[(uint64_t)d * TL + t]);
    return CELLECTOR_OK;
}
// the arguments of a donor call, behind its model_call_scope
static cellector_status donor_args_check(cellector_ctx *c, const char *what, const uint8_t *gt, uint32_t D, const cellector_donor_params *p)
{
    CHK(donor_count_check(c, what, gt, "gt", D));
    CHK(donor_params_check(c, what, p));
    return gt_values_check(c, what, "donor", gt, D);
}
// the soft calls: every row of gp is three NaN (no call) or three finite weights >= 0 that are not all zero
static cellector_status donor_gp_check(cellector_ctx *c, const char *what, const float *gp, uint32_t D, const cellector_donor_params *p)
{
    CHK(donor_count_check(c, what, gp, "gp", D));
    CHK(donor_params_check(c, what, p));
    const uint64_t TL = c->total_loci;
    for (uint32_t d = 0; d < D; d++)
        for (uint64_t t = 0; t < TL; t++) {
            const float *r = gp + ((uint64_t)d * TL + t) * 3;
            if (std::isnan(r[0]) && std::isnan(r[1]) && std::isnan(r[2])) continue;
            bool fine = r[0] > 0.f || r[1] > 0.f || r[2] > 0.f;
            for (int g = 0; g < 3; g++) fine = fine && r[g] >= 0.f && std::isfinite(r[g]);
            if (!fine)
                return ctx_fail(c, CELLECTOR_EINVAL, "%s: gp of donor %u at locus %llu is (%g, %g, %g): three NaN (no call), or three finite weights >= 0 that are not all zero",
                                what, d, (unsigned long long)t, (double)r[0], (double)r[1], (double)r[2]);
        }
    return CELLECTOR_OK;
}

cellector_status cellector_donor_tables(cellector_ctx *c, const uint8_t *gt, uint32_t n_donors, const cellector_donor_params *p,
                                        const uint8_t *mask, double *tab1, double *tab2, uint64_t *packed)
{
    if (!c) return CELLECTOR_EINVAL;
    cellector_donor_params prm = params_or_default(cellector_donor_default_params, p);
    CHK(model_call_scope(c, "donor_tables"));
    CHK(donor_args_check(c, "donor_tables", gt, n_donors, &prm));
    SETDEV(c);
    return donor_tables_run(c, gt, n_donors, &prm, mask, tab1, tab2, packed);
}

// the prior and the anchors of a cell call (u8 anchors, or the panel's u16); lp [D]: the caller's prior, or zeros
template <class Anchor>
static cellector_status donor_prior_anchor_check(cellector_ctx *c, const char *what, uint32_t D, const double *log_prior, const Anchor *anchor,
                                                 double *lp)
{
    bool any = !log_prior;
    for (uint32_t d = 0; log_prior && d < D; d++) {
        if (std::isnan(log_prior[d]) || log_prior[d] == INFINITY)
            return ctx_fail(c, CELLECTOR_EINVAL, "%s: log_prior[%u] = %g is neither a finite value nor -inf", what, d, log_prior[d]);
        any = any || log_prior[d] != -INFINITY;
        lp[d] = log_prior[d];
    }
    if (!any) return ctx_fail(c, CELLECTOR_EINVAL, "%s: log_prior is -inf for every donor", what);
    for (uint64_t i = 0; anchor && i < c->nloc; i++)
        if (anchor[i] >= D)
            return ctx_fail(c, CELLECTOR_EINVAL, "%s: anchor of cell %llu is %u, not below the %u donors", what, (unsigned long long)i,
                            (unsigned)anchor[i], D);
    return CELLECTOR_OK;
}

// cellector_donor_posteriors (gp null) and cellector_donor_posteriors_gp (gt null): the same checks, the same run
static cellector_status donor_posteriors_call(cellector_ctx *c, const char *what, const uint8_t *gt, const float *gp, uint32_t n_donors,
                                              const cellector_donor_params *p, const double *log_prior, const uint8_t *anchor,
                                              const uint8_t *mask, double *ll, double *pair_ll, double *posterior, double *pair_posterior,
                                              double *doublet_posterior, uint8_t *best, uint8_t *second, uint8_t *best_pair,
                                              uint32_t *n_entries, uint8_t *status, uint8_t *anchor_out, cellector_donor_summary *out,
                                              double *tab1, double *tab2, bool soft)
{
    if (!c) return CELLECTOR_EINVAL;
    cellector_donor_params prm = params_or_default(cellector_donor_default_params, p);
    CHK(model_call_scope(c, what));
    CHK(soft ? donor_gp_check(c, what, gp, n_donors, &prm) : donor_args_check(c, what, gt, n_donors, &prm));
    const uint32_t D = n_donors;
    double lp[64] = {};
    CHK(donor_prior_anchor_check(c, what, D, log_prior, anchor, lp));
    const double log_singlet = std::log(1.0 - prm.doublet_rate);
    const double log_pair = D > 1 ? std::log(prm.doublet_rate / (double)(D - 1)) : 0.0;
    SETDEV(c);
    return donor_posteriors_run(c, gt, gp, D, &prm, lp, anchor, mask, log_singlet, log_pair, ll, pair_ll, posterior, pair_posterior,
                                doublet_posterior, best, second, best_pair, n_entries, status, anchor_out, out, tab1, tab2, nullptr);
}

cellector_status cellector_donor_posteriors(cellector_ctx *c, const uint8_t *gt, uint32_t n_donors, const cellector_donor_params *p,
                                            const double *log_prior, const uint8_t *anchor, const uint8_t *mask, double *ll, double *pair_ll,
                                            double *posterior, double *pair_posterior, double *doublet_posterior, uint8_t *best,
                                            uint8_t *second, uint8_t *best_pair, uint32_t *n_entries, uint8_t *status, uint8_t *anchor_out,
                                            cellector_donor_summary *out, double *tab1, double *tab2)
{
    return donor_posteriors_call(c, "donor_posteriors", gt, nullptr, n_donors, p, log_prior, anchor, mask, ll, pair_ll, posterior, pair_posterior,
                                 doublet_posterior, best, second, best_pair, n_entries, status, anchor_out, out, tab1, tab2, false);
}

cellector_status cellector_match_donors(cellector_ctx *c, const uint8_t *labels, uint32_t n_classes, const uint8_t *gt, uint32_t n_donors,
                                        const cellector_donor_params *p, const uint8_t *mask, double *ll, uint8_t *best, double *margin,
                                        uint64_t *cells)
{
    if (!c) return CELLECTOR_EINVAL;
    cellector_donor_params prm = params_or_default(cellector_donor_default_params, p);
    CHK(class_call_check(c, "match_donors", labels, n_classes, nullptr, nullptr));
    CHK(donor_args_check(c, "match_donors", gt, n_donors, &prm));
    SETDEV(c);
    return donor_match_run(c, labels, n_classes, gt, nullptr, n_donors, &prm, mask, ll, best, margin, cells);
}

// ---- donor panels: kernels_donor_panel.hip --------------------------------------------------------------------------
// how many donors a panel holds, is gt there, are the parameters and the calls in range
static cellector_status panel_args_check(cellector_ctx *c, const char *what, const uint8_t *gt, uint32_t D, const cellector_donor_params *p)
{
    if (D < 1 || D > 4096) return ctx_fail(c, CELLECTOR_EINVAL, "%s: %u donors, 1..4096 are supported", what, D);
    if (!gt) return ctx_fail(c, CELLECTOR_EINVAL, "%s: null gt", what);
    CHK(donor_params_check(c, what, p));
    return gt_values_check(c, what, "donor", gt, D);
}

cellector_status cellector_donor_panel(cellector_ctx *c, const uint8_t *gt, uint32_t n_donors, uint32_t shortlist, const cellector_donor_params *p,
                                       const double *log_prior, const uint16_t *anchor, const uint8_t *mask, uint16_t *cand, double *cand_ll,
                                       double *cand_pair_ll, double *cand_posterior, double *cand_pair_posterior, double *doublet_posterior,
                                       double *best_posterior, uint16_t *best, uint16_t *second, uint16_t *best_pair, uint16_t *anchor_out,
                                       uint32_t *n_entries, uint8_t *status, uint64_t *donor_cells, cellector_donor_panel_summary *out,
                                       double *ll, uint64_t *packed, double *tab1, double *tab2)
{
    if (!c) return CELLECTOR_EINVAL;
    const char *what = "donor_panel";
    cellector_donor_params prm = params_or_default(cellector_donor_default_params, p);
    CHK(model_call_scope(c, what));
    CHK(panel_args_check(c, what, gt, n_donors, &prm));
    const uint32_t D = n_donors;
    if (shortlist < 1 || shortlist > 64) return ctx_fail(c, CELLECTOR_EINVAL, "%s: a shortlist of %u, 1..64 are supported", what, shortlist);
    std::vector<double> lp(D, 0.0);
    CHK(donor_prior_anchor_check(c, what, D, log_prior, anchor, lp.data()));
    const double log_singlet = std::log(1.0 - prm.doublet_rate);
    const double log_pair = D > 1 ? std::log(prm.doublet_rate / (double)(D - 1)) : 0.0;
    SETDEV(c);
    return donor_panel_run(c, gt, D, shortlist < D ? shortlist : D, &prm, lp.data(), anchor, mask, log_singlet, log_pair, cand, cand_ll,
                           cand_pair_ll, cand_posterior, cand_pair_posterior, doublet_posterior, best_posterior, best, second, best_pair,
                           anchor_out, n_entries, status, donor_cells, out, ll, packed, tab1, tab2);
}

cellector_status cellector_match_donors_panel(cellector_ctx *c, const uint8_t *labels, uint32_t n_classes, const uint8_t *gt, uint32_t n_donors,
                                              const cellector_donor_params *p, const uint8_t *mask, double *ll, uint16_t *best, double *margin,
                                              uint64_t *cells)
{
    if (!c) return CELLECTOR_EINVAL;
    cellector_donor_params prm = params_or_default(cellector_donor_default_params, p);
    CHK(class_call_check(c, "match_donors_panel", labels, n_classes, nullptr, nullptr));
    CHK(panel_args_check(c, "match_donors_panel", gt, n_donors, &prm));
    SETDEV(c);
    return donor_panel_match_run(c, labels, n_classes, gt, n_donors, &prm, mask, ll, best, margin, cells);
}

// ---- the fit of the called hypothesis: k_donor_moments and k_donor_fit of kernels_donors.hip -------------------------------------
cellector_status cellector_donor_fit_default_params(cellector_donor_fit_params *out)
{
    if (!out) return CELLECTOR_EINVAL;
    out->iqr_multiple = 3.0;
    out->min_cells = 8;
    return CELLECTOR_OK;
}

cellector_status cellector_donor_moment_tables(cellector_ctx *c, const cellector_donor_params *p, const uint8_t *mask, double *mom1, double *mom2)
{
    if (!c) return CELLECTOR_EINVAL;
    cellector_donor_params prm = params_or_default(cellector_donor_default_params, p);
    CHK(model_call_scope(c, "donor_moment_tables"));
    CHK(donor_params_check(c, "donor_moment_tables", &prm));
    SETDEV(c);
    return donor_moment_tables_run(c, &prm, mask, mom1, mom2);
}

cellector_status cellector_donor_fit(cellector_ctx *c, const uint8_t *gt, uint32_t n_donors, const cellector_donor_params *p,
                                     const cellector_donor_fit_params *fit, const double *log_prior, const uint8_t *anchor, const uint8_t *mask,
                                     double *fit_e, double *fit_v, double *pair_e, double *pair_v, double *z, double *pair_z, double *call_z,
                                     uint8_t *hyp_a, uint8_t *hyp_b, uint8_t *status, uint8_t *unmatched, cellector_donor_fit_summary *out,
                                     double *mom1, double *mom2)
{
    if (!c) return CELLECTOR_EINVAL;
    cellector_donor_params prm = params_or_default(cellector_donor_default_params, p);
    cellector_donor_fit_params fp = params_or_default(cellector_donor_fit_default_params, fit);
    CHK(model_call_scope(c, "donor_fit"));
    CHK(donor_args_check(c, "donor_fit", gt, n_donors, &prm));
    if (!(fp.iqr_multiple >= 0.0)) return ctx_fail(c, CELLECTOR_EINVAL, "donor_fit: iqr_multiple = %g is not a value >= 0", fp.iqr_multiple);
    if (fp.min_cells < 4) return ctx_fail(c, CELLECTOR_EINVAL, "donor_fit: min_cells must be at least 4");
    const uint32_t D = n_donors;
    double lp[64] = {};
    CHK(donor_prior_anchor_check(c, "donor_fit", D, log_prior, anchor, lp));
    const double log_singlet = std::log(1.0 - prm.doublet_rate);
    const double log_pair = D > 1 ? std::log(prm.doublet_rate / (double)(D - 1)) : 0.0;
    SETDEV(c);
    return donor_fit_run(c, gt, D, &prm, &fp, lp, anchor, mask, log_singlet, log_pair, fit_e, fit_v, pair_e, pair_v, z, pair_z, call_z, hyp_a,
                         hyp_b, status, unmatched, out, mom1, mom2);
}

// ---- the donor calls from genotype probabilities: the soft kernels of kernels_donors.hip ------------------------------------------
cellector_status cellector_donor_posteriors_gp(cellector_ctx *c, const float *gp, uint32_t n_donors, const cellector_donor_params *p,
                                               const double *log_prior, const uint8_t *anchor, const uint8_t *mask, double *ll, double *pair_ll,
                                               double *posterior, double *pair_posterior, double *doublet_posterior, uint8_t *best,
                                               uint8_t *second, uint8_t *best_pair, uint32_t *n_entries, uint8_t *status, uint8_t *anchor_out,
                                               cellector_donor_summary *out, double *tab1, double *tab2)
{
    return donor_posteriors_call(c, "donor_posteriors_gp", nullptr, gp, n_donors, p, log_prior, anchor, mask, ll, pair_ll, posterior,
                                 pair_posterior, doublet_posterior, best, second, best_pair, n_entries, status, anchor_out, out, tab1, tab2, true);
}

cellector_status cellector_donor_weights(cellector_ctx *c, const float *gp, uint32_t n_donors, double *w, uint8_t *kind)
{
    if (!c) return CELLECTOR_EINVAL;
    cellector_donor_params prm = params_or_default(cellector_donor_default_params, (const cellector_donor_params *)nullptr);
    CHK(model_call_scope(c, "donor_weights"));
    CHK(donor_gp_check(c, "donor_weights", gp, n_donors, &prm));
    SETDEV(c);
    return donor_weights_run(c, gp, n_donors, w, kind);
}

cellector_status cellector_match_donors_gp(cellector_ctx *c, const uint8_t *labels, uint32_t n_classes, const float *gp, uint32_t n_donors,
                                           const cellector_donor_params *p, const uint8_t *mask, double *ll, uint8_t *best, double *margin,
                                           uint64_t *cells)
{
    if (!c) return CELLECTOR_EINVAL;
    cellector_donor_params prm = params_or_default(cellector_donor_default_params, p);
    CHK(class_call_check(c, "match_donors_gp", labels, n_classes, nullptr, nullptr));
    CHK(donor_gp_check(c, "match_donors_gp", gp, n_donors, &prm));
    SETDEV(c);
    return donor_match_run(c, labels, n_classes, nullptr, gp, n_donors, &prm, mask, ll, best, margin, cells);
}

// ---- ambient fraction estimation: kernels_ambient.hip --------------------------------------------------------------
cellector_status cellector_ambient_default_params(cellector_ambient_params *out)
{
    if (!out) return CELLECTOR_EINVAL;
    out->err = 0.01;
    out->lo = 0.0;
    out->hi = 0.5;
    out->grid = 16;
    out->rounds = 3;
    out->min_loci = 1;
    return CELLECTOR_OK;
}

// what every ambient call checks before anything is written or launched: the scope of the donor calls, then the arguments all share
static cellector_status ambient_scope_check(cellector_ctx *c, const char *what, uint32_t G, double err)
{
    CHK(model_call_scope(c, what));
    if (G < 4 || G > 32) return ctx_fail(c, CELLECTOR_EINVAL, "%s: %u grid points, 4..32 are supported", what, G);
    if (!(err > 0.0 && err < 0.5)) return ctx_fail(c, CELLECTOR_EINVAL, "%s: err = %g is not within (0, 0.5)", what, err);
    return CELLECTOR_OK;
}
static cellector_status ambient_grid_check(cellector_ctx *c, const char *what, const double *rho, uint32_t G)
{
    if (!rho) return ctx_fail(c, CELLECTOR_EINVAL, "%s: null rho", what);
    for (uint32_t j = 0; j < G; j++)
        if (!(rho[j] >= 0.0 && rho[j] < 1.0)) return ctx_fail(c, CELLECTOR_EINVAL, "%s: rho[%u] = %g is not within [0, 1)", what, j, rho[j]);
    return CELLECTOR_OK;
}
static cellector_status ambient_sources_check(cellector_ctx *c, const char *what, const uint8_t *gt, uint32_t S, const uint8_t *assign,
                                              uint64_t min_loci)
{
    if (S < 1 || S > 64) return ctx_fail(c, CELLECTOR_EINVAL, "%s: %u sources, 1..64 are supported", what, S);
    if (!gt) return ctx_fail(c, CELLECTOR_EINVAL, "%s: null gt", what);
    if (!assign) return ctx_fail(c, CELLECTOR_EINVAL, "%s: null assign", what);
    if (min_loci < 1) return ctx_fail(c, CELLECTOR_EINVAL, "%s: min_loci must be at least 1", what);
    CHK(gt_values_check(c, what, "source", gt, S));
    for (uint64_t i = 0; i < c->nloc; i++)
        if (assign[i] != 255 && assign[i] >= S)
            return ctx_fail(c, CELLECTOR_EINVAL, "%s: assign of cell %llu is %u, neither 255 nor below the %u sources", what,
                            (unsigned long long)i, (unsigned)assign[i], S);
    return CELLECTOR_OK;
}

cellector_status cellector_ambient_tables(cellector_ctx *c, const double *rho, uint32_t n_grid, double err, const uint8_t *mask, double *tab)
{
    if (!c) return CELLECTOR_EINVAL;
    CHK(ambient_scope_check(c, "ambient_tables", n_grid, err));
    CHK(ambient_grid_check(c, "ambient_tables", rho, n_grid));
    SETDEV(c);
    return ambient_tables_run(c, rho, n_grid, err, mask, tab);
}

cellector_status cellector_ambient_profile(cellector_ctx *c, const uint8_t *gt, uint32_t n_sources, const uint8_t *assign, const double *rho,
                                           uint32_t n_grid, double err, uint64_t min_loci, const uint8_t *mask, double *ll, double *total,
                                           double *source_total, uint64_t *source_cells, uint32_t *n_entries, double *cell_rho,
                                           double *cell_se, double *tab)
{
    if (!c) return CELLECTOR_EINVAL;
    CHK(ambient_scope_check(c, "ambient_profile", n_grid, err));
    CHK(ambient_grid_check(c, "ambient_profile", rho, n_grid));
    CHK(ambient_sources_check(c, "ambient_profile", gt, n_sources, assign, min_loci));
    SETDEV(c);
    return ambient_profile_run(c, gt, n_sources, assign, rho, n_grid, err, min_loci, mask, ll, total, source_total, source_cells, n_entries,
                               cell_rho, cell_se, tab);
}

cellector_status cellector_estimate_ambient(cellector_ctx *c, const uint8_t *gt, uint32_t n_sources, const uint8_t *assign,
                                            const cellector_ambient_params *params, const uint8_t *mask, cellector_ambient_summary *summary,
                                            double *cell_rho, double *cell_se, uint32_t *n_entries)
{
    if (!c) return CELLECTOR_EINVAL;
    cellector_ambient_params prm = params_or_default(cellector_ambient_default_params, params);
    CHK(ambient_scope_check(c, "estimate_ambient", prm.grid, prm.err));
    if (!(prm.lo >= 0.0 && prm.lo < prm.hi && prm.hi < 1.0))
        return ctx_fail(c, CELLECTOR_EINVAL, "estimate_ambient: lo = %g, hi = %g do not satisfy 0 <= lo < hi < 1", prm.lo, prm.hi);
    if (prm.rounds < 1 || prm.rounds > 8) return ctx_fail(c, CELLECTOR_EINVAL, "estimate_ambient: %u rounds, 1..8 are supported", prm.rounds);
    CHK(ambient_sources_check(c, "estimate_ambient", gt, n_sources, assign, prm.min_loci));
    SETDEV(c);
    return ambient_estimate_run(c, gt, n_sources, assign, &prm, mask, summary, cell_rho, cell_se, n_entries);
}

// ---- donor pair fractions: kernels_pair_fraction.hip ----------------------------------------------------------------
cellector_status cellector_pair_fraction_default_params(cellector_pair_fraction_params *out)
{
    if (!out) return CELLECTOR_EINVAL;
    out->min_fraction = 0.1;
    out->min_loci = 1;
    return CELLECTOR_OK;
}

// the grid of a pair fraction call: the caller's, checked, or the default j / 16.0; grid [32] receives it
static cellector_status pair_fraction_grid_check(cellector_ctx *c, const char *what, const double *frac, uint32_t *G, double *grid)
{
    if (!frac) {
        *G = 17;
        for (uint32_t j = 0; j < 17; j++) grid[j] = (double)j / 16.0;
        return CELLECTOR_OK;
    }
    if (*G < 4 || *G > 32) return ctx_fail(c, CELLECTOR_EINVAL, "%s: %u grid points, 4..32 are supported", what, *G);
    for (uint32_t j = 0; j < *G; j++) {
        if (!(frac[j] >= 0.0 && frac[j] <= 1.0)) return ctx_fail(c, CELLECTOR_EINVAL, "%s: frac[%u] = %g is not within [0, 1]", what, j, frac[j]);
        if (j && !(frac[j] > frac[j - 1]))
            return ctx_fail(c, CELLECTOR_EINVAL, "%s: frac[%u] = %g is not above frac[%u] = %g: the grid ascends strictly", what, j, frac[j],
                            j - 1, frac[j - 1]);
        grid[j] = frac[j];
    }
    return CELLECTOR_OK;
}

cellector_status cellector_pair_fraction_tables(cellector_ctx *c, const cellector_donor_params *donor_params, const double *frac, uint32_t n_grid,
                                                const uint8_t *mask, double *tab)
{
    if (!c) return CELLECTOR_EINVAL;
    cellector_donor_params prm = params_or_default(cellector_donor_default_params, donor_params);
    CHK(model_call_scope(c, "pair_fraction_tables"));
    CHK(donor_params_check(c, "pair_fraction_tables", &prm));
    double grid[32];
    uint32_t G = n_grid;
    CHK(pair_fraction_grid_check(c, "pair_fraction_tables", frac, &G, grid));
    SETDEV(c);
    return pair_fraction_tables_run(c, &prm, grid, G, mask, tab);
}

cellector_status cellector_donor_pair_fractions(cellector_ctx *c, const uint8_t *gt, uint32_t n_donors, const cellector_donor_params *donor_params,
                                                const cellector_pair_fraction_params *params, const uint8_t *pair_a, const uint8_t *pair_b,
                                                const double *frac, uint32_t n_grid, const uint8_t *mask, double *ll, uint32_t *n_entries,
                                                double *cell_frac, double *cell_se, uint8_t *j_star, uint8_t *kind,
                                                cellector_pair_fraction_summary *summary, double *tab)
{
    if (!c) return CELLECTOR_EINVAL;
    const char *what = "donor_pair_fractions";
    cellector_donor_params prm = params_or_default(cellector_donor_default_params, donor_params);
    cellector_pair_fraction_params fp = params_or_default(cellector_pair_fraction_default_params, params);
    CHK(model_call_scope(c, what));
    CHK(donor_args_check(c, what, gt, n_donors, &prm));
    const uint32_t D = n_donors;
    if (!pair_a) return ctx_fail(c, CELLECTOR_EINVAL, "%s: null pair_a", what);
    if (!pair_b) return ctx_fail(c, CELLECTOR_EINVAL, "%s: null pair_b", what);
    for (uint64_t i = 0; i < c->nloc; i++) {
        if (pair_a[i] == 255) continue;
        if (pair_a[i] >= D)
            return ctx_fail(c, CELLECTOR_EINVAL, "%s: pair_a of cell %llu is %u, neither 255 nor below the %u donors", what, (unsigned long long)i,
                            (unsigned)pair_a[i], D);
        if (pair_b[i] >= D)
            return ctx_fail(c, CELLECTOR_EINVAL, "%s: pair_b of cell %llu is %u, not below the %u donors", what, (unsigned long long)i,
                            (unsigned)pair_b[i], D);
        if (pair_b[i] == pair_a[i])
            return ctx_fail(c, CELLECTOR_EINVAL, "%s: pair_b of cell %llu is %u, its pair_a: a pair is two donors", what, (unsigned long long)i,
                            (unsigned)pair_b[i]);
    }
    double grid[32];
    uint32_t G = n_grid;
    CHK(pair_fraction_grid_check(c, what, frac, &G, grid));
    if (!(fp.min_fraction >= 0.0 && fp.min_fraction <= 0.5))
        return ctx_fail(c, CELLECTOR_EINVAL, "%s: min_fraction = %g is not within [0, 0.5]", what, fp.min_fraction);
    if (fp.min_loci < 1) return ctx_fail(c, CELLECTOR_EINVAL, "%s: min_loci must be at least 1", what);
    SETDEV(c);
    return pair_fractions_run(c, gt, D, &prm, &fp, pair_a, pair_b, grid, G, mask, ll, n_entries, cell_frac, cell_se, j_star, kind, summary, tab);
}

// ---- donor genotype refinement: kernels_donor_genotypes.hip ------------------------------------------------
cellector_status cellector_donor_genotypes_default_params(cellector_donor_genotypes_params *out)
{
    if (!out) return CELLECTOR_EINVAL;
    out->err = 0.01;
    out->ambient = 0.03;
    out->gt_threshold = 0.99;
    out->prior_floor = 0.01;
    return CELLECTOR_OK;
}

cellector_status cellector_donor_genotypes(cellector_ctx *c, const uint8_t *assign, const float *prior, uint32_t n_donors,
                                           const cellector_donor_genotypes_params *params, uint64_t *cells, uint64_t *alt, uint64_t *ref,
                                           double *q, uint8_t *gt_out, uint8_t *kind, cellector_donor_genotypes_summary *summary, double *tab,
                                           double *pass_ms)
{
    if (!c) return CELLECTOR_EINVAL;
    const char *what = "donor_genotypes";
    cellector_donor_genotypes_params prm = params_or_default(cellector_donor_genotypes_default_params, params);
    CHK(model_call_scope(c, what));
    cellector_donor_params dp;  // (err and ambient are the donor call's, and so are their checks)
    cellector_donor_default_params(&dp);
    dp.err = prm.err;
    dp.ambient = prm.ambient;
    const uint32_t D = n_donors;
    if (D < 1 || D > 64) return ctx_fail(c, CELLECTOR_EINVAL, "%s: %u donors, 1..64 are supported", what, D);
    CHK(donor_params_check(c, what, &dp));
    if (!(prm.gt_threshold >= 0.0 && prm.gt_threshold <= 1.0))
        return ctx_fail(c, CELLECTOR_EINVAL, "%s: gt_threshold = %g is not within [0, 1]", what, prm.gt_threshold);
    if (!(prm.prior_floor >= 0.0 && prm.prior_floor <= 1.0))
        return ctx_fail(c, CELLECTOR_EINVAL, "%s: prior_floor = %g is not within [0, 1]", what, prm.prior_floor);
    if (!assign) return ctx_fail(c, CELLECTOR_EINVAL, "%s: null assign", what);
    for (uint64_t i = 0; i < c->nloc; i++)
        if (assign[i] >= D && assign[i] != 255)
            return ctx_fail(c, CELLECTOR_EINVAL, "%s: assign of cell %llu is %u, neither below the %u donors nor 255 (no part)", what,
                            (unsigned long long)i, (unsigned)assign[i], D);
    if (prior) CHK(donor_gp_check(c, what, prior, D, &dp));
    REQUIRE(c, c->keep_coo && (c->coo.locus || !c->nnz), "donor_genotypes needs the staged COO (option keep_coo=1)");
    SETDEV(c);
    return donor_genotypes_run(c, assign, prior, D, &prm, cells, alt, ref, q, gt_out, kind, summary, tab, pass_ms);
}
