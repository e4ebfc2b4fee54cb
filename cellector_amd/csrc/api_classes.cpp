// The label models of the C ABI: K-genotype classes and their doublet classes (kernels_classes.hip), clusters without labels
// (kernels_cluster.hip), class genotypes (kernels_genotypes.hip, genotype_host.h).  class_call_check is in api_checks.h.
#include <cstring>
#include <vector>

#include "api_checks.h"
#include "genotype_host.h"

// ---- K-genotype classes: kernels_classes.hip ------------------------------------------------------------
// step 1 of the class model: the exact integer tallies of a labelling (main.rs:598-611 sums the same counts for two classes)
cellector_status cellector_class_tallies(cellector_ctx *c, const uint8_t *labels, uint32_t n_classes, uint64_t *cells, uint64_t *alt,
                                         uint64_t *ref)
{
    if (!c) return CELLECTOR_EINVAL;
    CHK(class_call_check(c, "class_tallies", labels, n_classes, nullptr, nullptr));
    SETDEV(c);
    return classes_tallies_run(c, labels, n_classes, nullptr, cells, alt, ref, nullptr, nullptr);
}

// step 2: init_alpha_betas (main.rs:598-611) for K classes
cellector_status cellector_class_alpha_betas(cellector_ctx *c, const uint8_t *labels, uint32_t n_classes, const double *scale, double *alpha,
                                             double *beta)
{
    if (!c) return CELLECTOR_EINVAL;
    CHK(class_call_check(c, "class_alpha_betas", labels, n_classes, scale, nullptr));
    SETDEV(c);
    return classes_tallies_run(c, labels, n_classes, scale, nullptr, nullptr, nullptr, alpha, beta);
}

// steps 1-6: get_cell_log_likelihoods (main.rs:541-591) per class and the prior / logsumexp chain of main.rs:264-276 over K terms
cellector_status cellector_class_posteriors(cellector_ctx *c, const uint8_t *labels, uint32_t n_classes, const double *scale,
                                            const double *log_prior, const uint8_t *mask, double *ll, double *posterior, uint8_t *best,
                                            uint64_t *qual)
{
    if (!c) return CELLECTOR_EINVAL;
    CHK(class_call_check(c, "class_posteriors", labels, n_classes, scale, log_prior));
    SETDEV(c);
    const cellector_status st = classes_run(c, labels, n_classes, scale, log_prior, mask, 0, 1, nullptr, nullptr, ll, posterior, best, qual);
    if (c->timing) timer_collect(c);
    return st;
}

// step 7: the hard-EM loop over steps 1-6 (the outer loop of main.rs:42-46, with K classes in place of the exclusion set)
cellector_status cellector_refine_classes(cellector_ctx *c, uint8_t *labels, uint32_t n_classes, const double *scale, const double *log_prior,
                                          const uint8_t *mask, uint32_t max_iter, uint64_t min_loci, cellector_refine_summary *out, double *ll,
                                          double *posterior, uint64_t *qual)
{
    if (!c) return CELLECTOR_EINVAL;
    CHK(class_call_check(c, "refine_classes", labels, n_classes, scale, log_prior));
    REQUIRE(c, min_loci >= 1, "refine_classes: min_loci must be at least 1");
    SETDEV(c);
    const cellector_status st = classes_run(c, labels, n_classes, scale, log_prior, mask, max_iter, min_loci, labels, out, ll, posterior,
                                            nullptr, qual);
    if (c->timing) timer_collect(c);
    return st;
}

// ---- doublet classes over the K classes: the second half of kernels_classes.hip ------------------------------
// what the doublet calls check on top of class_call_check: a live class must remain once the held cells are out
static cellector_status doublet_call_check(cellector_ctx *c, const char *what, const uint8_t *labels, const uint8_t *held, uint32_t K,
                                           const double *scale, const double *pair_scale, const double *log_prior,
                                           const double *log_pair_prior)
{
    CHK(class_call_check(c, what, labels, K, scale, log_prior));
    bool any = !held;
    for (uint64_t i = 0; held && !any && i < c->nloc; i++) any = labels[i] != 255 && !held[i];
    if (!any) return ctx_fail(c, CELLECTOR_EINVAL, "%s: every labelled cell is held: all %u classes are dead", what, K);
    for (uint32_t k = 0; pair_scale && k < K; k++)
        if (!std::isfinite(pair_scale[k]) || pair_scale[k] < 0.0)
            return ctx_fail(c, CELLECTOR_EINVAL, "%s: pair_scale[%u] = %g is not a finite value >= 0", what, k, pair_scale[k]);
    for (uint32_t p = 0; log_pair_prior && p < K * (K - 1) / 2; p++)
        if (std::isnan(log_pair_prior[p])) return ctx_fail(c, CELLECTOR_EINVAL, "%s: log_pair_prior[%u] is NaN", what, p);
    return CELLECTOR_OK;
}

// step 3 of the doublet model: the P pair distributions (main.rs:245-246 for K = 2)
cellector_status cellector_class_pair_alpha_betas(cellector_ctx *c, const uint8_t *labels, const uint8_t *held, uint32_t n_classes,
                                                  const double *pair_scale, double *alpha, double *beta)
{
    if (!c) return CELLECTOR_EINVAL;
    CHK(doublet_call_check(c, "class_pair_alpha_betas", labels, held, n_classes, nullptr, pair_scale, nullptr, nullptr));
    SETDEV(c);
    return class_pairs_run(c, labels, held, n_classes, pair_scale, alpha, beta);
}

// steps 1-6: the K singlets and the P pairs in one chain (calculate_posteriors, main.rs:228-280, is K = 2), and the call of
// main.rs:150
cellector_status cellector_class_doublets(cellector_ctx *c, const uint8_t *labels, const uint8_t *held, uint32_t n_classes,
                                          const double *scale, const double *pair_scale, const double *log_prior,
                                          const double *log_pair_prior, const uint8_t *mask, double *ll, double *ll_pair, double *posterior,
                                          double *doublet_posterior, uint8_t *best, uint8_t *best_pair, uint8_t *call, uint64_t *qual)
{
    if (!c) return CELLECTOR_EINVAL;
    CHK(doublet_call_check(c, "class_doublets", labels, held, n_classes, scale, pair_scale, log_prior, log_pair_prior));
    SETDEV(c);
    const cellector_status st = class_doublets_run(c, labels, held, n_classes, scale, pair_scale, log_prior, log_pair_prior, mask, 0.5, 0, 1,
                                                   nullptr, nullptr, nullptr, ll, ll_pair, posterior, doublet_posterior, best, best_pair, call,
                                                   qual);
    if (c->timing) timer_collect(c);
    return st;
}

// step 7: the held-out refine
cellector_status cellector_refine_class_doublets(cellector_ctx *c, uint8_t *labels, uint8_t *held, uint32_t n_classes, const double *scale,
                                                 const double *pair_scale, const double *log_prior, const double *log_pair_prior,
                                                 const uint8_t *mask, double doublet_threshold, uint32_t max_iter, uint64_t min_loci,
                                                 cellector_refine_doublets_summary *out, double *ll, double *ll_pair, double *posterior,
                                                 double *doublet_posterior, uint8_t *best_pair, uint64_t *qual)
{
    if (!c) return CELLECTOR_EINVAL;
    CHK(doublet_call_check(c, "refine_class_doublets", labels, held, n_classes, scale, pair_scale, log_prior, log_pair_prior));
    REQUIRE(c, min_loci >= 1, "refine_class_doublets: min_loci must be at least 1");
    if (!(doublet_threshold >= 0.0 && doublet_threshold <= 1.0))
        return ctx_fail(c, CELLECTOR_EINVAL, "refine_class_doublets: doublet_threshold = %g is not within [0, 1]", doublet_threshold);
    SETDEV(c);
    const cellector_status st = class_doublets_run(c, labels, held, n_classes, scale, pair_scale, log_prior, log_pair_prior, mask,
                                                   doublet_threshold, max_iter, min_loci, labels, held, out, ll, ll_pair, posterior,
                                                   doublet_posterior, nullptr, best_pair, nullptr, qual);
    if (c->timing) timer_collect(c);
    return st;
}

// ---- genotype clusters without labels: kernels_cluster.hip ----------------------------------------------------
cellector_status cellector_cluster_default_params(cellector_cluster_params *out)
{
    if (!out) return CELLECTOR_EINVAL;
    out->theta_floor = 0.01;
    out->anneal_base = 20.0;
    out->tol = 0.01;
    out->anneal_steps = 9;
    out->max_iter = 50;
    out->min_loci = 1;
    return CELLECTOR_OK;
}

// what every cluster call checks before anything is written or launched
static cellector_status cluster_call_check(cellector_ctx *c, const char *what, double theta_floor)
{
    CHK(model_call_scope(c, what));
    if (!(theta_floor > 0.0 && theta_floor < 0.5))
        return ctx_fail(c, CELLECTOR_EINVAL, "%s: theta_floor = %g is not within (0, 0.5)", what, theta_floor);
    return CELLECTOR_OK;
}
static cellector_status cluster_columns_check(cellector_ctx *c, const char *what, uint32_t K, uint32_t R)
{
    if (K < 2 || K > 16) return ctx_fail(c, CELLECTOR_EINVAL, "%s: %u clusters, 2..16 are supported", what, K);
    if (R < 1) return ctx_fail(c, CELLECTOR_EINVAL, "%s: at least one restart is needed", what);
    if ((uint64_t)K * R > 64) return ctx_fail(c, CELLECTOR_EINVAL, "%s: %u clusters x %u restarts = %llu columns, at most 64 are supported", what, K, R,
                                              (unsigned long long)K * R);
    return CELLECTOR_OK;
}

cellector_status cellector_cluster(cellector_ctx *c, uint32_t n_clusters, uint32_t n_restarts, uint64_t seed, const cellector_cluster_params *p,
                                   const uint8_t *mask, uint8_t *labels, double *ll, double *posterior, double *theta, double *objective,
                                   cellector_cluster_summary *out)
{
    if (!c) return CELLECTOR_EINVAL;
    cellector_cluster_params prm = params_or_default(cellector_cluster_default_params, p);
    CHK(cluster_call_check(c, "cluster", prm.theta_floor));
    CHK(cluster_columns_check(c, "cluster", n_clusters, n_restarts));
    if (prm.anneal_steps < 1 || prm.anneal_steps > 16)
        return ctx_fail(c, CELLECTOR_EINVAL, "cluster: anneal_steps = %u is not within 1..16", prm.anneal_steps);
    if (!std::isfinite(prm.anneal_base) || prm.anneal_base <= 0.0)
        return ctx_fail(c, CELLECTOR_EINVAL, "cluster: anneal_base = %g is not a finite value > 0", prm.anneal_base);
    if (!std::isfinite(prm.tol) || prm.tol <= 0.0) return ctx_fail(c, CELLECTOR_EINVAL, "cluster: tol = %g is not a finite value > 0", prm.tol);
    REQUIRE(c, prm.min_loci >= 1, "cluster: min_loci must be at least 1");
    SETDEV(c);
    return cluster_run(c, n_clusters, n_restarts, seed, &prm, mask, labels, ll, posterior, theta, objective, out);
}

cellector_status cellector_cluster_m_step(cellector_ctx *c, const double *w, uint32_t J, const uint8_t *mask, double theta_floor, double *A,
                                          double *T, double *theta, double *tab)
{
    if (!c) return CELLECTOR_EINVAL;
    CHK(cluster_call_check(c, "cluster_m_step", theta_floor));
    if (J < 1 || J > 64) return ctx_fail(c, CELLECTOR_EINVAL, "cluster_m_step: %u columns, 1..64 are supported", J);
    REQUIRE(c, w != nullptr, "cluster_m_step: null w");
    for (uint64_t i = 0, n = c->nloc * J; i < n; i++)
        if (!(w[i] >= 0.0))
            return ctx_fail(c, CELLECTOR_EINVAL, "cluster_m_step: w of cell %llu, column %llu is %g: neither NaN nor a negative value is a weight",
                            (unsigned long long)(i / J), (unsigned long long)(i % J), w[i]);
    SETDEV(c);
    return cluster_m_step_run(c, w, J, mask, theta_floor, A, T, theta, tab);
}

cellector_status cellector_cluster_e_step(cellector_ctx *c, const double *tab, uint32_t K, uint32_t R, const double *temp, const uint8_t *mask,
                                          double *s, double *w, double *objective)
{
    if (!c) return CELLECTOR_EINVAL;
    CHK(cluster_call_check(c, "cluster_e_step", 0.25));
    CHK(cluster_columns_check(c, "cluster_e_step", K, R));
    REQUIRE(c, tab != nullptr, "cluster_e_step: null tab");
    for (uint64_t i = 0; temp && i < c->nloc; i++)
        if (!(temp[i] >= 1.0))
            return ctx_fail(c, CELLECTOR_EINVAL, "cluster_e_step: temp of cell %llu is %g: a temperature is a value >= 1", (unsigned long long)i, temp[i]);
    SETDEV(c);
    return cluster_e_step_run(c, tab, K, R, temp, mask, s, w, objective);
}

// ---- class genotypes: kernels_genotypes.hip and genotype_host.h ---------------------------------------------
// load_mtx_final + the rule of output_final_vcf (main.rs:52-131) for the K classes of a labelling
cellector_status cellector_class_genotypes(cellector_ctx *c, const uint8_t *labels, uint32_t n_classes, double ambient, double gt_threshold,
                                           uint64_t *cells, uint64_t *alt, uint64_t *ref, uint8_t *gt, double *gp, double *gp3)
{
    if (!c) return CELLECTOR_EINVAL;
    CHK(class_call_check(c, "class_genotypes", labels, n_classes, nullptr, nullptr));
    if (!(ambient >= 0.0 && ambient <= 1.0)) return ctx_fail(c, CELLECTOR_EINVAL, "class_genotypes: ambient = %g is not within [0, 1]", ambient);
    if (!(gt_threshold >= 0.0 && gt_threshold <= 1.0))
        return ctx_fail(c, CELLECTOR_EINVAL, "class_genotypes: gt_threshold = %g is not within [0, 1]", gt_threshold);
    REQUIRE(c, c->keep_coo && (c->coo.locus || !c->nnz), "final tallies need the staged COO (option keep_coo=1)");
    SETDEV(c);
    const uint32_t K = n_classes;
    const uint64_t TL = c->total_loci, n = c->nloc, planes = (uint64_t)(K + 1) * 2;
    // every buffer first: on CELLECTOR_ENOMEM nothing has been written
    DevBuf<uint64_t> d_acc;
    DevBuf<uint8_t> d_lab;
    CHK(dev_alloc(c, &d_acc, planes * TL));
    CHK(dev_alloc(c, &d_lab, n));
    std::vector<uint64_t> h;
    try {
        if (alt || ref || gt || gp || gp3) h.resize(planes * TL);
    } catch (const std::bad_alloc &) {
        return ctx_fail(c, CELLECTOR_ENOMEM, "class_genotypes: out of host memory");
    }
    if (n) HIPCHK(c, hipMemcpyAsync(d_lab, labels, n, hipMemcpyHostToDevice, c->stream));
    CHK(launch_genotype_tallies(c, d_lab, K, d_acc));
    const bool rule = gt || gp || gp3;
    if ((alt || ref || rule) && TL) CHK(d2h(c, h.data(), d_acc, planes * TL * 8));
    else HIPCHK(c, hipStreamSynchronize(c->stream));  // (the caller's labels have been read, the scratch may go)
    d_acc.reset();
    d_lab.reset();
    if (cells) {
        for (uint32_t k = 0; k <= K; k++) cells[k] = 0;
        for (uint64_t i = 0; i < n; i++) cells[labels[i] == 255 ? K : labels[i]]++;
    }
    for (uint32_t k = 0; k <= K && TL; k++) {
        if (alt) memcpy(alt + (uint64_t)k * TL, h.data() + (uint64_t)k * 2 * TL, TL * 8);
        if (ref) memcpy(ref + (uint64_t)k * TL, h.data() + ((uint64_t)k * 2 + 1) * TL, TL * 8);
    }
    if (!rule) return CELLECTOR_OK;
    for (uint64_t l = 0; l < TL; l++) {
        uint64_t A = 0, R = 0;
        for (uint32_t k = 0; k <= K; k++) { A += h[(uint64_t)k * 2 * TL + l]; R += h[((uint64_t)k * 2 + 1) * TL + l]; }
        const GenotypeLocus g = genotype_locus(A, R, ambient);
        for (uint32_t k = 0; k < K; k++) {
            const GenotypeCall q = genotype_call(g, h[(uint64_t)k * 2 * TL + l], h[((uint64_t)k * 2 + 1) * TL + l], gt_threshold);
            const uint64_t o = (uint64_t)k * TL + l;
            if (gt) gt[o] = q.gt;
            if (gp) gp[o] = q.gp;
            if (gp3) { gp3[3 * o] = q.q[0]; gp3[3 * o + 1] = q.q[1]; gp3[3 * o + 2] = q.q[2]; }
        }
    }
    return CELLECTOR_OK;
}
