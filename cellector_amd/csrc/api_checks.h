// Internal to the C-ABI layer (ctx_core.cpp, api_*.cpp), not part of the public ABI: the state checks every entry point shares, the
// scope check of the whole-matrix model calls, and the argument checks that more than one file uses.
#pragma once
#include <cmath>

#include "ctx.h"
#include "multi.h"

#define READY(c) REQUIRE(c, (c) && (c)->state == cellector_ctx::ST_READY, "no matrix loaded")
// per-locus state is replicated on every shard: shard 0 of a multi-device ctx answers
#define SHARD0(c, call)                                                      \
    do {                                                                     \
        if ((c)->multi) {                                                    \
            const cellector_ctx *s0__ = multi_shard0(c);                     \
            const cellector_status st__ = (call);                            \
            if (st__ != CELLECTOR_OK) (c)->err = s0__->err;                  \
            return st__;                                                     \
        }                                                                    \
    } while (0)

// The scope of every whole-matrix model call.  They sum count planes over all cells: one device holding every cell.  (Summing the
// planes across shards needs an exchange the public LOCUS buffer has no room for.)
static inline cellector_status whole_matrix_scope(const cellector_ctx *c, const char *what)
{
    if (c->multi) return ctx_fail(c, CELLECTOR_EINVAL, "%s works on a single-device ctx: the shards' count planes are not exchanged", what);
    if (comm_active(c->comm))
        return ctx_fail(c, CELLECTOR_EINVAL, "%s works on a ctx without a communicator: the shards' count planes are not exchanged", what);
    if (c->state == cellector_ctx::ST_READY ? c->nloc != c->total_cells : c->req_cell_begin != 0)
        return ctx_fail(c, CELLECTOR_EINVAL, "%s works on a ctx that holds all cells, not on a cellector_set_shard range: the shards' "
                                             "count planes are not exchanged", what);
    if (c->state == cellector_ctx::ST_READY && c->nnz >= (1ull << 32))  // (kernels_locus_moments.hip refuses the same: no counter may wrap)
        return ctx_fail(c, CELLECTOR_EINVAL, "%s: %llu entries, the locus histograms count in 32 bits (below 2^32 entries)", what,
                        (unsigned long long)c->nnz);
    return CELLECTOR_OK;
}

// The three steps every whole-matrix model call opens with.  The first failing one decides the message a caller sees.
static inline cellector_status model_call_scope(const cellector_ctx *c, const char *what)
{
    CHK(whole_matrix_scope(c, what));
    READY(c);
    if (c->em_phase != 0) return ctx_fail(c, CELLECTOR_EINVAL, "%s: iteration in flight (finish it with cellector_em_finish)", what);
    return CELLECTOR_OK;
}

// the defaults, overridden by the caller's struct if given
template <class P>
static inline P params_or_default(cellector_status (*defaults)(P *), const P *p)
{
    P prm;
    return p ? *p : (defaults(&prm), prm);
}

// what every class call checks before anything is written or launched
static inline cellector_status class_call_check(cellector_ctx *c, const char *what, const uint8_t *labels, uint32_t K, const double *scale,
                                                const double *log_prior)
{
    CHK(model_call_scope(c, what));
    if (!labels) return ctx_fail(c, CELLECTOR_EINVAL, "%s: null labels", what);
    if (K < 1 || K > 16) return ctx_fail(c, CELLECTOR_EINVAL, "%s: %u classes, 1..16 are supported", what, K);
    bool any = false;
    for (uint64_t i = 0; i < c->nloc; i++) {
        if (labels[i] >= K && labels[i] != 255)
            return ctx_fail(c, CELLECTOR_EINVAL, "%s: cell %llu has label %u, neither below the %u classes nor 255 (unlabelled)", what,
                            (unsigned long long)i, (unsigned)labels[i], K);
        any = any || labels[i] != 255;
    }
    if (!any) return ctx_fail(c, CELLECTOR_EINVAL, "%s: every cell is unlabelled: all %u classes are dead", what, K);
    for (uint32_t k = 0; scale && k < K; k++)
        if (!std::isfinite(scale[k]) || scale[k] < 0.0)
            return ctx_fail(c, CELLECTOR_EINVAL, "%s: scale[%u] = %g is not a finite value >= 0", what, k, scale[k]);
    for (uint32_t k = 0; log_prior && k < K; k++)
        if (std::isnan(log_prior[k])) return ctx_fail(c, CELLECTOR_EINVAL, "%s: log_prior[%u] is NaN", what, k);
    return CELLECTOR_OK;
}

// what every donor call checks before anything is written or launched (the scope first: class_call_check's own for the match):
// how many donors and is their array there (calls: gt, or the gp of a soft call; null_name: what the message calls it) ...
static inline cellector_status donor_count_check(cellector_ctx *c, const char *what, const void *calls, const char *null_name, uint32_t D)
{
    if (D < 1 || D > 64) return ctx_fail(c, CELLECTOR_EINVAL, "%s: %u donors, 1..64 are supported", what, D);
    if (!calls) return ctx_fail(c, CELLECTOR_EINVAL, "%s: null %s", what, null_name);
    return CELLECTOR_OK;
}
// ... and are the parameters in range (all the tables, which depend on no donor, check)
static inline cellector_status donor_params_check(cellector_ctx *c, const char *what, const cellector_donor_params *p)
{
    if (!(p->err > 0.0 && p->err < 0.5)) return ctx_fail(c, CELLECTOR_EINVAL, "%s: err = %g is not within (0, 0.5)", what, p->err);
    if (!(p->ambient >= 0.0 && p->ambient < 1.0)) return ctx_fail(c, CELLECTOR_EINVAL, "%s: ambient = %g is not within [0, 1)", what, p->ambient);
    if (!(p->doublet_rate >= 0.0 && p->doublet_rate < 1.0))
        return ctx_fail(c, CELLECTOR_EINVAL, "%s: doublet_rate = %g is not within [0, 1)", what, p->doublet_rate);
    if (!(p->posterior_threshold >= 0.0 && p->posterior_threshold <= 1.0))
        return ctx_fail(c, CELLECTOR_EINVAL, "%s: posterior_threshold = %g is not within [0, 1]", what, p->posterior_threshold);
    if (p->min_loci < 1) return ctx_fail(c, CELLECTOR_EINVAL, "%s: min_loci must be at least 1", what);
    return CELLECTOR_OK;
}
