// The ingests of the C ABI: mtx, coo and synthetic (kernels_parse.hip, kernels_synth.hip), joined (kernels_join.hip), the multi-device
// text ingest's two steps, cellector_ingest_finish (kernels_ingest.hip, kernels_tiled_build.hip); the accessors; the exchange buffers.
#include <cmath>
#include <cstdio>
#include <algorithm>
#include <vector>

#include "api_checks.h"

// ---- ingest -------------------------------------------------------------------------------------------
static cellector_status begin_ingest(cellector_ctx *c, uint64_t total_loci, uint64_t total_cells)
{
    SETDEV(c);
    drop_matrix(c);  // (an ingest from outside: cellector_cell_origin is the identity again, cellector_cell_source all 0)
    // a caller-bound PASS1 buffer serves every matrix, with its whole capacity (n_pass1 is what the last one used of it)
    if (c->pass1_bound) { c->x_pass1 = c->pass1_bound; c->n_pass1 = c->pass1_bound_cap; }
    REQUIRE(c, total_loci <= 0xffffffffull && total_cells <= 0xffffffffull, "dims exceed 32-bit indices");
    c->total_loci = total_loci;
    c->total_cells = total_cells;
    if (c->ingest_all_cells) {
        c->cell_begin = 0;
        c->cell_end = total_cells;
    } else if (comm_active(c->comm)) {  // rank r owns the r-th contiguous range: equal ranges, or the partition it was given
        if (c->comm.has_bounds && c->comm.bounds[c->comm.n] != total_cells)
            return ctx_fail(c, CELLECTOR_EINVAL, "the partition covers %llu cells, the matrix has %llu",
                            (unsigned long long)c->comm.bounds[c->comm.n], (unsigned long long)total_cells);
        comm_range(c->comm, total_cells, c->comm.rank, &c->cell_begin, &c->cell_end);
    } else {
        c->cell_begin = c->req_cell_begin;
        c->cell_end = c->req_cell_end;
    }
    if (c->cell_end > total_cells) c->cell_end = total_cells;
    if (c->cell_begin > c->cell_end) c->cell_begin = c->cell_end;
    c->nloc = c->cell_end - c->cell_begin;
    const uint64_t need = (uint64_t)P1_PLANES * total_loci;
    if (c->x_pass1) {
        REQUIRE(c, c->n_pass1 >= need, "bound PASS1 exchange buffer too small");
    } else {
        CHK(dev_alloc(c, &c->x_pass1_own, need));
        c->x_pass1 = c->x_pass1_own;
    }
    c->n_pass1 = need;
    return CELLECTOR_OK;
}

cellector_status cellector_ingest_coo(cellector_ctx *c, uint64_t total_loci, uint64_t total_cells, uint64_t nnz,
                                      const uint32_t *locus0, const uint32_t *cell0, const uint32_t *alt,
                                      const uint32_t *ref)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return multi_ingest_coo(c, total_loci, total_cells, nnz, locus0, cell0, alt, ref);
    REQUIRE(c, nnz == 0 || (locus0 && cell0 && alt && ref), "null COO array");
    CHK(begin_ingest(c, total_loci, total_cells));
    CHK(ingest_stage_host_coo(c, nnz, locus0, cell0, alt, ref));
    CHK(ingest_pass1(c));
    c->state = cellector_ctx::ST_STAGED;
    return CELLECTOR_OK;
}

cellector_status cellector_ingest_mtx(cellector_ctx *c, const char *alt_path, const char *ref_path)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return multi_ingest_mtx(c, alt_path, ref_path);
    REQUIRE(c, alt_path && ref_path, "null path");
    const bool timing = getenv("CELLECTOR_TIMING") != nullptr && c->comm.rank == 0;
    LapTimer t;
    MtxInput *in = nullptr;
    uint64_t tl = 0, tc = 0;
    CHK(ctx_mtx_open(c, alt_path, ref_path, &in, &tl, &tc, true));
    if (timing) fprintf(stderr, "[timing]   open / inflate          %8.3f s\n", t.lap());
    cellector_status s = begin_ingest(c, tl, tc);
    if (s == CELLECTOR_OK) s = ingest_stage_mtx_device(c, in);  // tokenised and converted on the GPU
    mtx_input_close(in);
    CHK(s);
    if (timing) fprintf(stderr, "[timing]   upload + device parse   %8.3f s\n", t.lap());
    CHK(ingest_pass1(c));
    c->state = cellector_ctx::ST_STAGED;
    return CELLECTOR_OK;
}

// ---- the joined ingests: two count streams keyed by (locus, cell) (kernels_join.hip) ------------------------------------------------
// why a ctx cannot take a joined ingest, or null: the scope of cellector_restage, before anything is staged
static const char *join_scope(const cellector_ctx *c, uint64_t total_cells)
{
    if (c->multi) return "is a multi-device ctx: its staged entries are sharded";
    if (comm_active(c->comm)) return "has a communicator: every rank stages its own cells";
    if (c->req_cell_begin != 0 || c->req_cell_end < total_cells) return "holds a cellector_set_shard range, not all cells";
    return nullptr;
}
static cellector_status join_mode_check(const cellector_ctx *c, int mode)
{
    if (mode != CELLECTOR_JOIN_REF && mode != CELLECTOR_JOIN_DEPTH)
        return ctx_fail(c, CELLECTOR_EINVAL, "join: mode must be CELLECTOR_JOIN_REF (1) or CELLECTOR_JOIN_DEPTH (2)");
    return CELLECTOR_OK;
}
// tokens -> staged COO -> PASS1; the ctx has been through begin_ingest
static cellector_status join_finish_stage(cellector_ctx *c, JoinTokens *first, JoinTokens *second, uint32_t index_base, int mode,
                                          cellector_join_summary *out, JoinPhases *ph)
{
    StagedCoo coo;
    CHK(join_stage(c, first, second, index_base, mode, &coo, out, ph));
    c->coo = std::move(coo);
    CHK(ingest_pass1(c));
    c->state = cellector_ctx::ST_STAGED;
    if (getenv("CELLECTOR_TIMING"))
        fprintf(stderr, "[timing]   join: tokens FIRST %.4f s, tokens SECOND %.4f s, checks %.4f s, sorts %.4f s, join %.4f s (its kernels %.3f ms)\n",
                ph->tokens_first, ph->tokens_second, ph->checks, ph->sorts, ph->join, ph->join_kernels_ms);
    return CELLECTOR_OK;
}

cellector_status cellector_ingest_mtx_joined(cellector_ctx *c, const char *first_path, const char *second_path, int mode,
                                             cellector_join_summary *out)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return ctx_fail(c, CELLECTOR_EINVAL, "ingest_mtx_joined: ctx %s", join_scope(c, 0));
    REQUIRE(c, first_path && second_path, "null path");
    CHK(join_mode_check(c, mode));
    MtxInput *in = nullptr;
    uint64_t tl = 0, tc = 0, first_hint = 0;
    CHK(ctx_mtx_open(c, first_path, second_path, &in, &tl, &tc, true));
    struct Closer { MtxInput *in; ~Closer() { mtx_input_close(in); } } closer{in};
    CHK(join_size_lines(c, in, &first_hint));
    if (const char *why = join_scope(c, tc)) return ctx_fail(c, CELLECTOR_EINVAL, "ingest_mtx_joined: ctx %s", why);
    // ---- validated: from here the ctx changes as in cellector_ingest_mtx
    CHK(begin_ingest(c, tl, tc));
    JoinTokens first, second;
    JoinPhases ph;
    CHK(join_parse_pair(c, in, first_hint, &first, &second, &ph));
    return join_finish_stage(c, &first, &second, 1u, mode, out, &ph);
}

cellector_status cellector_ingest_coo_joined(cellector_ctx *c, uint64_t total_loci, uint64_t total_cells, uint64_t n_first,
                                             const uint32_t *locus0_a, const uint32_t *cell0_a, const uint32_t *count_a, uint64_t n_second,
                                             const uint32_t *locus0_b, const uint32_t *cell0_b, const uint32_t *count_b, int mode,
                                             cellector_join_summary *out)
{
    if (!c) return CELLECTOR_EINVAL;
    if (const char *why = join_scope(c, total_cells)) return ctx_fail(c, CELLECTOR_EINVAL, "ingest_coo_joined: ctx %s", why);
    REQUIRE(c, n_first == 0 || (locus0_a && cell0_a && count_a), "null COO array");
    REQUIRE(c, n_second == 0 || (locus0_b && cell0_b && count_b), "null COO array");
    CHK(join_mode_check(c, mode));
    CHK(begin_ingest(c, total_loci, total_cells));
    JoinTokens side[2];
    JoinPhases ph;
    LapTimer t;
    const uint64_t n[2] = {n_first, n_second};
    const uint32_t *src[2][3] = {{locus0_a, cell0_a, count_a}, {locus0_b, cell0_b, count_b}};
    for (int s = 0; s < 2; s++) {
        DevBuf<uint32_t> *dst[3] = {&side[s].locus, &side[s].cell, &side[s].count};
        side[s].n = n[s];
        for (int k = 0; k < 3; k++) {
            CHK(dev_alloc(c, dst[k], n[s]));
            if (n[s]) HIPCHK(c, hipMemcpyAsync(dst[k]->get(), src[s][k], n[s] * 4, hipMemcpyHostToDevice, c->stream));
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
        (s ? ph.tokens_second : ph.tokens_first) = t.lap();
    }
    return join_finish_stage(c, &side[0], &side[1], 0u, mode, out, &ph);
}

cellector_status cellector_load_mtx_joined(cellector_ctx *c, const char *first_path, const char *second_path, int mode, uint64_t min_alt,
                                           uint64_t min_ref, cellector_join_summary *out)
{
    CHK(cellector_ingest_mtx_joined(c, first_path, second_path, mode, out));
    return cellector_ingest_finish(c, min_alt, min_ref);
}

// Multi-device text ingest, step 1: shard `c` tokenises the whole pair and stages the entries of ALL cells (global cell index).
cellector_status ffi_stage_mtx_all_cells(cellector_ctx *c, const char *alt_path, const char *ref_path, cellector_ctx *helper)
{
    REQUIRE(c, alt_path && ref_path, "null path");
    MtxInput *in = nullptr;
    uint64_t tl = 0, tc = 0;
    CHK(ctx_mtx_open(c, alt_path, ref_path, &in, &tl, &tc));
    c->ingest_all_cells = true;
    cellector_status s = begin_ingest(c, tl, tc);
    if (s == CELLECTOR_OK) s = ingest_stage_mtx_device(c, in, helper);
    c->ingest_all_cells = false;
    mtx_input_close(in);
    return s;
}
// ... step 2: a shard takes over its routed entries (arrays on its own device, cell index local, file order) as its staged COO.
cellector_status ffi_adopt_staged(cellector_ctx *c, uint64_t total_loci, uint64_t total_cells, StagedCoo &&coo)
{
    CHK(begin_ingest(c, total_loci, total_cells));
    c->coo = std::move(coo);
    CHK(ingest_pass1(c));
    c->state = cellector_ctx::ST_STAGED;
    return CELLECTOR_OK;
}

cellector_status cellector_ingest_synthetic(cellector_ctx *c, uint64_t total_loci, uint64_t total_cells,
                                            double density, uint64_t seed, double minority_fraction,
                                            double doublet_fraction)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return multi_ingest_synthetic(c, total_loci, total_cells, density, seed, minority_fraction, doublet_fraction);
    CHK(begin_ingest(c, total_loci, total_cells));
    CHK(synth_generate(c, density, seed, minority_fraction, doublet_fraction));
    CHK(ingest_pass1(c));
    c->state = cellector_ctx::ST_STAGED;
    return CELLECTOR_OK;
}

cellector_status cellector_write_staged_mtx(cellector_ctx *c, const char *alt_path, const char *ref_path)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return ctx_fail(c, CELLECTOR_EINVAL, "write_staged_mtx works on a single-device ctx (the staged entries of a multi-device ctx are sharded)");
    REQUIRE(c, alt_path && ref_path, "null path");
    REQUIRE(c, c->state != cellector_ctx::ST_EMPTY, "write_staged_mtx without a staged matrix");
    SETDEV(c);
    return synth_write_mtx(c, alt_path, ref_path);
}

cellector_status cellector_ingest_finish(cellector_ctx *c, uint64_t min_alt, uint64_t min_ref)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return multi_ingest_finish(c, min_alt, min_ref);
    REQUIRE(c, c->state == cellector_ctx::ST_STAGED, "ingest_finish without a staged matrix");
    SETDEV(c);
    const bool timing = getenv("CELLECTOR_TIMING") != nullptr && c->comm.rank == 0;
    LapTimer t;
    if (comm_active(c->comm)) {  // exchange point 1: global pass-1 counts and allele totals (every shard applies the same locus filter)
        CHK((cellector_status)comm_allreduce_sum(c, c->x_pass1, (uint64_t)P1_PLANES * c->total_loci));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    CHK(ingest_build(c, min_alt, min_ref));
    if (timing) fprintf(stderr, "[timing]   CSC / CSR build         %8.3f s\n", t.lap());
    const uint64_t L = c->L, n = c->nloc;
    CHK(dev_alloc(c, &c->ab, L)); CHK(dev_alloc(c, &c->ab6, 8 * L));
    CHK(dev_alloc(c, &c->mask, L)); CHK(dev_alloc(c, &c->mask_next, L));
    CHK(dev_alloc(c, &c->flags, n)); CHK(dev_alloc(c, &c->flags_new, n));
    CHK(dev_alloc(c, &c->ll, n)); CHK(dev_alloc(c, &c->ell, n)); CHK(dev_alloc(c, &c->nloci, n));
    CHK(dev_alloc(c, &c->post, 4 * n));
    // (with a communicator every rank owns an equal slot of NORM: the in-place all-gather's layout)
    const uint64_t need_norm = comm_active(c->comm) ? comm_cells_per_rank(c->total_cells, c->comm.n) * (uint64_t)c->comm.n : c->total_cells;
    const uint64_t need_locus = (uint64_t)LB_PLANES * L + LC_COUNTERS;
    if (c->x_norm) REQUIRE(c, c->n_norm >= need_norm, "bound NORM exchange buffer too small");
    else { CHK(dev_alloc(c, &c->x_norm_own, need_norm)); c->x_norm = c->x_norm_own; }
    if (c->x_locus) REQUIRE(c, c->n_locus >= need_locus, "bound LOCUS exchange buffer too small");
    else { CHK(dev_alloc(c, &c->x_locus_own, need_locus)); c->x_locus = c->x_locus_own; }
    c->n_norm = need_norm;
    c->n_locus = need_locus;
    CHK(em_state_clear(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    {
        // The near-tie band of cellector_iter_summary.n_near_threshold follows the matrix' depth: the reference's ln_gamma
        // differences (stats.rs:41-53) carry ~eps * lnGamma(alpha + beta) of cancellation error per term, which the device's
        // product form does not reproduce — 1e-11 on a normalised LL at alpha + beta ~ 1e4 (vartrix-like depth), 1e-8 at 1e6.
        // band = max(1e-9, 8 eps lnGamma(max over the used loci of S_alt + S_ref + 2)), relative to max(1, |threshold|);
        // the global totals are the same on every shard.
        std::vector<double> sa(L), sr(L);
        if (L) {
            HIPCHK(c, hipMemcpy(sa.data(), c->s_alt, L * 8, hipMemcpyDeviceToHost));
            HIPCHK(c, hipMemcpy(sr.data(), c->s_ref, L * 8, hipMemcpyDeviceToHost));
        }
        double max_ab = 2.0;
        for (uint64_t l = 0; l < L; l++) max_ab = std::max(max_ab, sa[l] + sr[l] + 2.0);
        c->near_rel = std::max(CELLECTOR_NEAR_TIE_REL, 8.0 * 2.220446049250313e-16 * lgamma(max_ab));
    }
    if (c->engine == 2) {
        CHK(tiled_build(c));
        // the packed by-locus CSC (8 B per entry: 16 GB at 2e9 entries) is only streamed by engine 1; engine 2 has built
        // its compact CSC and overflow CSC from it.  Engine 1 must therefore be chosen BEFORE the ingest.
        c->csc_ent.reset();
    }
    if (timing) fprintf(stderr, "[timing]   tiled layouts           %8.3f s\n", t.lap());
    dev_cache_trim(c->device);  // the ingest's big temporaries are done: hand this device's cached blocks back
    c->state = cellector_ctx::ST_READY;
    c->em_phase = 0; c->iteration = 0; c->have_iter = false; c->n_excluded_global = 0;
    return CELLECTOR_OK;
}

cellector_status cellector_load_mtx(cellector_ctx *c, const char *a, const char *r, uint64_t min_alt, uint64_t min_ref)
{
    CHK(cellector_ingest_mtx(c, a, r));
    return cellector_ingest_finish(c, min_alt, min_ref);
}

cellector_status cellector_load_coo(cellector_ctx *c, uint64_t tl, uint64_t tc, uint64_t nnz, const uint32_t *l,
                                    const uint32_t *ce, const uint32_t *a, const uint32_t *r, uint64_t min_alt,
                                    uint64_t min_ref)
{
    CHK(cellector_ingest_coo(c, tl, tc, nnz, l, ce, a, r));
    return cellector_ingest_finish(c, min_alt, min_ref);
}

// ---- accessors ----------------------------------------------------------------------------------------
cellector_status cellector_dims(const cellector_ctx *c, cellector_dims_t *o)
{
    if (!c || !o) return CELLECTOR_EINVAL;
    if (c->multi) return multi_dims(c, o);
    o->total_cells = c->total_cells; o->total_loci = c->total_loci; o->loci_used = c->L;
    o->cell_begin = c->cell_begin; o->cell_end = c->cell_end; o->nnz_used = c->nnz;
    return CELLECTOR_OK;
}

cellector_status cellector_locus_ids(const cellector_ctx *c, uint64_t *out)
{
    if (!c) return CELLECTOR_EINVAL;
    SHARD0(c, cellector_locus_ids(s0__, out));
    READY(c);
    return d2h(c, out, c->locus_ids, c->L * 8);
}

cellector_status cellector_locus_counts(const cellector_ctx *c, double *out)
{
    if (!c) return CELLECTOR_EINVAL;
    SHARD0(c, cellector_locus_counts(s0__, out));
    READY(c);
    std::vector<double> a(c->L), r(c->L);
    CHK(d2h(c, a.data(), c->s_alt, c->L * 8));
    CHK(d2h(c, r.data(), c->s_ref, c->L * 8));
    for (uint64_t l = 0; l < c->L; l++) { out[2 * l] = r[l]; out[2 * l + 1] = a[l]; }
    return CELLECTOR_OK;
}

cellector_status cellector_entries_per_cell(const cellector_ctx *c, uint32_t *out)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return multi_entries_per_cell(c, out);
    READY(c);
    std::vector<uint64_t> p(c->nloc + 1);
    CHK(d2h(c, p.data(), c->csr_ptr, (c->nloc + 1) * 8));
    for (uint64_t i = 0; i < c->nloc; i++) out[i] = (uint32_t)(p[i + 1] - p[i]);
    return CELLECTOR_OK;
}

cellector_status cellector_csr_rows(const cellector_ctx *c, uint64_t rb, uint64_t re, uint64_t *row_ptr,
                                    uint64_t *entries, uint64_t capacity)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return multi_csr_rows(c, rb, re, row_ptr, entries, capacity);
    READY(c);
    REQUIRE(c, rb <= re && re <= c->nloc && row_ptr, "bad row range");
    CHK(d2h(c, row_ptr, c->csr_ptr + rb, (re - rb + 1) * 8));
    const uint64_t base = row_ptr[0], cnt = row_ptr[re - rb] - base;
    for (uint64_t i = 0; i <= re - rb; i++) row_ptr[i] -= base;
    if (entries) {
        REQUIRE(c, capacity >= cnt, "entries capacity too small");
        CHK(d2h(c, entries, c->csr_ent + base, cnt * 8));
    }
    return CELLECTOR_OK;
}

// ---- exchange buffers ---------------------------------------------------------------------------------
cellector_status cellector_exchange_buffer(cellector_ctx *c, cellector_xchg which, void **dev_ptr, uint64_t *n)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return ctx_fail(c, CELLECTOR_EINVAL, "the exchange buffers of a multi-device ctx are internal");
    double *p = nullptr;
    uint64_t cnt = 0;
    switch (which) {
    case CELLECTOR_XCHG_PASS1: p = c->x_pass1; cnt = c->n_pass1; break;
    case CELLECTOR_XCHG_NORM:
        p = c->x_norm; cnt = c->state == cellector_ctx::ST_READY ? c->total_cells : c->n_norm; break;
    case CELLECTOR_XCHG_LOCUS:
        p = c->x_locus;
        cnt = c->state == cellector_ctx::ST_READY ? (uint64_t)LB_PLANES * c->L + LC_COUNTERS : c->n_locus; break;
    default: return ctx_fail(c, CELLECTOR_EINVAL, "unknown exchange buffer");
    }
    if (dev_ptr) *dev_ptr = p;
    if (n) *n = cnt;
    return CELLECTOR_OK;
}

cellector_status cellector_bind_exchange_buffer(cellector_ctx *c, cellector_xchg which, void *dev_ptr, uint64_t n)
{
    if (!c || !dev_ptr) return CELLECTOR_EINVAL;
    if (c->multi || comm_active(c->comm)) return ctx_fail(c, CELLECTOR_EINVAL, "a ctx with a communicator owns its exchange buffers");
    double *p = (double *)dev_ptr;
    c->tables_prebuilt = false;  // (tables built ahead read the old buffers)
    switch (which) {
    case CELLECTOR_XCHG_PASS1:
        REQUIRE(c, c->state == cellector_ctx::ST_EMPTY, "bind PASS1 before ingest");
        c->x_pass1_own.reset();
        c->x_pass1 = c->pass1_bound = p; c->n_pass1 = c->pass1_bound_cap = n;
        break;
    case CELLECTOR_XCHG_NORM:
        REQUIRE(c, c->state != cellector_ctx::ST_READY || n >= c->total_cells, "NORM buffer too small");
        c->x_norm_own.reset();
        c->x_norm = p; c->n_norm = n;
        break;
    case CELLECTOR_XCHG_LOCUS:
        REQUIRE(c, c->state != cellector_ctx::ST_READY || n >= (uint64_t)LB_PLANES * c->L + LC_COUNTERS,
                "LOCUS buffer too small");
        if (c->state == cellector_ctx::ST_READY) {
            // carry the current tallies over (they seed the next alpha/beta update)
            HIPCHK(c, hipMemcpyAsync(p, c->x_locus, ((uint64_t)LB_PLANES * c->L + LC_COUNTERS) * 8,
                                     hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        c->x_locus_own.reset();
        c->x_locus = p; c->n_locus = n;
        break;
    default: return ctx_fail(c, CELLECTOR_EINVAL, "unknown exchange buffer");
    }
    return CELLECTOR_OK;
}
