// The EM loop of the C ABI: the em_* calls (kernels_em.hip, kernels_select.hip, kernels_resolve.hip, kernels_tiled.hip), placing its
// state (kernels_state.hip), the iter_* readers, and the calls on a caller's alpha / beta: cell_log_likelihoods, cell_pmfs
// (kernels_pmfs.hip), the variances (kernels_variance.hip), the locus moments (kernels_locus_moments.hip); order_statistics.
#include <cstring>
#include <algorithm>
#include <chrono>
#include <vector>

#include "api_checks.h"

// ---- EM iteration -------------------------------------------------------------------------------------
cellector_status cellector_em_begin(cellector_ctx *c)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return ctx_fail(c, CELLECTOR_EINVAL, "a multi-device ctx runs whole iterations: cellector_em_iteration");
    READY(c);
    REQUIRE(c, c->em_phase == 0, "em_begin: previous iteration not finished");
    SETDEV(c);
    c->filter_fused = false;  // (set by this iteration's locus pass; one left by an iteration that failed before em_finish is stale)
    // engine 2 forms alpha/beta inside its first kernel (k_build_tables); an empty shard has no cell pass at all
    if (c->engine != 2 || c->prebuilt_expected != c->compute_expected) c->tables_prebuilt = false;
    if (c->engine != 2 || c->nloc == 0) CHK(launch_alpha_beta(c));
    if (c->nloc != c->total_cells && c->norm_zero && !comm_active(c->comm))  // other shards' slices must be zero before a SUM exchange
        HIPCHK(c, hipMemsetAsync(c->x_norm, 0, c->total_cells * 8, c->stream));
    cellector_status st = c->engine == 2 ? tiled_cell_pass(c, c->ab, c->x_norm + c->cell_begin, true)
                                         : launch_cell_ll(c, c->ab, c->x_norm + c->cell_begin);
    c->work_zeroed = false;  // (only this iteration's first tile pass may rely on k_alpha_beta's reset)
    CHK(st);
    // options cell_variance / normalization: expected_log_variances under this iteration's alpha/beta, and the z-scores over
    // this shard's slice of NORM (main.rs:317-318)
    c->iter_var = c->cell_variance || c->normalization != 0;
    if (c->iter_var) CHK(launch_cell_variance(c, c->normalization != 0, c->x_norm + c->cell_begin));
    c->em_phase = 1;
    return CELLECTOR_OK;
}

cellector_status cellector_em_threshold(cellector_ctx *c, double iqr_multiple)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return ctx_fail(c, CELLECTOR_EINVAL, "a multi-device ctx runs whole iterations: cellector_em_iteration");
    READY(c);
    REQUIRE(c, c->em_phase == 1, "em_threshold without em_begin");
    if (c->locus_moments) CHK(whole_matrix_scope(c, "locus_moments 1"));  // (before anything of this phase is queued)
    SETDEV(c);
    const uint64_t n = c->total_cells;
    REQUIRE(c, n > 0, "no cells");
    // exact median / R-8 quartiles / threshold, all on the device (no host round trip in this phase).
    // Exchange point 2: a ctx with a communicator runs the radix select over the shards' keys where they are and exchanges
    // digit histograms (six all-reduces of 48 KB); option sharded_select = 0 gathers every shard's slice of the normalised
    // LLs instead and selects over all of them on every shard.  (A host that runs the exchanges itself gathers NORM before
    // this call.)
    if (comm_active(c->comm) && comm_sharded_select(c->comm, c->sharded_select, n)) {
        CHK(select_threshold_sharded(c, c->x_norm + c->cell_begin, c->nloc, n, iqr_multiple));
    } else {
        if (comm_active(c->comm)) CHK((cellector_status)comm_allgather_cells(c, c->x_norm, n));
        CHK(select_threshold(c, c->x_norm, n, iqr_multiple));
    }
    c->res_last_mode = 0;
    if (c->resolve_ties) {  // the cells next to the order statistics and the threshold with the reference's arithmetic
        REQUIRE(c, !comm_active(c->comm), "resolve_ties works on a single-device ctx");
        CHK(resolve_ties(c, iqr_multiple));
        c->res_last_mode = c->resolve_ties;
    }
    // (the counters k_flag adds to were reset by this iteration's k_alpha_beta)
    CHK(launch_flag(c, c->sel_out + 10));
    if (c->engine == 2) CHK(tiled_locus_pass(c));
    else CHK(launch_locus_stats(c));
    // option locus_moments: the expected contribution and variance per locus under this iteration's alpha/beta and mask and the
    // new exclusion set.  Here c->ab still is the cell pass' (em_finish queues the next iteration's table kernel, which rewrites
    // it) and flags_new the new set (em_finish swaps it in).
    c->iter_lm = c->locus_moments;
    if (c->iter_lm) CHK(launch_locus_moments(c));
    c->em_phase = 2;
    return CELLECTOR_OK;
}

cellector_status cellector_em_finish(cellector_ctx *c, cellector_iter_summary *out)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return ctx_fail(c, CELLECTOR_EINVAL, "a multi-device ctx runs whole iterations: cellector_em_iteration");
    READY(c);
    REQUIRE(c, c->em_phase == 2, "em_finish without em_threshold");
    SETDEV(c);
    // exchange point 3: per-locus minority tallies, contribution sums and the change counters
    if (comm_active(c->comm)) CHK((cellector_status)comm_allreduce_sum(c, c->x_locus, (uint64_t)LB_PLANES * c->L + LC_COUNTERS));
    if (c->filter_fused) c->filter_fused = false;  // (engine 2, unsharded: k_locus_finalize applied the filter)
    else CHK(launch_locus_filter(c));
    CHK(launch_iter_summary(c));
    // the next iteration's first kernel is queued behind the summary: it runs while the host waits for the summary, wakes
    // up and decides (should the loop end here, the tables it built are simply never used)
    if (c->engine == 2 && c->tiled_ready) CHK(tiled_prebuild_tables(c));
    // the fallback of the poll below: the event that rides on the table kernel's dispatch, else one recorded behind the summary
    hipEvent_t ev_wait = c->tab_event_valid ? c->ev_tab : c->ev_sum;
    if (!c->tab_event_valid) HIPCHK(c, hipEventRecord(c->ev_sum, c->stream));

    // The iteration's only host synchronisation.  The summary kernel stores its sequence number behind the values in
    // pinned memory: polling that wakes the host a few tens of microseconds before hipEventSynchronize returns, and the
    // next iteration's tile kernel is the next thing the GPU waits for.  (The event stays the fallback: it is polled too,
    // and waited for once the summary is 20 ms late.)
    {
        const double want = (double)c->sum_seq;
        const uint64_t *seq = reinterpret_cast<const uint64_t *>(c->h_sel + CELLECTOR_SUM_SEQ);
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t spin = 1;; spin++) {
            const uint64_t bits = __atomic_load_n(seq, __ATOMIC_ACQUIRE);
            double have;
            memcpy(&have, &bits, sizeof have);
            if (have == want) break;
            if ((spin & 0xfffu) == 0) {
                if (hipEventQuery(ev_wait) == hipSuccess) break;
                if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) {
                    HIPCHK(c, hipEventSynchronize(ev_wait));
                    break;
                }
            }
            __builtin_ia32_pause();
        }
    }
    double cnt[LC_COUNTERS];
    uint32_t dc[8] = {0};
    for (int i = 0; i < LC_COUNTERS; i++) cnt[i] = c->h_sel[i];
    dc[0] = (uint32_t)c->h_sel[LC_COUNTERS];
    c->last_median = c->h_sel[LC_COUNTERS + 1]; c->last_iqr = c->h_sel[LC_COUNTERS + 2]; c->last_thr = c->h_sel[LC_COUNTERS + 3];
    if (dc[0]) {
        c->n_masked_loci += dc[0];
        if (c->tiled_ready) CHK(tiled_masked_update(c));
    }
    std::swap(c->flags, c->flags_new);   // excluded_cells <- new_excluded (main.rs:43)
    std::swap(c->mask, c->mask_next);    // loci_used for the next iteration; mask_next keeps this iteration's
    // engine 2's locus pass left the counts of the new set in tally / cnt2: they are the current set's now
    if (c->engine == 2 && c->tiled_ready) c->tally_valid = true;
    c->n_excluded_global = (uint64_t)cnt[LC_N_EXCLUDED];
    c->iteration++;
    c->have_iter = true;
    c->var_formed = c->iter_var;
    c->lm_formed = c->iter_lm;
    c->em_phase = 0;
    // (timers are read out when asked for — cellector_kernel_time — not here: waiting for the last event pair and destroying
    //  the events is host time on the path to the next iteration's first launch; a long run is drained now and then)
    if (c->timing && c->timers[CELLECTOR_K_TILE_LL].start.size() + c->timers[CELLECTOR_K_CELL_LL].start.size() > 512) timer_collect(c);
    if (out) {
        out->n_new_excluded = (uint64_t)cnt[LC_N_NEW];
        out->n_rescued = (uint64_t)cnt[LC_N_RESCUED];
        out->n_excluded = c->n_excluded_global;
        out->any_change = (out->n_new_excluded > 0 || out->n_rescued > 0) ? 1 : 0;  // main.rs:335
        out->n_loci_filtered = dc[0];
        out->n_near_threshold = (uint64_t)cnt[LC_N_NEAR];
        out->median = c->last_median; out->iqr = c->last_iqr; out->threshold = c->last_thr;
    }
    return CELLECTOR_OK;
}

cellector_status cellector_em_iteration(cellector_ctx *c, double iqr_multiple, cellector_iter_summary *out)
{
    if (c && c->multi) return multi_em_iteration(c, iqr_multiple, out);
    CHK(cellector_em_begin(c));
    CHK(cellector_em_threshold(c, iqr_multiple));
    return cellector_em_finish(c, out);
}

// The EM state a load leaves, queued on the stream: all loci used, no cell excluded, the outputs zero (cellector_ingest_finish,
// cellector_em_reset)
cellector_status em_state_clear(cellector_ctx *c)
{
    const uint64_t L = c->L, n = c->nloc;
    HIPCHK(c, hipMemsetAsync(c->mask, 1, L ? L : 1, c->stream));  // load_data.rs:176-179: all loci used
    HIPCHK(c, hipMemsetAsync(c->mask_next, 1, L ? L : 1, c->stream));
    HIPCHK(c, hipMemsetAsync(c->flags, 0, n ? n : 1, c->stream));   // main.rs:37: the empty set
    HIPCHK(c, hipMemsetAsync(c->flags_new, 0, n ? n : 1, c->stream));
    HIPCHK(c, hipMemsetAsync(c->ll, 0, (n ? n : 1) * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(c->ell, 0, (n ? n : 1) * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(c->nloci, 0, (n ? n : 1) * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(c->x_norm, 0, (c->n_norm ? c->n_norm : 1) * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(c->x_locus, 0, ((uint64_t)LB_PLANES * L + LC_COUNTERS) * 8, c->stream));
    return CELLECTOR_OK;
}

// ---- placing the EM state ------------------------------------------------------------------------------
// (exclusion set, loci mask) is the whole state of the loop; everything else a ctx carries from one call to the next is
// derived from the two and is dropped or formed again here.
static cellector_status state_call_check(cellector_ctx *c, const char *what)
{
    READY(c);
    if (c->em_phase != 0) return ctx_fail(c, CELLECTOR_EINVAL, "%s: iteration in flight (finish it with cellector_em_finish)", what);
    // a shard whose exchanges the host drives has no exchange point here to hang the tally reduction on
    if (!comm_active(c->comm) && c->nloc != c->total_cells)
        return ctx_fail(c, CELLECTOR_EINVAL, "%s: a cellector_set_shard ctx without a communicator cannot place EM state "
                        "(attach a communicator, or use cellector_create_multi)", what);
    return CELLECTOR_OK;
}

// what the calls left for each other and was derived from the state that is being replaced
static void state_drop_carried(cellector_ctx *c)
{
    c->tally_valid = false;      // the next locus pass recounts tally / cnt2 (the path a reload takes)
    c->tables_prebuilt = false;  // em_finish queued k_build_tables from the OLD tallies and mask: the next em_begin builds again
    c->tab_event_valid = false;  // ... and forks the side stream from a fresh event, not from that kernel's
    c->filter_fused = false;
    c->work_zeroed = false;
    c->res_last_mode = 0;
    c->pa_last_mode = 0;
    c->pa_labels_changed = c->pa_qual_changed = 0;
    c->pa_ids.clear();
}

cellector_status cellector_set_excluded(cellector_ctx *c, const uint8_t *flags)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return multi_set_excluded(c, flags);
    CHK(state_call_check(c, "set_excluded"));
    REQUIRE(c, flags || c->nloc == 0, "set_excluded: null flags");
    SETDEV(c);
    const uint64_t n = c->nloc, L = c->L;
    std::vector<uint8_t> f(n);
    for (uint64_t i = 0; i < n; i++) f[i] = flags[i] ? 1 : 0;
    state_drop_carried(c);  // (forces recounts and rebuilds only: harmless should the placement fail below)
    CHK(launch_state_tallies(c, f.data()));  // allocates, then writes the flags and the tallies; synchronises
    // the exchange the locus pass of an iteration is followed by: global tallies and the global member count on every rank
    if (comm_active(c->comm)) CHK((cellector_status)comm_allreduce_sum(c, c->x_locus, (uint64_t)LB_PLANES * L + LC_COUNTERS));
    double n_exc = 0.0;
    CHK(d2h(c, &n_exc, c->x_locus + (uint64_t)LB_PLANES * L + LC_N_EXCLUDED, sizeof n_exc));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->n_excluded_global = (uint64_t)n_exc;
    return CELLECTOR_OK;
}

cellector_status cellector_set_loci_mask(cellector_ctx *c, const uint8_t *used)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return multi_set_loci_mask(c, used);
    CHK(state_call_check(c, "set_loci_mask"));
    REQUIRE(c, used || c->L == 0, "set_loci_mask: null mask");
    SETDEV(c);
    const uint64_t L = c->L;
    std::vector<uint8_t> m(L);
    uint64_t n_masked = 0;
    for (uint64_t l = 0; l < L; l++) {
        m[l] = used[l] ? 1 : 0;
        n_masked += m[l] ? 0 : 1;
    }
    // engine 2's recount needs an all-ones "old" mask: allocated before the mask is written, so a failure leaves the ctx as it was
    DevBuf<uint8_t> ones;
    if (c->tiled_ready && L && c->nloc) CHK(dev_alloc(c, &ones, L));
    state_drop_carried(c);
    if (L) {
        HIPCHK(c, hipMemcpyAsync(c->mask, m.data(), L, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->mask_next, m.data(), L, hipMemcpyHostToDevice, c->stream));
    }
    // engine 2 subtracts every cell's entries at masked loci from its used-locus count; engine 1 reads the mask itself
    // (k_alpha_beta marks a masked locus' alpha, k_cell_ll skips it): nothing else to place
    if (c->tiled_ready) CHK(tiled_masked_recount(c, ones.get()));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (m and the scratch may go)
    c->n_masked_loci = n_masked;
    return CELLECTOR_OK;
}

cellector_status cellector_em_reset(cellector_ctx *c)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return multi_em_reset(c);
    CHK(state_call_check(c, "em_reset"));
    SETDEV(c);
    const uint64_t n = c->nloc;
    state_drop_carried(c);
    CHK(em_state_clear(c));
    if (c->var) HIPCHK(c, hipMemsetAsync(c->var, 0, (n ? n : 1) * 8, c->stream));
    if (c->tiled_ready) {
        HIPCHK(c, hipMemsetAsync(c->masked_cnt, 0, (n ? n : 1) * 4, c->stream));
        HIPCHK(c, hipMemsetAsync(c->flag_bits, 0, ((n + 31) / 32 + 1) * 4, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->var_formed = false;
    c->lm_formed = false;
    c->iteration = 0; c->have_iter = false; c->n_excluded_global = 0; c->n_masked_loci = 0;
    c->last_median = c->last_iqr = c->last_thr = 0;
    return CELLECTOR_OK;
}

cellector_status cellector_iter_resolution(const cellector_ctx *c, cellector_resolution_t *out)
{
    if (!c || !out) return CELLECTOR_EINVAL;
    memset(out, 0, sizeof *out);
    if (c->multi || !c->res_last_mode) return CELLECTOR_OK;  // (nothing was resolved in the last iteration)
    REQUIRE(c, c->em_phase != 1, "iter_resolution between em_begin and em_threshold");
    uint32_t cnt[4];
    CHK(d2h(c, cnt, c->res_cnt, sizeof cnt));
    out->n_evaluated = (uint64_t)cnt[0] + cnt[1];
    out->n_flags_changed = cnt[2];
    out->changed = cnt[3];
    out->mode = (uint32_t)c->res_last_mode;
    return CELLECTOR_OK;
}

cellector_status cellector_iter_resolved_cells(const cellector_ctx *c, uint32_t *ids)
{
    if (!c || !ids) return CELLECTOR_EINVAL;
    if (c->multi || !c->res_last_mode) return CELLECTOR_OK;
    REQUIRE(c, c->em_phase != 1, "iter_resolved_cells between em_begin and em_threshold");
    uint32_t cnt[2];
    CHK(d2h(c, cnt, c->res_cnt, sizeof cnt));
    return d2h(c, ids, c->res_cand, ((uint64_t)cnt[0] + cnt[1]) * sizeof(uint32_t));
}

cellector_status cellector_iter_cell_outputs(const cellector_ctx *c, double *ll, double *ell, double *nl, double *norm)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return multi_iter_cell_outputs(c, ll, ell, nl, norm);
    READY(c);
    const size_t b = c->nloc * 8;
    if (ll) CHK(d2h(c, ll, c->ll, b));
    if (ell) CHK(d2h(c, ell, c->ell, b));
    if (nl) CHK(d2h(c, nl, c->nloci, b));
    if (norm) CHK(d2h(c, norm, c->x_norm + c->cell_begin, b));
    return CELLECTOR_OK;
}

cellector_status cellector_iter_locus_outputs(const cellector_ctx *c, double *cmin, double *cmaj, uint64_t *nmin,
                                              uint64_t *nmaj, uint64_t *amin, uint64_t *rmin, uint64_t *amaj,
                                              uint64_t *rmaj)
{
    if (!c) return CELLECTOR_EINVAL;
    SHARD0(c, cellector_iter_locus_outputs(s0__, cmin, cmaj, nmin, nmaj, amin, rmin, amaj, rmaj));
    READY(c);
    REQUIRE(c, c->have_iter && c->em_phase == 0, "no finished iteration");
    const uint64_t L = c->L;
    std::vector<double> buf(LB_PLANES * L), sa(L), sr(L), ne(L);
    std::vector<uint8_t> m(L);
    CHK(d2h(c, buf.data(), c->x_locus, LB_PLANES * L * 8));
    CHK(d2h(c, sa.data(), c->s_alt, L * 8));
    CHK(d2h(c, sr.data(), c->s_ref, L * 8));
    CHK(d2h(c, ne.data(), c->n_ent, L * 8));
    CHK(d2h(c, m.data(), c->mask_next, L));  // the mask this iteration's passes ran under
    for (uint64_t l = 0; l < L; l++) {
        const bool live = m[l] != 0;  // a masked locus has no PMFData at all (main.rs:556)
        const double am = buf[LB_ALT_MIN * L + l], rm = buf[LB_REF_MIN * L + l], cm = buf[LB_CELLS_MIN * L + l];
        if (cmin) cmin[l] = buf[LB_CONTRIB_MIN * L + l];
        if (cmaj) cmaj[l] = buf[LB_CONTRIB_MAJ * L + l];
        if (nmin) nmin[l] = (uint64_t)cm;
        if (nmaj) nmaj[l] = live ? (uint64_t)(ne[l] - cm) : 0;
        if (amin) amin[l] = live ? (uint64_t)am : 0;
        if (rmin) rmin[l] = live ? (uint64_t)rm : 0;
        if (amaj) amaj[l] = live ? (uint64_t)(sa[l] - am) : 0;
        if (rmaj) rmaj[l] = live ? (uint64_t)(sr[l] - rm) : 0;
    }
    return CELLECTOR_OK;
}

cellector_status cellector_loci_mask(const cellector_ctx *c, uint8_t *out)
{
    if (!c) return CELLECTOR_EINVAL;
    SHARD0(c, cellector_loci_mask(s0__, out));
    READY(c);
    return d2h(c, out, c->mask, c->L);
}

cellector_status cellector_excluded(const cellector_ctx *c, uint8_t *out)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return multi_excluded(c, out);
    READY(c);
    return d2h(c, out, c->flags, c->nloc);
}

cellector_status cellector_alpha_betas(const cellector_ctx *c, double *alpha, double *beta)
{
    if (!c) return CELLECTOR_EINVAL;
    SHARD0(c, cellector_alpha_betas(s0__, alpha, beta));
    READY(c);
    const uint64_t L = c->L;
    std::vector<double> buf(LB_PLANES * L), sa(L), sr(L);
    CHK(d2h(c, buf.data(), c->x_locus, LB_PLANES * L * 8));
    CHK(d2h(c, sa.data(), c->s_alt, L * 8));
    CHK(d2h(c, sr.data(), c->s_ref, L * 8));
    for (uint64_t l = 0; l < L; l++) {
        if (alpha) alpha[l] = (sa[l] + 1.0) - buf[LB_ALT_MIN * L + l];
        if (beta) beta[l] = (sr[l] + 1.0) - buf[LB_REF_MIN * L + l];
    }
    return CELLECTOR_OK;
}

cellector_status cellector_cell_log_likelihoods(cellector_ctx *c, const double *alpha, const double *beta,
                                                const uint8_t *mask, double *ll, double *ell, double *nl)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return multi_cell_log_likelihoods(c, alpha, beta, mask, ll, ell, nl);
    READY(c);
    REQUIRE(c, alpha && beta, "null alpha/beta");
    REQUIRE(c, c->em_phase == 0, "iteration in flight");
    SETDEV(c);
    c->tables_prebuilt = false;  // this pass overwrites alpha/beta and the tables
    c->work_zeroed = false;
    CHK(launch_ab_from_host(c, alpha, beta, mask));
    // the tiled engine subtracts every cell's entries at masked loci from its used-locus count: the counts of THIS call's mask
    // go into scratch (the ctx's own masked_cnt belongs to the loop's mask and stays)
    if (c->engine == 2) {
        DevBuf<uint32_t> cnt;
        CHK(dev_alloc(c, &cnt, c->nloc));
        CHK(tiled_call_masked_count(c, mask, cnt.get()));
        CHK(tiled_cell_pass(c, c->ab, nullptr, false, cnt.get()));
        HIPCHK(c, hipStreamSynchronize(c->stream));  // (the scratch goes)
    } else CHK(launch_cell_ll(c, c->ab, nullptr));
    const size_t b = c->nloc * 8;
    if (ll) CHK(d2h(c, ll, c->ll, b));
    if (ell) CHK(d2h(c, ell, c->ell, b));
    if (nl) CHK(d2h(c, nl, c->nloci, b));
    if (c->timing) timer_collect(c);
    return CELLECTOR_OK;
}

// PMFData (main.rs:527-539) of listed cells: kernels_pmfs.hip
cellector_status cellector_cell_pmfs(cellector_ctx *c, const double *alpha, const double *beta, const uint8_t *mask, const uint32_t *cells,
                                     uint64_t n_cells, uint64_t *rec_ptr, uint64_t capacity, uint32_t *locus_index, uint32_t *alt,
                                     uint32_t *ref, double *log_pmf, double *expected_log_pmf, double *expected_log_variance)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi)
        return multi_cell_pmfs(c, alpha, beta, mask, cells, n_cells, rec_ptr, capacity, locus_index, alt, ref, log_pmf, expected_log_pmf,
                               expected_log_variance);
    READY(c);
    REQUIRE(c, c->em_phase == 0, "cell_pmfs: iteration in flight (finish it with cellector_em_finish)");
    REQUIRE(c, (alpha && beta) || c->L == 0, "cell_pmfs: null alpha/beta");
    REQUIRE(c, rec_ptr && (cells || n_cells == 0), "cell_pmfs: null rec_ptr or cell list");
    for (uint64_t j = 0; j < n_cells; j++)  // every id before anything is written or launched
        if (cells[j] >= c->nloc)
            return ctx_fail(c, CELLECTOR_EINVAL, "cell_pmfs: cell id %u (list position %llu) out of range: %llu cells", cells[j],
                            (unsigned long long)j, (unsigned long long)c->nloc);
    SETDEV(c);
    return pmfs_run(c, alpha, beta, mask, cells, n_cells, rec_ptr, capacity, locus_index, alt, ref, log_pmf, expected_log_pmf,
                    expected_log_variance);
}

// expected_log_variances (main.rs:587) under caller alpha/beta/mask: kernels_variance.hip
cellector_status cellector_cell_log_variances(cellector_ctx *c, const double *alpha, const double *beta, const uint8_t *mask,
                                              double *expected_log_variance)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return multi_cell_log_variances(c, alpha, beta, mask, expected_log_variance);
    READY(c);
    REQUIRE(c, c->em_phase == 0, "cell_log_variances: iteration in flight (finish it with cellector_em_finish)");
    REQUIRE(c, (alpha && beta) || c->L == 0, "cell_log_variances: null alpha/beta");
    REQUIRE(c, expected_log_variance || c->nloc == 0, "cell_log_variances: null output");
    SETDEV(c);
    return variance_run(c, alpha, beta, mask, expected_log_variance);
}

cellector_status cellector_iter_cell_variances(const cellector_ctx *c, double *out)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return multi_iter_cell_variances(c, out);
    READY(c);
    REQUIRE(c, c->em_phase == 0, "iter_cell_variances: iteration in flight (finish it with cellector_em_finish)");
    REQUIRE(c, c->var_formed, "iter_cell_variances: not formed (the last finished iteration ran with options cell_variance and "
                              "normalization both 0, or none has finished since the load / cellector_em_reset)");
    REQUIRE(c, out || c->nloc == 0, "iter_cell_variances: null output");
    if (c->nloc == 0) return CELLECTOR_OK;
    return d2h(c, out, c->var, c->nloc * 8);
}

// ---- locus moments: kernels_locus_moments.hip -----------------------------------------------------------
cellector_status cellector_locus_moments(cellector_ctx *c, const double *alpha, const double *beta, const uint8_t *mask, const uint8_t *flags,
                                         double *exp_min, double *exp_maj, double *var_min, double *var_maj)
{
    if (!c) return CELLECTOR_EINVAL;
    CHK(model_call_scope(c, "locus_moments"));
    REQUIRE(c, (alpha && beta) || c->L == 0, "locus_moments: null alpha/beta");
    REQUIRE(c, flags || c->nloc == 0, "locus_moments: null flags");
    SETDEV(c);
    return locus_moments_run(c, alpha, beta, mask, flags, exp_min, exp_maj, var_min, var_maj);
}

cellector_status cellector_locus_total_counts(cellector_ctx *c, const uint8_t *flags, uint32_t *out)
{
    if (!c) return CELLECTOR_EINVAL;
    CHK(model_call_scope(c, "locus_total_counts"));
    REQUIRE(c, out || c->L == 0, "locus_total_counts: null output");
    SETDEV(c);
    return locus_total_counts_run(c, flags, out);
}

cellector_status cellector_iter_locus_moments(const cellector_ctx *c, double *exp_min, double *exp_maj, double *var_min, double *var_maj)
{
    if (!c) return CELLECTOR_EINVAL;
    CHK(model_call_scope(c, "iter_locus_moments"));
    REQUIRE(c, c->lm_formed, "iter_locus_moments: not formed (the last finished iteration ran with option locus_moments 0, or none "
                             "has finished since the load / cellector_em_reset)");
    const uint64_t L = c->L;
    double *const out[4] = {exp_min, exp_maj, var_min, var_maj};
    for (int k = 0; k < 4; k++)
        if (out[k] && L) CHK(d2h(c, out[k], c->lm_out + (uint64_t)k * L, L * 8));
    return CELLECTOR_OK;
}

// (a shard of a multi-device ctx is handed its slice of the keys; n_total = all keys)
cellector_status ffi_order_statistics(cellector_ctx *c, const double *keys, uint64_t n_local, uint64_t n_total, double iqr_multiple, double *out3)
{
    REQUIRE(c, n_total > 0 && (keys || !n_local), "order statistics: no keys");
    SETDEV(c);
    DevBuf<double> d_keys;
    CHK(dev_alloc(c, &d_keys, n_local ? n_local : 1));
    cellector_status st = CELLECTOR_OK;
    if (n_local && hipMemcpyAsync(d_keys, keys, n_local * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess)
        st = ctx_fail(c, CELLECTOR_EDEVICE, "upload of the keys failed");
    if (st == CELLECTOR_OK)
        st = comm_active(c->comm) && comm_sharded_select(c->comm, c->sharded_select, n_total) ? select_threshold_sharded(c, d_keys, n_local, n_total, iqr_multiple)
                                                       : select_threshold(c, d_keys, n_local, iqr_multiple);
    if (st == CELLECTOR_OK && out3) st = d2h(c, out3, c->sel_out + 8, 3 * sizeof(double));
    else (void)hipStreamSynchronize(c->stream);
    return st;
}
cellector_status cellector_order_statistics(cellector_ctx *c, const double *keys, uint64_t n, double iqr_multiple, double *out3)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return multi_order_statistics(c, keys, n, iqr_multiple, out3);
    REQUIRE(c, !comm_active(c->comm) || c->comm.n == 1,
            "order statistics on one rank of a communicator: every rank would have to call with its slice");
    return ffi_order_statistics(c, keys, n, n, iqr_multiple, out3);
}
