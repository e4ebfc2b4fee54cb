// The options and the cell ranges of a ctx: cellector_set_option, set_partition, partition, set_shard.  Switching to engine 2 on a
// loaded ctx builds the tiles (kernels_tiled_build.hip); nothing else here launches.
#include <cstring>

#include "api_checks.h"
#include "ref_log.h"

// ref_log.h repeats the C library's log (glibc >= 2.28 as selected on a CPU with FMA).  A host whose log is another one (an
// older glibc, the variant without FMA on a CPU or VM that hides it) would give other bits: checked once, on arguments where
// that log is not correctly rounded (a correctly rounded or differently built log differs there) and a few ordinary ones.
static bool ref_log_matches_host()
{
    static const int ok = [] {
        const double xs[] = {0x1.1000000000001p+0, 0x1.9029699ac8b51p-1, 0x1.107d0786575abp+9, 0x1.9d92c3bf393efp+264,
                             0x1.244a7d7500750p-319, 0x1.0cf011ed22e53p-1, 0x1.6e752447f96bdp+40, 0x1.5abd26f74c705p+17,
                             0x1.0d67af17a1c3dp+14, 0x1.a16d6a77cb0b3p-16, 2.0, 0.5, 3.0, 1e6, 0.999999, 1.000001};
        for (double x : xs) {
            volatile double vx = x;  // (the host's log at run time, not a constant folded by the compiler)
            const double a = std::log(vx), b = ref_log(x);
            if (memcmp(&a, &b, sizeof a) != 0) return 0;
        }
        return 1;
    }();
    return ok != 0;
}

cellector_status cellector_set_option(cellector_ctx *c, const char *key, int64_t v)
{
    if (!c || !key) return CELLECTOR_EINVAL;
    if (!strcmp(key, "resolve_ties")) {
        if (v < 0 || v > 2) return ctx_fail(c, CELLECTOR_EINVAL, "resolve_ties must be 0 (off), 1 (the near-tie bands) or 2 (every cell)");
        if (v && (c->multi || comm_active(c->comm)))
            return ctx_fail(c, CELLECTOR_EINVAL, "resolve_ties works on a single-device ctx: a sharded run would need the candidates of every shard");
        if (c->multi) return CELLECTOR_OK;  // (0 on a multi-device ctx: nothing to switch off)
        if (v && c->normalization)
            return ctx_fail(c, CELLECTOR_EINVAL, "resolve_ties with normalization 1: the reference has no arithmetic of the z-score "
                                                 "mode to resolve to (set normalization 0 first)");
        if (v && c->state == cellector_ctx::ST_READY && c->nnz && !c->res_ent)
            return ctx_fail(c, CELLECTOR_EINVAL, "resolve_ties keeps every cell's entries in file order at the ingest: set it before the ingest");
        if (v && !ref_log_matches_host())
            return ctx_fail(c, CELLECTOR_EINVAL, "resolve_ties: this host's C library log differs from the one ref_log.h repeats "
                                                 "(glibc >= 2.28, FMA variant), so the reference's bits cannot be promised");
        c->resolve_ties = (int)v;
        return CELLECTOR_OK;
    }
    if (!strcmp(key, "resolve_posteriors")) {
        if (v < 0 || v > 2)
            return ctx_fail(c, CELLECTOR_EINVAL, "resolve_posteriors must be 0 (off), 1 (the cells next to a decision edge) or 2 (every cell)");
        if (v && (c->multi || comm_active(c->comm)))
            return ctx_fail(c, CELLECTOR_EINVAL, "resolve_posteriors works on a single-device ctx");
        if (c->multi) return CELLECTOR_OK;  // (0 on a multi-device ctx: nothing to switch off)
        if (v && c->state == cellector_ctx::ST_READY && c->nnz && !c->res_ent)
            return ctx_fail(c, CELLECTOR_EINVAL, "resolve_posteriors needs every cell's entries in file order, kept at the ingest: set it before the ingest");
        if (v && !ref_log_matches_host())
            return ctx_fail(c, CELLECTOR_EINVAL, "resolve_posteriors: this host's C library log differs from the one ref_log.h repeats "
                                                 "(glibc >= 2.28, FMA variant), so the reference's bits cannot be promised");
        c->resolve_posteriors = (int)v;
        return CELLECTOR_OK;
    }
    if (!strcmp(key, "locus_moments")) {
        if (v != 0 && v != 1) return ctx_fail(c, CELLECTOR_EINVAL, "locus_moments must be 0 (off) or 1");
        if (v) CHK(whole_matrix_scope(c, "locus_moments 1"));
        if (c->multi) return CELLECTOR_OK;  // (0 on a multi-device ctx: nothing to switch off)
        c->locus_moments = v != 0;
        return CELLECTOR_OK;
    }
    if (c->multi) return multi_set_option(c, key, v);
    if (!strcmp(key, "compute_expected")) {
        if (!v && c->normalization)
            return ctx_fail(c, CELLECTOR_EINVAL, "compute_expected 0 with normalization 1: the z-score needs the expected term "
                                                 "(set normalization 0 first)");
        c->compute_expected = v != 0;
    }
    else if (!strcmp(key, "cell_variance")) c->cell_variance = v != 0;
    else if (!strcmp(key, "normalization")) {
        if (v != 0 && v != 1)
            return ctx_fail(c, CELLECTOR_EINVAL, "normalization must be 0 (log-likelihood per used locus, main.rs:316) or 1 (z-score, main.rs:317-318)");
        if (v && c->resolve_ties)
            return ctx_fail(c, CELLECTOR_EINVAL, "normalization 1 with resolve_ties %d: the reference has no arithmetic of the z-score "
                                                 "mode to resolve to (set resolve_ties 0 first)", c->resolve_ties);
        if (v && !c->compute_expected)
            return ctx_fail(c, CELLECTOR_EINVAL, "normalization 1 with compute_expected 0: the z-score needs the expected term "
                                                 "(set compute_expected 1 first)");
        c->normalization = (int)v;
    }
    else if (!strcmp(key, "ref_arith")) {
        if (v && c->engine != 1) return ctx_fail(c, CELLECTOR_EINVAL, "ref_arith evaluates every entry with the reference's ln_gamma arithmetic: an engine 1 option (set engine 1 first)");
        c->ref_arith = v != 0;
    }
    else if (!strcmp(key, "timing")) {
        c->timing = v < 0 ? 0 : (v > 3 ? 3 : (int)v);
        for (KernelTimer &t : c->timers) t.calls = 0;
        if (c->timing && hipSetDevice(c->device) == hipSuccess)  // events ready before the timed loop starts
            while (c->ev_pool.size() < 64) {
                hipEvent_t e;
                if (hipEventCreate(&e) != hipSuccess) break;
                c->ev_pool.push_back(e);
            }
    }
    else if (!strcmp(key, "keep_coo")) c->keep_coo = v != 0;
    else if (!strcmp(key, "bank_order")) c->bank_order = v != 0;
    else if (!strcmp(key, "fuse_filter")) c->fuse_filter = v != 0;
    else if (!strcmp(key, "synth_continue_pct")) {
        if (v < 0 || v > 90) return ctx_fail(c, CELLECTOR_EINVAL, "synth_continue_pct must be within 0..90");
        c->synth_continue_pct = (int)v;
    }
    else if (!strcmp(key, "overlap")) {
        if (v < 0 || v > 2) return ctx_fail(c, CELLECTOR_EINVAL, "overlap must be 0, 1 or 2");
        c->overlap = (int)v;
    }
    else if (!strcmp(key, "side_lds")) c->side_lds = (int)v;
    else if (!strcmp(key, "ovf_deep_wide")) c->ovf_deep_wide = v != 0;
    else if (!strcmp(key, "ovf_deep")) {
        if (v < -1 || v > 1) return ctx_fail(c, CELLECTOR_EINVAL, "ovf_deep must be -1 (automatic), 0 or 1");
        if (c->tiled_ready && v >= 0 && c->ovf_deep != (v != 0))
            return ctx_fail(c, CELLECTOR_EINVAL, "ovf_deep decides which overflow layouts the ingest builds: set it before the ingest");
        c->ovf_deep_opt = (int)v;
    }
    else if (!strcmp(key, "t2_waves")) {
        if (v < 0 || v > (1 << 20)) return ctx_fail(c, CELLECTOR_EINVAL, "t2_waves must be 0 (automatic) or within 1..2^20");
        c->t2_waves = (int)v;
    }
    else if (!strcmp(key, "t2_helper")) {
        if (v < -1 || v > 64) return ctx_fail(c, CELLECTOR_EINVAL, "t2_helper must be -1 (automatic), 0 (off) or 1..64 blocks per free CU (forced)");
        c->t2_helper = (int)v;
    }
    else if (!strcmp(key, "t2_cache")) {
        if (v < -1 || v > 1) return ctx_fail(c, CELLECTOR_EINVAL, "t2_cache must be -1 (automatic), 0 (off) or 1 (on)");
        c->t2_cache = (int)v;
    }
    else if (!strcmp(key, "t2_fill")) {
        if (v < -1 || v > 1) return ctx_fail(c, CELLECTOR_EINVAL, "t2_fill must be -1 (decided on the device), 0 (bypass) or 1 (fill)");
        c->t2_fill = (int)v;
    }
    else if (!strcmp(key, "t2")) {
        if (v < -1 || v > 1) return ctx_fail(c, CELLECTOR_EINVAL, "t2 must be -1 (automatic), 0 or 1");
        if (c->tiled_ready && v >= 0 && c->t2 != (v != 0))
            return ctx_fail(c, CELLECTOR_EINVAL, "t2 decides which overflow layouts the ingest builds: set it before the ingest");
        c->t2_opt = (int)v;
    }
    else if (!strcmp(key, "t2_tiles")) {
        if (!(v == -1 || v == 0 || v == 6 || v == 8)) return ctx_fail(c, CELLECTOR_EINVAL, "t2_tiles must be -1 (automatic), 0, 6 or 8");
        if (c->tiled_ready && v >= 0 && c->t2_tiles != (int)v)
            return ctx_fail(c, CELLECTOR_EINVAL, "t2_tiles decides which layouts the ingest builds: set it before the ingest");
        c->t2_tiles_opt = (int)v;
    }
    else if (!strcmp(key, "norm_zero")) c->norm_zero = v != 0;
    else if (!strcmp(key, "sharded_select")) c->sharded_select = v < 0 ? -1 : (v != 0);
    else if (!strcmp(key, "parse_window")) c->parse_window_opt = v < 0 ? 0 : v;
    else if (!strcmp(key, "write_window")) c->write_window_opt = v < 0 ? 0 : v;
    else if (!strcmp(key, "gz_device")) {
        if (v != 0 && v != 1) return ctx_fail(c, CELLECTOR_EINVAL, "gz_device must be 0 (a .gz is inflated on the host) or 1 (a BGZF .gz on the device)");
        c->gz_device = v != 0;
    }
    else if (!strcmp(key, "tile_groups")) {
        if (v < 0 || v > 64) return ctx_fail(c, CELLECTOR_EINVAL, "tile_groups must be 0 (automatic) or 1..64");
        c->tile_groups_opt = (int)v;
    }
    else if (!strcmp(key, "tile_sb")) {
        if (v != 0 && v != 2 && v != 4) return ctx_fail(c, CELLECTOR_EINVAL, "tile_sb must be 0 (automatic), 2 or 4");
        c->tile_sb_opt = (int)v;
    }
    else if (!strcmp(key, "locus_mode")) {
        if (v < 0 || v > 2) return ctx_fail(c, CELLECTOR_EINVAL, "locus_mode must be 0 (automatic), 1 (stream) or 2 (minority-driven)");
        c->locus_mode = (int)v;
    }
    else if (!strcmp(key, "tally_delta")) {
        if (v != 0 && v != 1) return ctx_fail(c, CELLECTOR_EINVAL, "tally_delta must be 0 (recount every iteration) or 1");
        c->tally_delta = v != 0;
    }
    else if (!strcmp(key, "class_delta")) {
        if (v != 0 && v != 1) return ctx_fail(c, CELLECTOR_EINVAL, "class_delta must be 0 (recount every refine step) or 1");
        c->class_delta = v != 0;
    }
    else if (!strcmp(key, "compact_bits")) {
        if (v != 0 && v != 32) return ctx_fail(c, CELLECTOR_EINVAL, "compact_bits must be 0 (automatic) or 32");
        c->c4_bits_opt = (int)v;
    } else if (!strcmp(key, "engine")) {
        if (v != 1 && v != 2) return ctx_fail(c, CELLECTOR_EINVAL, "engine must be 1 (CSR/CSC kernels) or 2 (tiled)");
        if (c->em_phase != 0) return ctx_fail(c, CELLECTOR_EINVAL, "cannot switch engine inside an iteration");
        if (v == 1 && c->state == cellector_ctx::ST_READY && !c->csc_ent && c->nnz)
            return ctx_fail(c, CELLECTOR_EINVAL, "engine 1 needs the by-locus CSC, which an engine-2 ingest releases: set engine 1 before the ingest");
        if (v == 2 && c->state == cellector_ctx::ST_READY && !c->tiled_ready) {
            HIPCHK(c, hipSetDevice(c->device));
            if (c->n_masked_loci) return ctx_fail(c, CELLECTOR_EINVAL, "switch to engine 2 before any locus is masked");
            CHK(tiled_build(c));
        }
        if (v == 2 && c->ref_arith) return ctx_fail(c, CELLECTOR_EINVAL, "ref_arith is an engine 1 option: clear it before switching to engine 2");
        c->engine = (int)v;
        // engine 1 moves the exclusion set without engine 2's kept counts; the fused filter is engine 2's alone
        c->tally_valid = false;
        c->filter_fused = false;
    }
    else return ctx_fail(c, CELLECTOR_EINVAL, "unknown option '%s'", key);
    return CELLECTOR_OK;
}

cellector_status cellector_set_partition(cellector_ctx *c, const uint64_t *bounds, int n_bounds)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return multi_set_partition(c, bounds, n_bounds);
    REQUIRE(c, comm_active(c->comm), "set_partition: the ctx has no communicator (a single shard takes cellector_set_shard)");
    REQUIRE(c, c->state == cellector_ctx::ST_EMPTY, "set_partition must precede the ingest");
    if (!bounds || n_bounds == 0) {  // back to the canonical equal ranges
        c->comm.has_bounds = false;
        c->tally_valid = false;
        return CELLECTOR_OK;
    }
    REQUIRE(c, n_bounds == c->comm.n + 1, "set_partition: one boundary more than there are ranks");
    REQUIRE(c, bounds[0] == 0, "set_partition: the first range starts at cell 0");
    for (int r = 0; r < c->comm.n; r++) REQUIRE(c, bounds[r] <= bounds[r + 1], "set_partition: boundaries must not decrease");
    for (int r = 0; r <= c->comm.n; r++) c->comm.bounds[r] = bounds[r];
    c->comm.has_bounds = true;
    c->tally_valid = false;
    return CELLECTOR_OK;
}

cellector_status cellector_partition(const cellector_ctx *c, uint64_t *bounds_out, int *n_ranks)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) c = multi_shard0(c);
    if (n_ranks) *n_ranks = c->comm.n;
    if (bounds_out) {
        REQUIRE(c, c->state != cellector_ctx::ST_EMPTY, "partition: nothing loaded yet");
        for (int r = 0; r < c->comm.n; r++) {
            uint64_t b, e;
            comm_range(c->comm, c->total_cells, r, &b, &e);
            bounds_out[r] = b;
            bounds_out[r + 1] = e;
        }
        if (c->comm.n == 1) { bounds_out[0] = c->cell_begin; bounds_out[1] = c->cell_end; }
    }
    return CELLECTOR_OK;
}

cellector_status cellector_set_shard(cellector_ctx *c, uint64_t b, uint64_t e)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi || comm_active(c->comm))
        return ctx_fail(c, CELLECTOR_EINVAL, "a ctx with a communicator shards the cells itself (contiguous ranges by rank: cellector_set_partition)");
    REQUIRE(c, c->state == cellector_ctx::ST_EMPTY, "set_shard must precede ingest");
    REQUIRE(c, b <= e, "empty or inverted shard range");
    REQUIRE(c, !(c->locus_moments && b != 0), "set_shard: option locus_moments 1 works on a ctx that holds all cells (set it 0 first)");
    c->req_cell_begin = b;
    c->req_cell_end = e;
    c->tally_valid = false;  // (the ingest that must follow rebuilds the counts anyway)
    return CELLECTOR_OK;
}
