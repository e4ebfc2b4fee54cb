// The re-staging calls of the C ABI: cellector_restage, cellector_combine and cellector_add_doublets replace the staged COO of a ctx
// by one made from entries already on the device (kernels_restage.hip, kernels_combine.hip, kernels_doublets.hip) and take a READY
// ctx back to STAGED; cellector_cell_origin, cellector_cell_source and cellector_staged_coo read the result, and
// cellector_write_mtx / cellector_format_mtx (kernels_mtx_write.hip) render it as mtx text.
#include <vector>

#include "ctx.h"

// why a ctx cannot take part in a re-staging call, or null.  They work where one device holds every cell (the conditions of
// whole_matrix_scope of api_checks.h, without its entry limit), between iterations, on a staged COO that is still there
static const char *restage_scope(const cellector_ctx *c)
{
    if (c->multi) return "is a multi-device ctx: its staged entries are sharded";
    if (comm_active(c->comm)) return "has a communicator: every rank stages its own cells";
    if (c->state == cellector_ctx::ST_EMPTY) return "has no staged matrix";
    if (c->nloc != c->total_cells) return "holds a cellector_set_shard range, not all cells";
    if (c->em_phase != 0) return "is between cellector_em_begin and cellector_em_finish";
    if (!c->coo.locus) return "is a loaded matrix without its staged COO (option keep_coo=1 before the ingest)";
    return nullptr;
}

// the threshold of the per-read draw: T = rate * 2^53 (0: the counts are copied)
static cellector_status thin_threshold(const cellector_ctx *c, const char *call, double downsample_rate, uint64_t *T)
{
    if (!(downsample_rate >= 0.0 && downsample_rate <= 1.0))  // (NaN fails both comparisons)
        return ctx_fail(c, CELLECTOR_EINVAL, "%s: downsample_rate %g is not in [0, 1]", call, downsample_rate);
    *T = (uint64_t)(downsample_rate * 9007199254740992.0);  // 2^53
    return CELLECTOR_OK;
}

// READY -> STAGED on the entries the ctx still holds: everything built from them goes as in a reload, the staged group stays
// (ingest_build only read PASS1).  The blocks stay in the cache: the new COO and the finish that follows take them from there.
static void unbuild_matrix(cellector_ctx *c, CallLaps &lap)
{
    if (c->state != cellector_ctx::ST_READY) return;
    drop_built(c);
    c->state = cellector_ctx::ST_STAGED;
    lap("drop built matrix");
}

// The commit point of a re-staging call: the new entries, origin and source move in over the old ones, the dims follow.  Nothing
// here fails.
static void staged_commit(cellector_ctx *c, StagedCoo &&coo, DevBuf<uint32_t> &&origin, DevBuf<uint8_t> &&source, uint64_t total_loci,
                          uint64_t total_cells)
{
    c->coo = std::move(coo);
    c->cell_origin = std::move(origin);
    c->cell_source = std::move(source);
    c->total_loci = total_loci;
    c->total_cells = total_cells; c->cell_begin = 0; c->cell_end = total_cells; c->nloc = total_cells;
    c->state = cellector_ctx::ST_STAGED;
}

// One side appended to the staged matrix as the next combine (cellector_combine, cellector_add_doublets).  `side` carries its final
// locus and cell numbers (cells from total_cells on), side_origin [n_side] (device) their origin; a side that does not ascend by
// (locus, cell) is sorted (sort_side) or an internal error.  The built matrix goes first; everything new is made beside the old
// entries and moved in at the end, so a failure on the way leaves the ctx STAGED with its old entries, dims, origin and source.
static cellector_status staged_append(cellector_ctx *c, CallLaps &lap, StagedCoo *side, const uint32_t *side_origin, uint64_t n_side,
                                      uint64_t total_loci_out, bool sort_side)
{
    unbuild_matrix(c, lap);
    const uint64_t n_ctx = c->total_cells;
    StagedCoo own_sorted, side_sorted, merged;
    DevBuf<uint32_t> origin;
    DevBuf<uint8_t> source;
    DevBuf<double> p1;
    CHK(combine_cells(c, n_ctx, n_side, c->cell_origin, side_origin, c->cell_source, (uint8_t)(c->n_combines + 1), &origin, &source));
    CooView a = c->coo.view(), b = side->view();
    bool asc_a = true, asc_b = true;
    CHK(combine_ascending(c, a, b, &asc_a, &asc_b));
    if (!asc_b && !sort_side) return ctx_fail(c, CELLECTOR_EDEVICE, "add_doublets: the doublet side does not ascend by (locus, cell)");
    if (!asc_a) { CHK(combine_sort(c, a, &own_sorted)); a = own_sorted.view(); }
    if (!asc_b) { CHK(combine_sort(c, b, &side_sorted)); side->reset(); b = side_sorted.view(); }
    lap("order check / sort");
    CHK(combine_merge(c, a, b, &merged));
    lap("merge");
    // PASS1 follows the locus count: the library's own buffer is made anew, a bound one was checked by the caller
    const uint64_t need_p1 = (uint64_t)P1_PLANES * total_loci_out;
    if (!c->pass1_bound && need_p1 != c->n_pass1) CHK(dev_alloc(c, &p1, need_p1));
    // ---- nothing below fails for memory
    staged_commit(c, std::move(merged), std::move(origin), std::move(source), total_loci_out, n_ctx + n_side);
    c->n_combines++;
    if (p1) { c->x_pass1_own = std::move(p1); c->x_pass1 = c->x_pass1_own; }
    c->n_pass1 = need_p1;
    CHK(ingest_pass1(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    lap("release + PASS1");
    return CELLECTOR_OK;
}

extern "C" {

// ---- a cell subset and per-read downsampling ------------------------------------------------------------------
cellector_status cellector_restage(cellector_ctx *c, const uint8_t *keep, double downsample_rate, uint64_t seed)
{
    if (!c) return CELLECTOR_EINVAL;
    // (a root ctx is refused in the words of the other calls that work on a single-device ctx)
    if (c->multi) return ctx_fail(c, CELLECTOR_EINVAL, "restage works on a single-device ctx: the staged entries of a multi-device ctx are sharded");
    if (const char *why = restage_scope(c)) return ctx_fail(c, CELLECTOR_EINVAL, "restage: ctx %s", why);
    uint64_t T = 0;
    CHK(thin_threshold(c, "restage", downsample_rate, &T));
    const uint64_t tc = c->total_cells;
    uint64_t n_keep = tc;
    if (keep) {
        n_keep = 0;
        for (uint64_t i = 0; i < tc; i++) n_keep += keep[i] != 0;
        if (n_keep == 0) return ctx_fail(c, CELLECTOR_EINVAL, "restage: the selection keeps none of the %llu cells", (unsigned long long)tc);
        if (n_keep == tc) keep = nullptr;  // every cell stays: nothing to renumber
    }
    SETDEV(c);
    CallLaps lap{"restage"};
    // ---- validated: from here the ctx changes.  The built matrix goes first, then the new COO is made beside the old one
    unbuild_matrix(c, lap);
    if (keep) {
        DevBuf<uint8_t> keep01;
        DevBuf<uint32_t> rank, origin;
        DevBuf<uint8_t> source;
        StagedCoo neu;
        CHK(restage_cell_ranks(c, keep, tc, n_keep, c->cell_origin, &keep01, &rank, &origin));
        if (c->cell_source) CHK(combine_source_select(c, tc, n_keep, rank, c->cell_source, &source));
        lap("cell ranks");
        CHK(restage_select(c, c->coo.view(), tc, keep01, rank, T, seed, &neu));  // (a failure up to here leaves the old entries staged)
        lap("count + scan + write");
        neu.sorted = c->coo.sorted;  // (a subsequence of a locus-major order is locus-major)
        staged_commit(c, std::move(neu), std::move(origin), std::move(source), c->total_loci, n_keep);  // (no source before: none now)
    } else {
        CHK(restage_thin(c, &c->coo, T, seed));
        lap("thin");
    }
    CHK(ingest_pass1(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    lap("release + PASS1");
    return CELLECTOR_OK;
}

cellector_status cellector_cell_origin(const cellector_ctx *c, uint32_t *out)
{
    if (!c || !out) return CELLECTOR_EINVAL;
    cellector_dims_t d;
    CHK(cellector_dims(c, &d));
    if (!c->multi && c->cell_origin) return d2h(c, out, c->cell_origin, d.total_cells * 4);
    for (uint64_t i = 0; i < d.total_cells; i++) out[i] = (uint32_t)i;
    return CELLECTOR_OK;
}

cellector_status cellector_cell_source(const cellector_ctx *c, uint8_t *out)
{
    if (!c || !out) return CELLECTOR_EINVAL;
    cellector_dims_t d;
    CHK(cellector_dims(c, &d));
    if (!c->multi && c->cell_source) return d2h(c, out, c->cell_source, d.total_cells);
    memset(out, 0, d.total_cells);
    return CELLECTOR_OK;
}

cellector_status cellector_staged_coo(const cellector_ctx *c, uint64_t *n, uint32_t *locus0, uint32_t *cell0, uint32_t *alt, uint32_t *ref,
                                      uint64_t capacity)
{
    if (!c || !n) return CELLECTOR_EINVAL;
    if (c->multi) return ctx_fail(c, CELLECTOR_EINVAL, "staged_coo works on a single-device ctx (the staged entries of a multi-device ctx are sharded)");
    REQUIRE(c, c->state != cellector_ctx::ST_EMPTY && c->coo.locus, "staged_coo without a staged matrix (option keep_coo=1)");
    *n = c->coo.n;
    if (!locus0 && !cell0 && !alt && !ref) return CELLECTOR_OK;
    REQUIRE(c, capacity >= c->coo.n, "staged_coo: capacity too small");
    const uint64_t m = c->coo.n;
    if (locus0) CHK(d2h(c, locus0, c->coo.locus, m * 4));
    if (cell0) CHK(d2h(c, cell0, c->coo.cell, m * 4));
    std::vector<uint16_t> h(m);
    for (int k = 0; k < 2; k++) {
        uint32_t *dst = k ? ref : alt;
        if (!dst) continue;
        CHK(d2h(c, h.data(), k ? c->coo.ref.get() : c->coo.alt.get(), m * 2));
        for (uint64_t i = 0; i < m; i++) dst[i] = h[i];
    }
    return CELLECTOR_OK;
}

// ---- merging a second staged matrix in ---------------------------------------------------------------------
cellector_status cellector_combine(cellector_ctx *c, const cellector_ctx *src, const uint8_t *src_keep, const uint32_t *locus_map,
                                   uint64_t total_loci_out, double downsample_rate, uint64_t seed)
{
    if (!c) return CELLECTOR_EINVAL;
    if (!src) return ctx_fail(c, CELLECTOR_EINVAL, "combine: src is NULL");
    if (c == src) return ctx_fail(c, CELLECTOR_EINVAL, "combine: ctx and src are the same ctx");
    if (const char *why = restage_scope(c)) return ctx_fail(c, CELLECTOR_EINVAL, "combine: ctx %s", why);
    if (const char *why = restage_scope(src)) return ctx_fail(c, CELLECTOR_EINVAL, "combine: src %s", why);
    if (c->device != src->device)
        return ctx_fail(c, CELLECTOR_EINVAL, "combine: ctx is on device %d, src on device %d", c->device, src->device);
    uint64_t T = 0;
    CHK(thin_threshold(c, "combine", downsample_rate, &T));
    const uint64_t n_ctx = c->total_cells, tc_src = src->total_cells, tl_src = src->total_loci;
    uint64_t n_kept = tc_src;
    if (src_keep) {
        n_kept = 0;
        for (uint64_t i = 0; i < tc_src; i++) n_kept += src_keep[i] != 0;
    }
    if (n_kept == 0) return ctx_fail(c, CELLECTOR_EINVAL, "combine: the selection keeps none of src's %llu cells", (unsigned long long)tc_src);
    if (total_loci_out < c->total_loci)
        return ctx_fail(c, CELLECTOR_EINVAL, "combine: total_loci_out %llu is below ctx's total_loci %llu", (unsigned long long)total_loci_out,
                        (unsigned long long)c->total_loci);
    if (total_loci_out > 0xffffffffull)
        return ctx_fail(c, CELLECTOR_EINVAL, "combine: total_loci_out %llu exceeds 32-bit indices", (unsigned long long)total_loci_out);
    if (locus_map) {
        for (uint64_t j = 0; j < tl_src; j++)
            if (locus_map[j] >= total_loci_out)
                return ctx_fail(c, CELLECTOR_EINVAL, "combine: locus_map[%llu] = %u is not below total_loci_out %llu", (unsigned long long)j,
                                locus_map[j], (unsigned long long)total_loci_out);
    } else if (tl_src > total_loci_out) {
        return ctx_fail(c, CELLECTOR_EINVAL, "combine: without a locus_map src's total_loci %llu must not exceed total_loci_out %llu",
                        (unsigned long long)tl_src, (unsigned long long)total_loci_out);
    }
    if (n_ctx + n_kept > 0xffffffffull)
        return ctx_fail(c, CELLECTOR_EINVAL, "combine: %llu + %llu cells exceed 32-bit indices", (unsigned long long)n_ctx,
                        (unsigned long long)n_kept);
    if (c->n_combines >= 255) return ctx_fail(c, CELLECTOR_EINVAL, "combine: 255 combines since the last ingest from outside (cell_source is a byte)");
    const uint64_t need_p1 = (uint64_t)P1_PLANES * total_loci_out;
    if (c->pass1_bound && c->pass1_bound_cap < need_p1)
        return ctx_fail(c, CELLECTOR_EINVAL, "combine: the bound PASS1 exchange buffer holds %llu values, total_loci_out %llu needs %llu",
                        (unsigned long long)c->pass1_bound_cap, (unsigned long long)total_loci_out, (unsigned long long)need_p1);
    SETDEV(c);
    CallLaps lap{"combine"};
    HIPCHK(c, hipStreamSynchronize(src->stream));  // (src is only read from here on, on ctx's stream)
    // ---- validated: from here ctx changes.  The built matrix goes before src's side is made (its blocks serve the selection)
    unbuild_matrix(c, lap);
    StagedCoo sel;
    DevBuf<uint32_t> src_origin;
    {
        // src's side: the selection and the draw are cellector_restage's, on src's arrays; then the renumbering
        std::vector<uint8_t> all;
        if (!src_keep) { all.assign(tc_src, 1); src_keep = all.data(); }
        DevBuf<uint8_t> keep01;
        DevBuf<uint32_t> rank, d_map;
        CHK(restage_cell_ranks(c, src_keep, tc_src, n_kept, src->cell_origin, &keep01, &rank, &src_origin));
        lap("cell ranks");
        CHK(restage_select(c, src->coo.view(), tc_src, keep01, rank, T, seed, &sel));
        lap("select src");
        if (locus_map) {
            CHK(dev_alloc(c, &d_map, tl_src));
            HIPCHK(c, hipMemcpyAsync(d_map, locus_map, tl_src * 4, hipMemcpyHostToDevice, c->stream));
        }
        CHK(combine_map(c, &sel, locus_map ? d_map.get() : nullptr, tl_src, (uint32_t)n_ctx));
        HIPCHK(c, hipStreamSynchronize(c->stream));  // (d_map and the host map are read)
        lap("map");
    }
    return staged_append(c, lap, &sel, src_origin, n_kept, total_loci_out, true);
}

// ---- synthetic doublets from resident cells -----------------------------------------------------------------
cellector_status cellector_add_doublets(cellector_ctx *c, const uint32_t *cell_a, const uint32_t *cell_b, uint64_t n_pairs,
                                        double downsample_rate, uint64_t seed)
{
    if (!c) return CELLECTOR_EINVAL;
    if (const char *why = restage_scope(c)) return ctx_fail(c, CELLECTOR_EINVAL, "add_doublets: ctx %s", why);
    if (n_pairs == 0) return ctx_fail(c, CELLECTOR_EINVAL, "add_doublets: no pairs");
    if (!cell_a || !cell_b) return ctx_fail(c, CELLECTOR_EINVAL, "add_doublets: %s is NULL", cell_a ? "cell_b" : "cell_a");
    uint64_t T = 0;
    CHK(thin_threshold(c, "add_doublets", downsample_rate, &T));
    const uint64_t n_ctx = c->total_cells;
    if (n_ctx + n_pairs > 0xffffffffull || n_ctx + n_pairs < n_ctx)
        return ctx_fail(c, CELLECTOR_EINVAL, "add_doublets: %llu + %llu cells exceed 32-bit indices", (unsigned long long)n_ctx,
                        (unsigned long long)n_pairs);
    for (uint64_t j = 0; j < n_pairs; j++) {
        if (cell_a[j] >= n_ctx || cell_b[j] >= n_ctx)
            return ctx_fail(c, CELLECTOR_EINVAL, "add_doublets: pair %llu (%u, %u) names a cell that is not below total_cells %llu",
                            (unsigned long long)j, cell_a[j], cell_b[j], (unsigned long long)n_ctx);
        if (cell_a[j] == cell_b[j])
            return ctx_fail(c, CELLECTOR_EINVAL, "add_doublets: pair %llu names cell %u twice", (unsigned long long)j, cell_a[j]);
    }
    if (c->n_combines >= 255)
        return ctx_fail(c, CELLECTOR_EINVAL, "add_doublets: 255 combines since the last ingest from outside (cell_source is a byte)");
    SETDEV(c);
    CallLaps lap{"add_doublets"};
    // ---- the doublet side, beside a built matrix that stays: a sum above CELLECTOR_MAX_COUNT is known only now and must leave
    // the ctx as it was
    StagedCoo dbl;
    DevBuf<uint32_t> dbl_origin;
    {
        // the fan table: cell c is side s of pair j for the values 2 j + s of fan_val[fan_ptr[c] .. fan_ptr[c + 1])
        std::vector<uint64_t> fan_ptr(n_ctx + 1, 0), fan_val(2 * n_pairs);
        for (uint64_t j = 0; j < n_pairs; j++) { fan_ptr[cell_a[j] + 1]++; fan_ptr[cell_b[j] + 1]++; }
        for (uint64_t i = 0; i < n_ctx; i++) fan_ptr[i + 1] += fan_ptr[i];
        {
            std::vector<uint64_t> at(fan_ptr.begin(), fan_ptr.end() - 1);
            for (uint64_t j = 0; j < n_pairs; j++) { fan_val[at[cell_a[j]]++] = 2 * j; fan_val[at[cell_b[j]]++] = 2 * j + 1; }
        }
        bool overflow = false;
        uint64_t over_pair = 0;
        uint32_t over_locus = 0;
        int over_allele = 0;
        CHK(doublets_build(c, c->coo.view(), n_ctx, c->total_loci, fan_ptr.data(), fan_val.data(), fan_val.size(), T, seed, &dbl, &overflow,
                           &over_pair, &over_locus, &over_allele));
        if (overflow)
            return ctx_fail(c, CELLECTOR_EINVAL, "add_doublets: pair %llu (%u, %u): the summed %s count at locus %u exceeds %u",
                            (unsigned long long)over_pair, over_pair < n_pairs ? cell_a[over_pair] : 0u,
                            over_pair < n_pairs ? cell_b[over_pair] : 0u, over_allele ? "alt" : "ref", over_locus, CELLECTOR_MAX_COUNT);
        CHK(doublets_origin(c, cell_a, n_pairs, n_ctx, c->cell_origin, &dbl_origin));
        lap("doublet side");
    }
    // ---- validated: from here ctx changes
    return staged_append(c, lap, &dbl, dbl_origin, n_pairs, c->total_loci, false);
}

// ---- the staged matrix as mtx text -------------------------------------------------------------------------------------
// what both calls check: the ctx (cellector_restage's scope), the mode, the flags
static cellector_status write_scope(const cellector_ctx *c, const char *call, int mode, uint32_t flags)
{
    if (c->multi) return ctx_fail(c, CELLECTOR_EINVAL, "%s works on a single-device ctx: the staged entries of a multi-device ctx are sharded", call);
    if (const char *why = restage_scope(c)) return ctx_fail(c, CELLECTOR_EINVAL, "%s: ctx %s", call, why);
    if (mode != CELLECTOR_WRITE_ALIGNED && mode != CELLECTOR_WRITE_SPARSE && mode != CELLECTOR_WRITE_DEPTH)
        return ctx_fail(c, CELLECTOR_EINVAL, "%s: mode %d is none of CELLECTOR_WRITE_ALIGNED, _SPARSE, _DEPTH", call, mode);
    if (flags & ~(CELLECTOR_MTX_SPACE | CELLECTOR_MTX_HEADER_ZERO))
        return ctx_fail(c, CELLECTOR_EINVAL, "%s: flags 0x%x hold a bit that is neither CELLECTOR_MTX_SPACE nor CELLECTOR_MTX_HEADER_ZERO", call, flags);
    return CELLECTOR_OK;
}

cellector_status cellector_write_mtx(cellector_ctx *c, const char *first_path, const char *second_path, int mode, uint32_t flags,
                                     cellector_write_summary *summary)
{
    if (!c) return CELLECTOR_EINVAL;
    CHK(write_scope(c, "write_mtx", mode, flags));
    if (!first_path || !second_path) return ctx_fail(c, CELLECTOR_EINVAL, "write_mtx: %s is NULL", first_path ? "second_path" : "first_path");
    if (!strcmp(first_path, second_path)) return ctx_fail(c, CELLECTOR_EINVAL, "write_mtx: both files are %s", first_path);
    SETDEV(c);
    return mtx_write_pair(c, first_path, second_path, mode, flags, summary);
}

cellector_status cellector_format_mtx(cellector_ctx *c, int which, int mode, uint32_t flags, uint64_t first_entry, uint64_t n_entries,
                                      uint8_t *out, uint64_t capacity, uint64_t *n_bytes, uint64_t *n_lines)
{
    if (!c) return CELLECTOR_EINVAL;
    CHK(write_scope(c, "format_mtx", mode, flags));
    if (which != 0 && which != 1) return ctx_fail(c, CELLECTOR_EINVAL, "format_mtx: which %d is neither 0 (first file) nor 1 (second)", which);
    if (first_entry > c->coo.n || n_entries > c->coo.n - first_entry)
        return ctx_fail(c, CELLECTOR_EINVAL, "format_mtx: entries [%llu, %llu + %llu) reach beyond the %llu staged", (unsigned long long)first_entry,
                        (unsigned long long)first_entry, (unsigned long long)n_entries, (unsigned long long)c->coo.n);
    SETDEV(c);
    uint64_t bytes = 0, lines = 0;
    const cellector_status st = mtx_format_range(c, which, mode, (flags & CELLECTOR_MTX_SPACE) ? ' ' : '\t', first_entry, n_entries, out, capacity,
                                                 &bytes, &lines);
    if (n_bytes) *n_bytes = bytes;  // (also when the capacity was too small)
    if (n_lines) *n_lines = lines;
    return st;
}

// ---- ... and as .mtx.gz: BGZF made on the device (kernels_bgzf.hip) ------------------------------------------------------
cellector_status cellector_write_mtx_bgzf(cellector_ctx *c, const char *first_path, const char *second_path, int mode, uint32_t flags,
                                          cellector_write_bgzf_summary *summary)
{
    if (!c) return CELLECTOR_EINVAL;
    CHK(write_scope(c, "write_mtx_bgzf", mode, flags));
    if (!first_path || !second_path)
        return ctx_fail(c, CELLECTOR_EINVAL, "write_mtx_bgzf: %s is NULL", first_path ? "second_path" : "first_path");
    if (!strcmp(first_path, second_path)) return ctx_fail(c, CELLECTOR_EINVAL, "write_mtx_bgzf: both files are %s", first_path);
    SETDEV(c);
    cellector_write_bgzf_summary gz = {};
    CHK(mtx_write_pair(c, first_path, second_path, mode, flags, nullptr, &gz));
    if (summary) *summary = gz;
    return CELLECTOR_OK;
}

cellector_status cellector_bgzf_compress(cellector_ctx *c, const uint8_t *in, uint64_t n, uint8_t *out, uint64_t capacity, uint64_t *n_out,
                                         uint64_t *n_blocks)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return ctx_fail(c, CELLECTOR_EINVAL, "bgzf_compress works on a single-device ctx: a multi-device root ctx has no device of its own");
    if (n && !in) return ctx_fail(c, CELLECTOR_EINVAL, "bgzf_compress: in is NULL for %llu bytes", (unsigned long long)n);
    SETDEV(c);
    uint64_t bytes = 0, blocks = 0;
    const cellector_status st = bgzf_compress_host(c, in, n, out, capacity, &bytes, &blocks);
    if (n_out) *n_out = bytes;  // (also when the capacity was too small)
    if (n_blocks) *n_blocks = blocks;
    return st;
}

cellector_status cellector_bgzf_decompress(cellector_ctx *c, const uint8_t *in, uint64_t n, uint8_t *out, uint64_t capacity, uint64_t *n_out,
                                           uint64_t *n_blocks)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return ctx_fail(c, CELLECTOR_EINVAL, "bgzf_decompress works on a single-device ctx: a multi-device root ctx has no device of its own");
    if (n && !in) return ctx_fail(c, CELLECTOR_EINVAL, "bgzf_decompress: in is NULL for %llu bytes", (unsigned long long)n);
    SETDEV(c);
    uint64_t bytes = 0, blocks = 0;
    const cellector_status st = bgzf_decompress_host(c, in, n, out, capacity, &bytes, &blocks);
    if (n_out) *n_out = bytes;  // (also when the capacity was too small)
    if (n_blocks) *n_blocks = blocks;
    return st;
}

}  // extern "C"
