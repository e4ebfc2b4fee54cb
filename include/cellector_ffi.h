/*
 * cellector_ffi.h — C ABI of libcellector_hip.so: the MI355X (gfx950) implementation of
 * cellector's genotype-likelihood / EM scoring path.
 *
 * The reference (wheaton5/cellector, Rust, single-threaded CPU) has no FFI of its own; the seams
 * below are the reference's own function boundaries, so a Rust host replaces each call with one
 * `extern "C"` call (binding shown in INTEGRATION.md).  Citations are file:line under
 * /root/reference/cellector/src/.
 *
 * Conventions
 *  - every function returns a cellector_status and never throws or aborts across the boundary;
 *    cellector_last_error(ctx) gives the message (the reference panics -> stderr + exit 101);
 *  - plain pointers and sizes only; host output buffers are caller-allocated and caller-owned;
 *  - a ctx owns all device memory, is bound to one GPU, and is driven by one host thread at a time;
 *  - a ctx holds ONE SHARD of the matrix: the cells [cell_begin, cell_end) of the global cell
 *    range, all loci.  Per-locus state is replicated on every shard.  Multi-GPU: either ONE ctx over
 *    several devices (cellector_create_multi) or one process per GPU with a communicator attached to
 *    its ctx (cellector_comm_init_rank) — in both the library runs the three exchanges itself over
 *    RCCL/xGMI; or, without a communicator, the host sums the three exchange buffers below at the
 *    marked points (cellector_set_shard + bind_exchange_buffer: e.g. torch.distributed tensors).  With
 *    a single shard nothing is exchanged and cellector_em_iteration() runs the phases back to back;
 *  - every kernel is launched on the ctx's stream (default: the null stream).
 */
#ifndef CELLECTOR_FFI_H
#define CELLECTOR_FFI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cellector_ctx cellector_ctx;

typedef enum {
    CELLECTOR_OK = 0,
    CELLECTOR_EINVAL = 1,  /* bad argument / call out of order            */
    CELLECTOR_EIO = 2,     /* cannot open/read a file (reader, load_data.rs:240-251) */
    CELLECTOR_EPARSE = 3,  /* malformed mtx text (read_mtx_lines, load_data.rs:190-204) */
    CELLECTOR_ENOMEM = 4,
    CELLECTOR_EDEVICE = 5, /* HIP runtime error                            */
    CELLECTOR_ECOMM = 6
} cellector_status;

/* ---- lifecycle ----------------------------------------------------------------------------- */
cellector_status cellector_create(cellector_ctx **out, int device_id);
void cellector_destroy(cellector_ctx *ctx);
/* number of visible GPUs (0 without one; never fails the process) */
cellector_status cellector_device_count(int *out);

/* ---- multi-GPU (the reference is ONE binary, main.rs:25-50: the host sees one logical matrix) ---------------
 * (1) One process, several GPUs.  The ctx owns one shard per listed device (rank r = the r-th of n equal contiguous
 *     cell ranges; per-locus state replicated), one host thread and one stream per shard, and an RCCL communicator
 *     over the devices (ncclCommInitAll).  EVERY entry point below works on it unchanged — ingest, cellector_em_iteration,
 *     outputs, posteriors, final tallies — and returns arrays in GLOBAL cell order; the three exchanges (PASS1 at load,
 *     NORM all-gather and LOCUS all-reduce per iteration) run inside the library over xGMI.  Not available on it:
 *     cellector_set_stream / set_shard / bind_exchange_buffer / em_begin|threshold|finish (internal) and
 *     cellector_write_staged_mtx.  n_devices == 1 gives a plain ctx.  A device listed more than once gives logical
 *     shards on that GPU, exchanged by device-side sums instead of RCCL (which refuses duplicate devices): the same
 *     sharded code path on a one-GPU box (tests, rehearsals).  At most 16 shards. */
cellector_status cellector_create_multi(cellector_ctx **out, const int *device_ids, int n_devices);
/* (2) One process per GPU (torch.distributed / MPI launchers).  Rank 0 makes an id, the host broadcasts its 128 bytes by
 *     whatever means it has, every rank attaches a communicator to its own single-device ctx BEFORE the ingest.  The ctx
 *     then owns rank r's cell range and performs the exchanges itself: cellector_ingest_finish all-reduces PASS1,
 *     cellector_em_threshold first all-gathers NORM, cellector_em_finish first all-reduces LOCUS (so cellector_em_iteration
 *     is the whole distributed iteration); per-cell outputs are this rank's cells.  CELLECTOR_ECOMM on RCCL failures. */
cellector_status cellector_comm_unique_id(void *out_128_bytes);
cellector_status cellector_comm_init_rank(cellector_ctx *ctx, const void *unique_id_128_bytes, int n_ranks, int rank);
const char *cellector_last_error(const cellector_ctx *ctx); /* ctx-owned, valid until next call */
const char *cellector_version(void);
/* hipStream_t to launch on (e.g. torch.cuda.current_stream().cuda_stream); NULL = null stream. */
cellector_status cellector_set_stream(cellector_ctx *ctx, void *hip_stream);
/* Options: "compute_expected" (default 1: also accumulate expected_log_beta_binomial_pmf,
 * stats.rs:8-33, into expected_ll like the reference; 0 = skip that diagnostic column),
 * "timing" (default 0; 1: record HIP events around every timed group of kernels; 2: only around
 * the engine's dominant kernel — each event pair idles the queue for a few microseconds; 3: ... around every
 * fourth launch of it only),
 * "keep_coo" (default 1: keep the staged all-loci COO for cellector_final_allele_tallies),
 * "engine" (default 2: table-driven passes over the tiled 16-bit layout; 1: CSR/CSC kernels that
 * evaluate every entry's log-pmf — same results within rounding, kept for A/B checks; choose it before the
 * ingest: an engine-2 ingest releases the packed by-locus CSC that only engine 1 streams),
 * "compact_bits" (default 0: the locus pass stores 24-bit entries when the shard has <= 2^20 cells,
 * else 32-bit; 32 forces the wide form — set before ingest),
 * "locus_mode" (engine 2, default 0: per iteration the device picks how the per-locus minority counts
 * of get_locus_log_likelihoods, main.rs:368-420, are formed — 2 = walk only the excluded cells' rows,
 * 1 = stream the whole compact CSC past the exclusion bitmask; bit-identical results; these are the forms of a recount),
 * "tally_delta" (engine 2, default 1: those counts are kept from one iteration to the next and updated with the cells
 * whose exclusion changed — nothing to count once the set stops moving; the device recounts the whole set when the change
 * is larger than the new set, and after a reload or an engine switch; 0 = recount every iteration; bit-identical — A/B),
 * "class_delta" (engines 1 and 2, default 1: cellector_refine_classes updates the per-class tallies between two steps from the
 * rows of the cells that moved, and recounts when more cells moved than a recount would walk; 0 = recount every step;
 * the same integers either way — A/B),
 * "overlap" (engine 2, default 1: the kernels of the few entries with alt+ref = 0 or > 4 run on a side
 * stream beside the table-lookup kernel; 2 = their locus-side part only after that kernel; 0 = everything
 * in one stream; same results to the bit),
 * "side_lds" (engine 2, default -1: automatic residency throttle of the side-stream kernels),
 * "ovf_deep" (engine 2, default -1: per matrix — when more than 3 % of the entries have alt+ref = 0 or > 4 (deep coverage)
 * their per-cell sums come from ONE unthrottled kernel that takes totals up to 17; 0 / 1 force either form; results agree
 * within rounding: the summation order inside a cell's overflow entries differs; "ovf_deep_wide", default 1: that kernel
 * gives 16 lanes to a row, 0 = a thread per row — A/B),
 * "tile_groups" (engine 2, default 0: the number of locus-chunk groups of the tile kernel is chosen per matrix;
 * 1..64 forces it — set before ingest; results may differ in the last bit),
 * "tile_sb" (engine 2, default 0: the tile kernel takes columns of 4 cell blocks, or of 2 when 4 would leave CUs idle, chosen
 * per launch; 2 or 4 forces the width — tests; read per launch, same results to the bit; other values: CELLECTOR_EINVAL),
 * "parse_window" (default 0: a text file of 1 GB or more is uploaded and tokenised in 256 MB windows, a smaller
 * one whole; a positive value forces windows of that many bytes — tests; lines of a windowed file may be 1 MB long),
 * "gz_device" (default 0: a ".gz" input is inflated on the host before the ingest; 1: cellector_ingest_mtx / cellector_load_mtx
 * and cellector_ingest_mtx_joined / cellector_load_mtx_joined on a single-device ctx leave a BGZF ".gz" compressed, upload the
 * compressed bytes and inflate them on the device — cellector_amd/csrc/kernels_inflate.hip, whole or window by window as
 * "parse_window" says.  Each file of the pair decides for itself: a plain file, a plain-gzip ".gz" and a file that
 * CELLECTOR_NO_BGZF covers go the way they go with 0.  Every call stages exactly what it stages with 0; a member the device
 * refuses hands the file back to the host reader, so a pair that fails with 0 fails with 1 with the same status (the error then
 * names the file, the member and the reason; a file the host reader accepts after all is announced on stderr).  The split
 * ingest of a multi-device ctx ignores the option.  Other values: CELLECTOR_EINVAL.  CELLECTOR_TIMING=1 prints one more line
 * per file: members, bytes in and out, the inflate kernel's GPU time),
 * "write_window" (default 0: cellector_write_mtx and cellector_format_mtx take the staged entries through windows of 2^23
 * entries; a positive value forces windows of that many entries — tests; the bytes written do not depend on it),
 * "synth_continue_pct" (default 30: cellector_ingest_synthetic draws an entry's total as 1 + Geometric(0.7), vartrix-like
 * shallow coverage; a larger value gives deeper counts, e.g. 60 = 1 + Geometric(0.4) — benchmarks of the count distribution),
 * "norm_zero" (default 1: a shard clears the other shards' slices of CELLECTOR_XCHG_NORM before it writes
 * its own, so that a SUM all-reduce completes the array; 0 when the caller all-gathers the slices),
 * "sharded_select" (1: a ctx with a communicator — cellector_create_multi, cellector_comm_init_rank — finds the
 * median / quartiles by a radix select over the shards' own keys, exchanging digit histograms: six all-reduces of 48 KB per
 * iteration; 0: every shard's normalised LLs are all-gathered and every shard selects over all of them; default -1: the
 * histograms for runs of 4 Mi cells and more on three or more ranks, else the gather; same bits either way),
 * "balance" (multi-device ctx, default 1: see cellector_set_partition), "ref_arith" (engine 1: every entry with the
 * reference's own ln_gamma arithmetic, stats.rs:41-53, instead of the exact product form), "t2" / "t2_waves" (engine 2:
 * the entries with totals 5..8 through per-(locus, pair) tables, default on unless the matrix has deep coverage),
 * "t2_helper" (engine 2: blocks of the tier-2 lookup kernel's helper grid per compute unit the tile grid leaves free;
 * -1 = automatic, 0 = none, n = forced; placement only, the results do not depend on it),
 * "t2_cache" (engine 2, default -1: the EM pass keeps every tier-2 entry's looked-up values and gathers again only at loci whose
 * (alpha, beta) bits differ from those the kept values were written under — nothing once the exclusion set stands still;
 * 1 = on, 0 = off, -1 = automatic; 16 bytes per overflow slot of device memory; same bits either way),
 * "t2_fill" (with t2_cache: what a pass does at the loci that moved, 1 = gather and keep, 0 = gather without keeping,
 * default -1 = the device decides per pass from how many loci moved since the pass before; same bits either way — A/B, tests),
 * "bank_order" (engine 2, default 1: the tile builder orders every row's entries and the rows of a slice against LDS bank
 * conflicts; 0 keeps file order, the layout whose per-cell sums do not depend on which cells share a shard),
 * "t2_tiles" (engine 2, deep coverage: the cell side of the totals 5..8 (8, the default of a matrix with more than 3 % of
 * its entries outside 1..4), or 5..6 (6), walks a second tile set with chunk tables in LDS; 0: evaluated entry by entry),
 * "resolve_ties" (engines 1 and 2, single-device ctx only, default 0 = off: 1 = inside cellector_em_threshold, the cells
 * whose normalised LL lies within 2 * band * max(1, |v|) of one of the six order statistics v behind the median and the
 * quartiles, and then of the threshold, are evaluated again with the reference's own arithmetic — its ln_gamma
 * differences, the C library's log and the file order of the cell's entries — and their LL and normalised LL replaced:
 * median, iqr, threshold and the exclusion flags are then the reference's bits (band: see n_near_threshold);
 * 2 = every cell is evaluated so (diagnostic: checks the band argument).  Set it before the ingest: the ingest then keeps
 * every cell's entries in file order as well (8 more bytes per entry), the order the reference adds a cell's terms in; set
 * after an ingest without it, 1 and 2 are refused.  A multi-device ctx or one with a communicator of more than one rank
 * refuses 1 and 2 with CELLECTOR_EINVAL, and so does a host whose C library log is not the one the device repeats
 * (glibc >= 2.28, FMA variant: checked on a few arguments).  Off: no launches, no allocations.
 * See cellector_iter_resolution),
 * "resolve_posteriors" (engines 1 and 2, single-device ctx only, default 0 = off; read by cellector_assign alone): 1 = the
 * cells whose label or qual could differ between the device's posterior-phase values and the reference's — those next to
 * p = T, 1 - p = T, doublet = 0.5, an integer qual or the saturation of p — get their three per-cell LLs in the
 * reference's arithmetic (its ln_gamma differences, the C library's log, all used loci, the file order of the cell's
 * entries) and the logsumexp chain, label and qual from the host's C library: labels and quals are then the reference's, and
 * the evaluated cells' posterior, doublet posterior and LLs are its bits; 2 = every cell is evaluated so (the whole output
 * is the reference's bits; the check of mode 1's band).  Needs the file-order copy like resolve_ties: set it before the
 * ingest (either of the two options being non-zero at the ingest keeps it); 1 / 2 after an ingest without it, other values,
 * a multi-device ctx, a communicator of more than one rank or a host with another C library log are refused with
 * CELLECTOR_EINVAL.  cellector_posteriors is not changed by it.  Off: no launches, no allocations.
 * See cellector_assign_resolution),
 * "cell_variance" (engines 1 and 2, default 0: 1 = every cell pass of the loop, cellector_em_begin, is followed by a pass over
 * the by-cell CSR that forms expected_log_variances, the fourth vector of get_cell_log_likelihoods (main.rs:587):
 * cellector_iter_cell_variances.  No other output changes.  Off, with normalization 0: no launches, no allocations),
 * "normalization" (default 0 = log_likelihood / loci_used, main.rs:316, the form the reference runs; 1 = the z-score its
 * author left beside it, main.rs:317-318: (log_likelihood - expected_log_likelihood) / sqrt(expected_log_variance), 0 for a
 * cell without used loci (main.rs:320-322) and for one whose variance is 0; other values: CELLECTOR_EINVAL.  1 implies the
 * variance pass.  The z-scores are then the keys of the median, the quartiles, the threshold, the exclusion flags and
 * n_near_threshold, and the `normalized` column of cellector_iter_cell_outputs.  Read by cellector_em_begin; works on
 * single-device, multi-device and communicator ctxs and on a cellector_set_shard ctx whose host drives the exchanges (the
 * NORM slice holds per-cell keys either way).  Refused with CELLECTOR_EINVAL, in whichever order the options are set:
 * normalization 1 together with resolve_ties 1 / 2 (the reference has no arithmetic of this mode to resolve to) and
 * normalization 1 together with compute_expected 0 (the z-score needs the expected term); resolve_posteriors is
 * independent.  n_near_threshold keeps its formula in this mode but has no reference counterpart there: no reference run
 * scores by these keys.  interquartile_range_multiple's default of 5 was chosen for the per-locus scale, not for this one),
 * "locus_moments" (engines 1 and 2, default 0: 1 = cellector_em_threshold, behind its locus pass, also forms the per-locus
 * expected contribution and variance of the new exclusion set and of the rest, under the alpha/beta and mask of the iteration's
 * cell pass: cellector_iter_locus_moments.  No other output changes; independent of compute_expected, ref_arith,
 * resolve_ties, resolve_posteriors, cell_variance and normalization.  A single-device ctx that holds all cells: 1 is refused
 * with CELLECTOR_EINVAL on a multi-device ctx, with a communicator of more than one rank and with a cellector_set_shard
 * range, whichever is set first.  Off: no launches, no allocations). */
cellector_status cellector_set_option(cellector_ctx *ctx, const char *key, int64_t value);

/* ---- sharding (before ingest) --------------------------------------------------------------- */
/* This ctx owns global cells [cell_begin, cell_end).  Default: all cells. */
cellector_status cellector_set_shard(cellector_ctx *ctx, uint64_t cell_begin, uint64_t cell_end);
/* A ctx with a communicator (cellector_create_multi, cellector_comm_init_rank) shards the cells itself: rank r owns
 * [bounds[r], bounds[r+1]).  Default: n equal contiguous ranges — except that the text / COO ingest of a multi-device ctx
 * cuts the ranges so that every shard holds about the same number of ENTRIES (option "balance", default 1): the reference's
 * per-cell lists (load_data.rs:151-174) differ in length by orders of magnitude on real data, and the slowest shard sets
 * the iteration.  cellector_set_partition gives the ranges explicitly (n_ranks + 1 non-decreasing boundaries from 0 to
 * total_cells, the same array on every rank, before the ingest; NULL / 0 = back to the default); cellector_partition
 * reads the ranges in use back (bounds_out may be NULL to ask for the number of ranks only). */
cellector_status cellector_set_partition(cellector_ctx *ctx, const uint64_t *bounds, int n_bounds);
cellector_status cellector_partition(const cellector_ctx *ctx, uint64_t *bounds_out /*[n_ranks + 1]*/, int *n_ranks);

/* ---- ingest: replaces load_cell_data (load_data.rs:134-181) + get_loci_used (:254-280) ------- */
/* Phase 1 — stage this shard's entries on the device and count, per locus, cells with ref>0 /
 * alt>0 (pass 1, load_data.rs:265-270) and the allele totals into CELLECTOR_XCHG_PASS1. */
cellector_status cellector_ingest_mtx(cellector_ctx *ctx, const char *alt_path, const char *ref_path);
/* Caller COO in file order, 0-based indices (any order; locus-major like vartrix is fastest). */
cellector_status cellector_ingest_coo(cellector_ctx *ctx, uint64_t total_loci, uint64_t total_cells,
                                      uint64_t nnz, const uint32_t *locus0, const uint32_t *cell0,
                                      const uint32_t *alt, const uint32_t *ref);
/* Deterministic synthetic vartrix-like matrix generated on the device (benchmarks; definition in
 * DESIGN.md / cellector_amd/synth.py, which produces bit-identical host data). */
cellector_status cellector_ingest_synthetic(cellector_ctx *ctx, uint64_t total_loci,
                                            uint64_t total_cells, double density, uint64_t seed,
                                            double minority_fraction, double doublet_fraction);
/* Benchmark utility, not a reference seam: writes the staged matrix (any ingest, option keep_coo=1)
 * as a vartrix-style alt.mtx / ref.mtx text pair (3-line header, `locus cell count`, 1-based, file
 * order), formatted on the device — BASELINE-sized inputs for the text path in seconds. */
cellector_status cellector_write_staged_mtx(cellector_ctx *ctx, const char *alt_path, const char *ref_path);
/* >>> multi-shard: all-reduce CELLECTOR_XCHG_PASS1 here <<< */
/* Phase 2 — locus filter `cells_ref >= min_ref && cells_alt >= min_alt` (load_data.rs:273),
 * compaction, CSR (by cell) + CSC (by locus) build on the device (pass 2, load_data.rs:151-174). */
cellector_status cellector_ingest_finish(cellector_ctx *ctx, uint64_t min_alt, uint64_t min_ref);
/* Single-shard conveniences = ingest + finish. */
cellector_status cellector_load_mtx(cellector_ctx *ctx, const char *alt_path, const char *ref_path,
                                    uint64_t min_alt, uint64_t min_ref);
cellector_status cellector_load_coo(cellector_ctx *ctx, uint64_t total_loci, uint64_t total_cells,
                                    uint64_t nnz, const uint32_t *locus0, const uint32_t *cell0,
                                    const uint32_t *alt, const uint32_t *ref, uint64_t min_alt,
                                    uint64_t min_ref);

/* ---- joined ingest: two count matrices keyed by (locus, cell) instead of zipped line by line -----------------
 * cellector_ingest_mtx reads the pair like the reference's izip! (load_data.rs:190-197): line i of the ref file belongs to line i
 * of the alt file and the ref file's indices are never read.  A pair whose files do not list the same keys in the same order —
 * zero lines dropped, filtered or sorted by another tool — or an alt-depth / total-depth pair (AD / DP, each file listing its
 * own non-zero keys) cannot be read that way.  The joined ingests take two streams of (locus, cell, count), FIRST and SECOND,
 * each in ANY order, and stage their join.  Opt-in: the aligned ingests do not change.
 *   Dims: both size lines must give the same total_loci and total_cells (CELLECTOR_EINVAL otherwise; the COO form takes them as
 *   arguments).
 *   mode CELLECTOR_JOIN_REF: SECOND holds ref counts.  One entry per distinct (locus, cell) that occurs in either stream;
 *   alt = FIRST's count there or 0, ref = SECOND's count there or 0.
 *   mode CELLECTOR_JOIN_DEPTH: SECOND holds alt + ref.  The same keys, the same alt; ref = depth - alt, an absent depth counting
 *   as 0.  A key with depth < alt is refused.
 *   Order: the staged COO ascends STRICTLY by (locus, cell), whatever order either stream had, and is locus-major.
 *   Zeros: a line with an explicit count 0 is a key like any other, so a (0, 0) entry exists only if a stream lists it.
 *   Equality with the aligned reader: the result is, array for array, what cellector_ingest_mtx stages from the COMPLETED pair:
 *   both files rewritten over the union of their keys in ascending order, with explicit zeros (mode DEPTH: the second one
 *   holding depth - alt).  cellector_amd/join.py is the bit-identical numpy twin.
 *   Refusals, each naming the smallest offender of its kind, checked in this order:
 *     1. a line that does not parse, in FIRST, then in SECOND (every line of a file counts: no file is cut at the other one's
 *        length): CELLECTOR_EPARSE, the aligned reader's words behind "FIRST file: " / "SECOND file: ";
 *     2. index 0 (text), a locus or cell out of range, a count above 65535, in FIRST, then in SECOND: CELLECTOR_EINVAL,
 *        "join: FIRST entry <i>: <what>", i the 0-based position in the stream, the words those of cellector_ingest_mtx;
 *     3. a key listed twice within one stream, FIRST, then SECOND: CELLECTOR_EINVAL, "join: SECOND lists (locus l, cell c)
 *        twice", 1-based, the smallest such key.  (The aligned reader keeps repeated lines as separate entries; a join cannot
 *        know which line of the other stream belongs to which.);
 *     4. mode DEPTH: CELLECTOR_EINVAL, "join: depth below alt at (locus l, cell c)", 1-based, the smallest such key.
 *   A refusal leaves the ctx as a failed cellector_ingest_mtx leaves it: the former matrix dropped, nothing staged.
 *   Scope, as cellector_restage: a single-device ctx without a communicator of more than one rank and without a
 *   cellector_set_shard range, engines 1 and 2; anything else is CELLECTOR_EINVAL with the ctx untouched, as are a mode other
 *   than the two, size lines that disagree and a file that cannot be opened.  Option keep_coo is honoured as by any ingest,
 *   option parse_window as by cellector_ingest_mtx (each file is windowed exactly when that call would window it).
 *   Afterwards the ctx is STAGED; cellector_ingest_finish follows unchanged.
 *   Memory: the tokens of both streams (12 B per entry; 20 B while a side's keys are formed) and 8 B + 4 B per entry of a side
 *   that has to be sorted, beside the staged COO (12 B per distinct key); the tokens are released as soon as the COO is written.
 *   The pre-mapping thread of the aligned text ingest is left out of this route: it is sized for token arrays that become the
 *   COO, and here the COO's size is known only after the join's first pass.
 *   CELLECTOR_TIMING=1 prints one line with the phases: tokens FIRST, tokens SECOND, checks, sorts, join (and the join
 *   kernels' GPU time between two events). */
#define CELLECTOR_JOIN_REF 1
#define CELLECTOR_JOIN_DEPTH 2
typedef struct {
    uint64_t n_first, n_second;   /* entries read                                                             */
    uint64_t n_both, n_first_only, n_second_only, n_out; /* keys in both / one stream; n_out = their sum       */
    uint32_t first_sorted, second_sorted; /* 1: the stream arrived strictly ascending, no sort ran            */
    uint32_t join_tile;           /* steps through the two streams one block of the join kernels walks; it    */
                                  /* writes at most join_tile + 1 entries                                     */
    uint32_t reserved;
} cellector_join_summary;
cellector_status cellector_ingest_mtx_joined(cellector_ctx *ctx, const char *first_path, const char *second_path, int mode,
                                             cellector_join_summary *out /*may be NULL*/);
cellector_status cellector_load_mtx_joined(cellector_ctx *ctx, const char *first_path, const char *second_path, int mode,
                                           uint64_t min_alt, uint64_t min_ref, cellector_join_summary *out /*may be NULL*/);
/* two caller COO streams, 0-based indices, any order (what a caller holding two sparse matrices has) */
cellector_status cellector_ingest_coo_joined(cellector_ctx *ctx, uint64_t total_loci, uint64_t total_cells, uint64_t n_first,
                                             const uint32_t *locus0_a, const uint32_t *cell0_a, const uint32_t *count_a,
                                             uint64_t n_second, const uint32_t *locus0_b, const uint32_t *cell0_b,
                                             const uint32_t *count_b, int mode, cellector_join_summary *out /*may be NULL*/);

typedef struct {
    uint64_t total_cells, total_loci; /* header dims (consume_mtx_header, load_data.rs:206-223) */
    uint64_t loci_used;               /* L = loci passing the filter                            */
    uint64_t cell_begin, cell_end;    /* this shard                                             */
    uint64_t nnz_used;                /* this shard's entries at used loci                      */
} cellector_dims_t;
cellector_status cellector_dims(const cellector_ctx *ctx, cellector_dims_t *out);
cellector_status cellector_locus_ids(const cellector_ctx *ctx, uint64_t *out /*[L]*/);
/* locus_counts of load_cell_data: out[2l] = sum ref, out[2l+1] = sum alt (load_data.rs:157-158) */
cellector_status cellector_locus_counts(const cellector_ctx *ctx, double *out /*[2L]*/);
/* cell.cell_loci_data.len() for the min_loci_for_assignment rule (main.rs:153) */
cellector_status cellector_entries_per_cell(const cellector_ctx *ctx, uint32_t *out /*[local cells]*/);
/* CSR rows of local cells [row_begin,row_end): row_ptr rebased to 0, entries packed
 * locus_index | alt << 32 | ref << 48 (diagnostics, tests, CPU-baseline sampling). */
cellector_status cellector_csr_rows(const cellector_ctx *ctx, uint64_t row_begin, uint64_t row_end,
                                    uint64_t *row_ptr /*[rows+1]*/, uint64_t *entries, uint64_t capacity);

/* ---- re-staging the resident matrix: a cell subset and per-read downsampling without the files ---------
 * The reference's cell set is whatever load_barcodes read (load_data.rs `load_barcodes`): dropping cells — the peel of the cells
 * called minority, a doublet or empty-droplet list, a barcode whitelist — means rewriting barcodes.tsv and both matrices and
 * loading again.  Its companion `combiner` samples cells (select_cells, combiner/src/main.rs:246-255; a barcode mask,
 * main.rs:257-280) and thins the reads (main.rs:83-88 and main.rs:102-107), again from files into files.  cellector_restage does both on
 * the staged COO the ctx still holds.
 *   keep: [total_cells] of the matrix now staged, non-zero = keep, NULL = all cells.  Kept cells are renumbered in ascending
 *   order of their old index; an entry survives iff its cell is kept, the survivors keep their relative order; a kept cell
 *   without entries stays as an empty row.
 *   downsample_rate: the probability that a read is REMOVED (the combiner's --downsample_rate), in [0, 1].  For the entry at
 *   position i of the staged arrays the call reads (before the compaction), allele a (0 = ref, 1 = alt, the order of
 *   main.rs:83-88) and read r = 0..count-1:  x = mix64(mix64((seed * GOLD) ^ ((i + 1) * GOLD)) + (2 r + a + 1) * GOLD), the read
 *   is removed iff (x >> 11) < (uint64_t)(downsample_rate * 2^53); mix64 = the splitmix64 finaliser, GOLD = 0x9E3779B97F4A7C15
 *   (the synthetic generator's).  All-integer: cellector_amd/restage.py is the bit-identical numpy twin.  Rate 0 draws nothing
 *   and copies the counts, rate 1 leaves every count 0.  An entry whose two counts both reach 0 STAYS, as the combiner writes it.
 *   The draw is keyed by position: it does not depend on keep, the launch grid or the engine.
 *   Staged order is file order.  For an input that was not locus-major it is, after a finished ingest, the stable sort by locus
 *   the ingest made: a restage before and after cellector_ingest_finish then draws differently — for such an input and only
 *   for such an input — and the order options resolve_ties / resolve_posteriors then call "file order" is the sorted one.
 * Afterwards the ctx is the one cellector_ingest_coo would have left for the restaged entries: state STAGED, total_cells = the
 * number of kept cells, total_loci unchanged, PASS1 formed again from the new entries, everything the former matrix owned
 * dropped exactly as a reload drops it (caller-bound NORM / LOCUS buffers are unbound, the iteration state is gone), options
 * keep their values.  The caller then calls cellector_ingest_finish(min_alt, min_ref): the locus filter, L, locus_counts, the
 * layouts, the near-tie band and the file-order copy of the resolve options are those of the restaged matrix.
 * keep == NULL with rate 0 is legal: the same entries, staged again — the way back from a loaded matrix to another min_alt.
 *   Allowed in state STAGED (after cellector_ingest_*) always, and on a loaded matrix when it kept its staged COO (option
 *   keep_coo 1 at the ingest) and no iteration is in flight.  A single-device ctx without a communicator that holds all cells.
 *   CELLECTOR_EINVAL with a message, the ctx untouched: a multi-device ctx, a communicator of more than one rank, a
 *   cellector_set_shard range, no staged matrix, a loaded matrix without its COO, a call between cellector_em_begin and
 *   cellector_em_finish, a rate outside [0, 1] or NaN, a selection of zero cells.
 *   Memory: after validation the built matrix is dropped FIRST, then the new COO is allocated beside the old one (peak: both
 *   COOs, 12 B per entry each, plus 18 B per cell and 8 B per 4096 entries) and the old one released.  On CELLECTOR_ENOMEM
 *   the ctx is left STAGED holding the OLD entries and dims, ready for cellector_ingest_finish.  With keep == NULL (or every
 *   cell kept) nothing is allocated: the counts are thinned where they are. */
cellector_status cellector_restage(cellector_ctx *ctx, const uint8_t *keep, double downsample_rate, uint64_t seed);
/* per current cell, its index in the matrix of the last ingest from outside (mtx / coo / synthetic); identity after such an
 * ingest; composed over repeated restages */
cellector_status cellector_cell_origin(const cellector_ctx *ctx, uint32_t *out /*[total_cells]*/);
/* diagnostic like cellector_csr_rows: the staged entries in staged order; all four arrays NULL = count only */
cellector_status cellector_staged_coo(const cellector_ctx *ctx, uint64_t *n, uint32_t *locus0, uint32_t *cell0,
                                      uint32_t *alt, uint32_t *ref, uint64_t capacity);

/* ---- merging a second staged matrix in: the other half of the reference's `combiner` ---------------------
 * The combiner takes a second dataset, renumbers its loci into the first one's numbering (get_locus_mapping,
 * combiner/src/main.rs:197-231), puts its cells behind the first one's (main.rs:161-186) and writes everything in the order of
 * lines.sort() (main.rs:111), from files into files.  cellector_combine does that between two ctxs on one GPU: the entries of
 * `src`'s staged COO join those of `ctx`; `src` is only read and is left exactly as it was, including a matrix it has built.
 *   src_keep: [src total_cells], non-zero = take the cell, NULL = all.  downsample_rate / seed: src's reads only.  Selection and
 *   thinning are exactly cellector_restage's — renumbering by ascending old index, the same all-integer draw — keyed by the
 *   position i in SRC's staged arrays before the selection: restage.restage_coo on src's arrays is the twin of this step.  The
 *   caller thins ctx's own reads beforehand with cellector_restage(ctx, NULL, rate, seed).
 *   locus_map: [src total_loci], src's 0-based locus -> the 0-based locus of the result, NULL = identity.  It need not be
 *   monotone or injective (two src loci may fold into one).  combine.locus_map_from_vcfs builds the combiner's map.
 *   A surviving src entry (l, c, alt, ref) becomes (locus_map[l], n_ctx + rank(c), alt, ref), n_ctx = ctx's total_cells before
 *   the call; ctx's own entries keep their indices.  total_cells becomes n_ctx + n_kept, total_loci becomes total_loci_out.
 *   Staged order afterwards: ALL entries ascending by (locus, cell, ref, alt), the combiner's sort on the tuple it pushes.  The
 *   order is unique: it depends neither on the order either side was staged in nor on the grid.  (The two sides' cell ranges
 *   are disjoint: each side is taken as it stands when its (locus, cell) pairs ascend strictly — every vartrix file, the
 *   synthetic generator and any restage of either — and sorted by the tuple otherwise; the sides are then merged by
 *   (locus, cell).)  The staged COO is locus-major afterwards.
 *   cellector_cell_origin of a new cell is SRC's cell_origin of the cell it came from; ctx's cells keep theirs.
 *   cellector_cell_source is 0 for every cell after an ingest from outside; a cell brought in by the k-th combine since that
 *   ingest gets k, ctx's cells keep theirs, the values src's cells had in src are not carried over.  cellector_restage composes
 *   the source the way it composes the origin; an ingest from outside clears it and the combine count.
 * Afterwards, as after a restage: state STAGED, PASS1 formed again from all entries, everything the former matrix of ctx owned
 * dropped as a reload drops it, options keep their values; cellector_ingest_finish follows.
 *   Both ctxs: single-device, on the same GPU, without a communicator or a cellector_set_shard range, holding a staged COO
 *   (state STAGED, or a loaded matrix that kept it: option keep_coo 1), not between cellector_em_begin and cellector_em_finish.
 *   CELLECTOR_EINVAL with a message (on ctx), BOTH ctxs untouched: ctx == src, different devices, a multi-device, communicator
 *   or sharded ctx on either side, no staged COO on either side, an iteration in flight on either side, a rate outside [0, 1]
 *   or NaN, a selection of zero cells, total_loci_out below ctx's total_loci or above 2^32 - 1, a map value >= total_loci_out
 *   (the message names the first one), a NULL map with src's total_loci > total_loci_out, n_ctx + n_kept > 2^32 - 1, more than
 *   255 combines since the last ingest from outside, a caller-bound PASS1 buffer smaller than 5 * total_loci_out (the
 *   size it was bound with counts, not what the last ingest used of it).
 *   Memory: after validation ctx's built matrix is dropped FIRST, then everything new is allocated beside ctx's entries: the
 *   selected src entries (12 B each) and the merged COO (12 B per entry of the result), so the peak is 24 B per ctx entry and
 *   24 B per selected src entry, plus 5 B per cell of the result, 18 B per src cell, 8 B per 4096 src entries and per 2048
 *   entries of the result; a side that has to be sorted adds 32 B per entry of that side (and the radix sort's scratch) while it is sorted, 12 B after.  On
 *   CELLECTOR_ENOMEM ctx is left STAGED holding its OLD entries, dims, origin and source, ready for cellector_ingest_finish. */
cellector_status cellector_combine(cellector_ctx *ctx, const cellector_ctx *src,
                                   const uint8_t *src_keep /*[src total_cells] or NULL = all*/,
                                   const uint32_t *locus_map /*[src total_loci] or NULL = identity*/,
                                   uint64_t total_loci_out, double downsample_rate, uint64_t seed);
/* per current cell: 0 = from the last ingest from outside, k = brought in by the k-th cellector_combine (or
 * cellector_add_doublets, which counts as one) since */
cellector_status cellector_cell_source(const cellector_ctx *ctx, uint8_t *out /*[total_cells]*/);

/* ---- synthetic doublets from resident cells: what the combiner announces and never does -------------------
 * combiner/src/main.rs:43 reads "decide which cells are doublets and that mapping", and nothing follows it.  A synthetic
 * doublet is two droplets' reads in one barcode: cellector_add_doublets appends, for j = 0..n_pairs-1, a cell n_ctx + j
 * (n_ctx = total_cells before the call) that holds at every locus the SUM of the counts of cell_a[j] and cell_b[j], so that
 * the doublet posterior (calculate_posteriors, main.rs:239-276) can be exercised on a real matrix at a chosen depth.
 *   Entries: for every locus at which cell_a[j] or cell_b[j] has at least one staged entry the new cell gets exactly ONE
 *   entry; its alt is the sum of the (thinned) alt of ALL entries of both parents at that locus — repeated (locus, cell) lines
 *   of a parent all count — its ref likewise.  An entry whose two sums are 0 STAYS, as in restage and combine.  A locus
 *   neither parent has gives no entry; a parent with an empty row adds nothing; two empty parents give an empty row.  The
 *   parents' own entries are never changed.  The same pair listed twice is legal: two cells with independent draws.
 *   downsample_rate: the probability that a parent's read is REMOVED on its way into the doublet, in [0, 1].  For the parent
 *   entry at position i of ctx's staged arrays as the call reads them, pair j, side s (0 = cell_a, 1 = cell_b), allele a
 *   (0 = ref, 1 = alt) and read r = 0..count-1:
 *     h = mix64(mix64((seed * GOLD) ^ ((i + 1) * GOLD)) ^ ((2 j + s + 1) * GOLD)),  x = mix64(h + (2 r + a + 1) * GOLD),
 *   the read is removed iff (x >> 11) < (uint64_t)(downsample_rate * 2^53); mix64 and GOLD are cellector_restage's, in
 *   uint64 wrap-around arithmetic.  The draw is independent per (pair, side), also where one cell is a parent in many pairs.
 *   All-integer: cellector_amd/doublets.py is the bit-identical numpy twin.  Rate 0 draws nothing, rate 1 leaves every
 *   doublet count 0.
 *   Staged order is file order.  For an input that was not locus-major it is, after a finished ingest, the stable sort by locus
 *   the ingest made: a call before and after cellector_ingest_finish then draws differently — for such an input and only
 *   for such an input (the caveat of cellector_restage, verbatim).
 *   Staged order afterwards: ALL entries ascending by (locus, cell, ref, alt), exactly as after cellector_combine: ctx's side is
 *   taken as it stands if its (locus, cell) pairs ascend strictly and sorted by the tuple otherwise, the doublet side ascends
 *   strictly by construction, the cell ranges are disjoint and the two are merged by (locus, cell).  The result is unique: it
 *   depends neither on the grid nor on the order of equal keys in the intermediate sort (integer sums commute).
 *   total_cells becomes n_ctx + n_pairs, total_loci is unchanged.  cellector_cell_origin of a new cell is that of cell_a[j].
 *   The call counts as a combine in the numbering of cellector_cell_source: new cells get n_combines + 1, ctx's cells keep
 *   theirs; cellector_restage composes both as it does today.  The caller keeps the pair list.
 * Afterwards, as after restage and combine: state STAGED, PASS1 formed again from all entries, everything the built matrix owned
 * dropped as a reload drops it, options keep their values; cellector_ingest_finish follows.
 *   The ctx: single-device, without a communicator or a cellector_set_shard range, holding a staged COO (state STAGED, or a
 *   loaded matrix that kept it: option keep_coo 1), not between cellector_em_begin and cellector_em_finish.
 *   CELLECTOR_EINVAL with a message, the ctx untouched (still READY with its built matrix if it had one): any of those
 *   conditions, n_pairs == 0, a NULL list, an index >= n_ctx (the message names the first such pair), cell_a[j] == cell_b[j]
 *   (the message names the pair), a rate outside [0, 1] or NaN, n_ctx + n_pairs > 2^32 - 1, more than 255 combines since the
 *   last ingest from outside, a summed count above 65535 (the message names pair, locus and allele of the first such entry in
 *   output order; ref before alt inside one entry).
 *   Memory: the doublet side is built FIRST, beside a built matrix that stays, so that the last refusal leaves the ctx as it
 *   was: 16 B per cell of ctx and per pair for the fan table, 8 B per 2048 ctx entries, then per emitted record (one per parent
 *   entry and pair it is in) 24 B and the radix sort's scratch while the records are sorted, 20 B while they are summed, plus
 *   20 B per doublet entry; 12 B per doublet entry remain.  Then the built matrix is dropped and the merged COO (12 B per entry
 *   of the result) is allocated beside ctx's entries and the doublet side: the peak there is 24 B per ctx entry and per doublet
 *   entry, plus 5 B per cell of the result and 8 B per 2048 entries of the result; a ctx side that has to be sorted adds 32 B per
 *   entry (and the radix sort's scratch) while it is sorted, 12 B after.  On CELLECTOR_ENOMEM before the drop the ctx is
 *   untouched; after it the ctx is left STAGED holding its OLD entries, dims, origin and source, ready for
 *   cellector_ingest_finish. */
cellector_status cellector_add_doublets(cellector_ctx *ctx, const uint32_t *cell_a /*[n_pairs]*/, const uint32_t *cell_b /*[n_pairs]*/,
                                        uint64_t n_pairs, double downsample_rate, uint64_t seed);

/* ---- the staged matrix as mtx text, made on the device: the way out for what the calls above make ------------------
 * The reference's `combiner` is a program that writes files (combiner/src/main.rs:52-116: alt.mtx, ref.mtx, barcodes.tsv, gt.tsv).
 * A matrix made on the device — a peel, a titration mixture, planted doublets, a downsampled copy, an AD / DP pair joined into
 * alt / ref — leaves it through cellector_write_mtx as the text every tool of the field reads and the library's own three readers
 * read back.  No format is invented here.  The lines are rendered by kernels (integers to decimal text, a byte-exact compaction
 * into a stream); cellector_amd/mtx_write.py is the byte-identical numpy twin.
 *   File layout: "%%MatrixMarket matrix coordinate real general\n% written by sprs\n", then `total_loci SEP total_cells SEP count\n`,
 *   then one line `locus0+1 SEP cell0+1 SEP value\n` per entry that is written, entries in STAGED order.  Numbers are plain decimal
 *   without sign, padding or exponent; the last byte of a file is '\n'.  SEP is '\t', or ' ' with CELLECTOR_MTX_SPACE (sprs /
 *   vartrix); count is the number of body lines of the file, or 0 with CELLECTOR_MTX_HEADER_ZERO.  Tabs + HEADER_ZERO + mode ALIGNED
 *   are the combiner's bytes (main.rs:67-69, :113-114).
 *   mode CELLECTOR_WRITE_ALIGNED: both files hold one line per staged entry, zeros explicit: alt in the first, ref in the second
 *   (read by cellector_ingest_mtx).  mode CELLECTOR_WRITE_SPARSE: the first file holds the entries with alt > 0, the second those
 *   with ref > 0 (read by CELLECTOR_JOIN_REF).  mode CELLECTOR_WRITE_DEPTH: the first holds alt where alt > 0, the second alt + ref
 *   where alt + ref > 0 (read by CELLECTOR_JOIN_DEPTH).
 *   Index arithmetic: index + 1 is formed in 64 bits (index 2^32 - 1 is written 4294967296); alt + ref of DEPTH reaches 131070.
 *   Dropped keys: n_dropped_keys counts the entries with alt = ref = 0 in every mode.  The combiner keeps them and ALIGNED writes
 *   them; under SPARSE and DEPTH they are in neither file, so a read-back lacks exactly those keys.
 *   Allowed where cellector_restage is: state STAGED, or a loaded matrix that kept its staged COO (option keep_coo 1) with no
 *   iteration in flight; a single-device ctx that holds all cells.  The calls only read the ctx: the staged COO, the built matrix,
 *   the EM state and every option are unchanged afterwards.
 *   CELLECTOR_EINVAL with a message: a multi-device ctx, a communicator of more than one rank, a cellector_set_shard range, no
 *   staged matrix, a loaded matrix without its COO, a call between cellector_em_begin and cellector_em_finish, an unknown mode or
 *   flag bit, `which` outside 0 / 1, a range that reaches beyond the staged entries, a capacity below n_bytes (n_bytes and n_lines
 *   are still returned), the two paths equal or NULL.
 *   CELLECTOR_EIO when a file cannot be created, written or closed.  A failed call leaves what it has written and REMOVES NOTHING:
 *   it never unlinks a path (a caller may pass a device node).  The first file is complete before the second is created.
 *   Windows: the entries go through windows of option "write_window" entries (default 0 = 2^23; a positive value forces that many —
 *   tests, like parse_window for the reader).  A window is formatted into one of two device buffers; while it is copied to pinned
 *   host memory on a second stream and then written by a host thread, the next one is formatted into the other buffer.  The bytes
 *   of a file depend neither on the window nor on the grid nor on the order the flags are or-ed in.  n_windows = the windows per
 *   file, ceil(n_entries / window).  Under SPARSE / DEPTH without HEADER_ZERO the count of the size line needs a length pass over
 *   all windows before the first byte is written.
 *   Memory: per call two device and two pinned host buffers of 29 B (the longest line) per entry of a window, 8 B per 1024.
 *   CELLECTOR_TIMING=1 prints one line: the host's time in formatting (and the two kernels' GPU time between events, summed over
 *   the windows; the format kernel is then awaited), waiting for copies, waiting for writes.
 * cellector_format_mtx: the body lines (no header) of the staged entries [first_entry, first_entry + n_entries) of file `which`
 * (0 / 1) to host memory; out == NULL: n_bytes and n_lines only.  No byte of out outside [0, n_bytes) is written. */
#define CELLECTOR_WRITE_ALIGNED 0
#define CELLECTOR_WRITE_SPARSE 1
#define CELLECTOR_WRITE_DEPTH 2
#define CELLECTOR_MTX_SPACE 1u
#define CELLECTOR_MTX_HEADER_ZERO 2u
typedef struct {
    uint64_t n_entries;                  /* staged entries                                                */
    uint64_t lines_first, lines_second;  /* body lines of the two files                                   */
    uint64_t bytes_first, bytes_second;  /* their sizes, header included                                  */
    uint64_t n_dropped_keys;             /* entries with alt = ref = 0                                    */
    uint64_t n_windows;                  /* windows per file                                              */
} cellector_write_summary;
cellector_status cellector_write_mtx(cellector_ctx *ctx, const char *first_path, const char *second_path, int mode, uint32_t flags,
                                     cellector_write_summary *summary /*may be NULL*/);
cellector_status cellector_format_mtx(cellector_ctx *ctx, int which, int mode, uint32_t flags, uint64_t first_entry, uint64_t n_entries,
                                      uint8_t *out, uint64_t capacity, uint64_t *n_bytes, uint64_t *n_lines);

/* ---- the same text as .mtx.gz, compressed block-wise on the device -------------------------------------------------
 * The field ships matrices as .mtx.gz, and cellector_write_mtx is bound by write(2), not by its kernels.  cellector_write_mtx_bgzf
 * writes the SAME text as BGZF (block-compressed gzip, what `bgzip` writes): independent gzip members of at most 64 KB, each with
 * its own CRC-32 and size field, then the 28-byte EOF member.  zcat, gzip -t, Python's gzip, htslib, the reference's
 * MultiGzDecoder (load_data.rs:246) and this library's own block-parallel reader (cellector_ingest_mtx and the joins take the
 * paths as they are) read it.  No format is invented.
 *   The stream: the text is cut at multiples of 32640 bytes; every piece is one member (18-byte BGZF header, one deflate block with
 *   BFINAL = 1, CRC-32, ISIZE).  The deflate block uses a PRESET Huffman table sent in the block (BTYPE = 10, the same bits in every
 *   block), and its only matches are against the same column of the line before: (length, distance = the length of that line), in
 *   pieces of at most 258 bytes; everything is defined inside a block.  A block the preset does not make smaller than len + 5 bytes
 *   is a stored block (BTYPE = 00).  cellector_amd/bgzf.py states the format and is the byte-identical numpy twin;
 *   cellector_amd/csrc/bgzf_format.h is its C form.  The bytes depend neither on the grid nor on any option.
 * cellector_bgzf_compress: n host bytes as their BGZF stream in host memory, compressed on the ctx's device; any ctx with a device
 *   of its own will do (state EMPTY included; a multi-device root ctx is refused).  n_out receives the stream's size (EOF member
 *   included), n_blocks its data blocks; out == NULL: those only.  CELLECTOR_EINVAL when capacity < n_out: the sizes are still
 *   returned and not a byte of out is written.  No byte of out outside [0, n_out) is written.  The ctx is only used for its device
 *   and stream: nothing of its state changes.
 * cellector_write_mtx_bgzf: the arguments, modes, flags, scope and refusals of cellector_write_mtx; each file equals the BGZF
 *   stream (cellector_bgzf_compress, bgzf.compress) of the file cellector_write_mtx would have written, the three header lines
 *   included.  Blocks are cut in the FILE's text, not in a window's: what a window leaves behind its last whole block is carried
 *   to the next on the device, so the files do not depend on "write_window".  summary->text is what cellector_write_mtx reports
 *   (sizes of the TEXT); file_bytes_* are the sizes of the files, blocks_* their data blocks, stored_blocks those of both files
 *   that are stored.  Memory: the text buffers of cellector_write_mtx once more on the device (one aligned, one with the carry), the
 *   members' slots, and pinned buffers of the compressed worst case.  CELLECTOR_TIMING=1 prints cellector_write_mtx's line and
 *   one more: blocks, bytes in and out, the two compress kernels' GPU time.
 * cellector_bgzf_decompress: the mirror of cellector_bgzf_compress, with its scope and its two-call sizing: the n host bytes of a BGZF
 *   stream as their text in host memory, inflated on the ctx's device (cellector_amd/csrc/inflate_format.h, kernels_inflate.hip: one
 *   wave per member).  Any BGZF stream will do, bgzip's and this library's alike: gzip members that carry the 'BC' size field, whole,
 *   of at most 64 KB of text each, stored, fixed and dynamic blocks, any number per member.  n_out receives the size of the text,
 *   n_blocks the members (EOF member and other empty ones included); out == NULL: those only.  CELLECTOR_EINVAL when
 *   capacity < n_out: the sizes are still returned and not a byte of out is written.  No byte of out outside [0, n_out) is ever
 *   written.  CELLECTOR_EPARSE when `in` is no such stream (plain gzip, a member cut short, ISIZE above 65536).  A member is refused
 *   exactly when zlib's inflate of its body fails or leaves input unused, or its length is not ISIZE, or its CRC-32 not the
 *   trailer's: CELLECTOR_EIO, and cellector_last_error names the smallest refused member of the launch by its index in the stream
 *   and says why; out may then hold the text of members before it.  The members go through the device in launches of 2048
 *   (CELLECTOR_INFLATE_CHUNK in the environment: fewer, for tests), so device memory does not grow with n.  The ctx is only used
 *   for its device and stream: nothing of its state changes.  CELLECTOR_TIMING=1 prints members, bytes in and out and the
 *   kernel's GPU time. */
typedef struct {
    cellector_write_summary text;                  /* what cellector_write_mtx reports for the same arguments */
    uint64_t file_bytes_first, file_bytes_second;  /* sizes of the two files, EOF member included              */
    uint64_t blocks_first, blocks_second;          /* their data blocks                                       */
    uint64_t stored_blocks;                        /* blocks of both files that are stored                    */
} cellector_write_bgzf_summary;
cellector_status cellector_bgzf_compress(cellector_ctx *ctx, const uint8_t *in, uint64_t n, uint8_t *out, uint64_t capacity,
                                         uint64_t *n_out, uint64_t *n_blocks);
cellector_status cellector_write_mtx_bgzf(cellector_ctx *ctx, const char *first_path, const char *second_path, int mode, uint32_t flags,
                                          cellector_write_bgzf_summary *summary /*may be NULL*/);
cellector_status cellector_bgzf_decompress(cellector_ctx *ctx, const uint8_t *in, uint64_t n, uint8_t *out, uint64_t capacity,
                                           uint64_t *n_out, uint64_t *n_blocks);

/* ---- exchange buffers (device memory, f64) --------------------------------------------------- */
typedef enum {
    CELLECTOR_XCHG_PASS1 = 0, /* [5*total_loci]: cells_ref | cells_alt | sum_ref | sum_alt | n_entries */
    CELLECTOR_XCHG_NORM = 1,  /* [total_cells]: normalised LL of every cell (own slice written, rest 0) */
    CELLECTOR_XCHG_LOCUS = 2  /* [5*L+8]: contrib_min | contrib_maj | cells_min | alt_min | ref_min |
                                 {n_new, n_rescued, n_excluded, ...}                               */
} cellector_xchg;
cellector_status cellector_exchange_buffer(cellector_ctx *ctx, cellector_xchg which, void **dev_ptr,
                                           uint64_t *n_f64);
/* Use caller-allocated device memory (e.g. a torch tensor) for an exchange buffer; must be called
 * before the buffer is first used (PASS1: after cellector_set_shard; NORM/LOCUS: after ingest_finish
 * sizes are known via cellector_exchange_buffer with dev_ptr == NULL). */
cellector_status cellector_bind_exchange_buffer(cellector_ctx *ctx, cellector_xchg which,
                                                void *dev_ptr, uint64_t n_f64);

/* ---- one EM iteration == compute_new_excluded (main.rs:308-347) ------------------------------ */
typedef struct {
    int32_t any_change;                /* main.rs:335                                            */
    uint64_t n_new_excluded, n_rescued; /* main.rs:333-334                                       */
    uint64_t n_excluded;               /* |new exclusion set| over all shards                    */
    uint64_t n_loci_filtered;          /* loci newly masked by the -80 filter (main.rs:444-447)  */
    double median, iqr, threshold;     /* main.rs:325-329                                        */
    /* Not in the reference: cells (all shards) with |normalised LL - threshold| <= band * max(1, |threshold|),
     * band = max(1e-9, 8 * 2^-52 * lgamma(max over the used loci of S_alt + S_ref + 2)).
     * The device evaluates log_beta_binomial_pmf as an exact product ratio; the reference's ln_gamma differences
     * (stats.rs:41-53) carry ~2^-52 * lnGamma(alpha + beta) of cancellation error per term — 1e-11 on a normalised
     * LL at vartrix-like depth (alpha + beta ~ 1e4: the band is its 1e-9 floor), 1e-8 at alpha + beta ~ 1e6 — so such
     * a cell could fall on the other side of main.rs:330-332's strict `<` in the reference.  Non-zero = the
     * bit-identical-assignment claim does not cover those cells of this iteration.  host/cellector prints one
     * stderr warning.  (Option ref_arith, engine 1, evaluates the reference's own formula instead; option
     * resolve_ties resolves these cells: cellector_iter_resolution.) */
    uint64_t n_near_threshold;
} cellector_iter_summary;

/* phase A: init_alpha_betas (main.rs:598-611) from the previous exclusion set's tallies, then
 * get_cell_log_likelihoods (main.rs:541-591) over this shard's cells and the normalisation of
 * main.rs:314-323 into this shard's slice of CELLECTOR_XCHG_NORM. */
cellector_status cellector_em_begin(cellector_ctx *ctx);
/* >>> multi-shard: all-reduce CELLECTOR_XCHG_NORM here <<< */
/* phase B: exact median / R-8 quartiles over all cells (statrs Data, main.rs:324-327), threshold
 * (main.rs:328-329), new exclusion flags of this shard's cells (main.rs:330-332) and this shard's
 * part of get_locus_log_likelihoods (main.rs:368-420) into CELLECTOR_XCHG_LOCUS. */
cellector_status cellector_em_threshold(cellector_ctx *ctx, double iqr_multiple);
/* >>> multi-shard: all-reduce CELLECTOR_XCHG_LOCUS here <<< */
/* phase C: locus filter (main.rs:428-451), any_change, state swap. */
cellector_status cellector_em_finish(cellector_ctx *ctx, cellector_iter_summary *out);
/* single shard: A, B, C back to back */
cellector_status cellector_em_iteration(cellector_ctx *ctx, double iqr_multiple,
                                        cellector_iter_summary *out);

/* ---- placing the EM state ---------------------------------------------------------------------
 * The reference's loop state is (excluded_cells, loci_used): main.rs:37 starts it from `HashSet::new()` and
 * load_data.rs:176-179 from all loci used; main.rs:43 and :444-447 are the only places that move it.  The three calls below
 * put a ctx at a state of the caller's choosing without a reload: warm starts from a known partition (the reference's -g
 * ground truth, a souporcell clustering, an earlier run's assignments), another interquartile_range_multiple on the resident
 * matrix, checkpoint / restore.  Everything the ctx derives from the state (the per-locus minority tallies behind
 * cellector_alpha_betas and the posterior phase, the kept counts of option tally_delta, the per-cell counts of entries at
 * masked loci, tables built ahead) is formed again or dropped.
 * All three need a loaded matrix and no iteration in flight (not between cellector_em_begin and cellector_em_finish), else
 * CELLECTOR_EINVAL.  They work on a single-device ctx, on a multi-device ctx (global arrays, global cell order, like
 * cellector_assign) and on a ctx with a communicator (this rank's local cells, like cellector_excluded; every rank makes
 * the same call, the library reduces the tallies itself).  A cellector_set_shard ctx WITHOUT a communicator is refused with
 * CELLECTOR_EINVAL: the host drives its exchanges and there is no exchange point for the tally reduction.
 * cellector_iter_cell_outputs keeps returning the last iteration's per-cell values after set_excluded / set_loci_mask.
 * cellector_iter_locus_outputs reads the exchange buffer and the mask the calls write, so after a placement it no longer
 * shows the last iteration (and after cellector_em_reset it is refused until an iteration has finished):
 *   - after set_excluded: the placed set's minority / majority counts and allele tallies, both contribution columns 0 (no
 *     pass produced any); the minority cell count of a locus the CURRENT mask masks is 0;
 *   - after set_loci_mask: the columns that are 0 at a masked locus (majority count, the four allele tallies) follow the
 *     NEW mask, the contributions stay the last pass', and the minority cell count is NOT formed again: it stays 0 at a
 *     locus the old mask masked and the new one uses, and keeps its value at a locus the new mask masks.
 * So for a locus view of a placed state call set_loci_mask first, then set_excluded; the order matters to this one call
 * only (nothing else reads that count before the next locus pass rewrites it).  Copy the locus outputs before a placement
 * if the last iteration's are still wanted.
 * Failure: the calls validate and allocate before they write.  If the tally exchange of a communicator fails afterwards
 * (CELLECTOR_ECOMM), the ctx holds the new flags with unreduced tallies: call cellector_em_reset or place a set again. */
/* excluded_cells := {i : flags[i] != 0} — replaces main.rs:37's `HashSet::new()` / main.rs:43's assignment.  Afterwards the
 * ctx is the one whose last cellector_em_finish produced this set: cellector_excluded returns it, cellector_alpha_betas is
 * init_alpha_betas(set) (main.rs:598-611), cellector_posteriors / _assign / _final_allele_tallies use it, and the next
 * iteration is compute_new_excluded(excluded_cells = set) with n_new_excluded / n_rescued counted against it
 * (main.rs:333-334).  The tallies are recounted on the device from the set's rows with integer atomics: exact for any set. */
cellector_status cellector_set_excluded(cellector_ctx *ctx, const uint8_t *flags /*[local cells]*/);
/* loci_used := used (1 = used, as cellector_loci_mask returns it; the same array on every rank) — replaces the all-true
 * vector of load_data.rs:176-179 and the filter's writes (main.rs:444-447).  A masked locus leaves the per-cell sums
 * (main.rs:556) and still counts in the tallies and alpha/beta, exactly like a locus the loop's own -80 filter masked.
 * All-zero and all-one masks are legal (all-zero: every normalised LL is 0, main.rs:315-322). */
cellector_status cellector_set_loci_mask(cellector_ctx *ctx, const uint8_t *used /*[L]*/);
/* Back to the state cellector_ingest_finish left — empty exclusion set, all loci used, iteration 0, zeroed exchange and
 * output buffers — i.e. main.rs:37 and load_data.rs:176-179 again, on the resident matrix.  No layout is rebuilt; options
 * keep their values. */
cellector_status cellector_em_reset(cellector_ctx *ctx);

/* What option resolve_ties did in the last iteration (all zero when it was off, and on a multi-device ctx). */
typedef struct {
    uint64_t n_evaluated;      /* cells evaluated with the reference's arithmetic                                     */
    uint64_t n_flags_changed;  /* exclusion flags that differ from those the device keys and threshold alone give      */
    uint32_t changed;          /* bits that changed: 1 median, 2 iqr, 4 threshold                                    */
    uint32_t mode;             /* the option's value in that iteration (1 or 2; 0: nothing was resolved)              */
} cellector_resolution_t;
cellector_status cellector_iter_resolution(const cellector_ctx *ctx, cellector_resolution_t *out);
/* ... and which cells it evaluated: n_evaluated local cell indices (order unspecified); nothing when it was off. */
cellector_status cellector_iter_resolved_cells(const cellector_ctx *ctx, uint32_t *ids /*[n_evaluated]*/);

/* outputs of the last iteration (host buffers; any pointer may be NULL) */
cellector_status cellector_iter_cell_outputs(const cellector_ctx *ctx, double *ll, double *expected_ll,
                                             double *loci_used_per_cell,
                                             double *normalized /*[local cells] each*/);
/* LocusLogLikelihoodData (main.rs:516-525) after the exchange, global over all shards */
cellector_status cellector_iter_locus_outputs(const cellector_ctx *ctx, double *contrib_min,
                                              double *contrib_maj, uint64_t *cells_min,
                                              uint64_t *cells_maj, uint64_t *alt_min,
                                              uint64_t *ref_min, uint64_t *alt_maj,
                                              uint64_t *ref_maj /*[L] each*/);
cellector_status cellector_loci_mask(const cellector_ctx *ctx, uint8_t *out /*[L]*/);
cellector_status cellector_excluded(const cellector_ctx *ctx, uint8_t *out /*[local cells]*/);
/* alpha/beta that the NEXT em_begin will use = init_alpha_betas(current excluded), main.rs:598 */
cellector_status cellector_alpha_betas(const cellector_ctx *ctx, double *alpha, double *beta /*[L]*/);

/* get_cell_log_likelihoods (main.rs:541-591) alone under caller alpha/beta/mask (host arrays).  Engine 2 runs its tile pass
 * whatever the mask: the per-cell counts of entries at the CALL's masked loci are formed in scratch for the call, the ctx's
 * own mask and counts (the loop's, cellector_set_loci_mask's) are left as they are.  Engine 1 runs the CSR kernel. */
cellector_status cellector_cell_log_likelihoods(cellector_ctx *ctx, const double *alpha,
                                                const double *beta, const uint8_t *mask /*[L] or NULL*/,
                                                double *ll, double *expected_ll,
                                                double *loci_used_per_cell /*[local cells]*/);

/* ---- the per-entry records behind those sums ---------------------------------------------------
 * PMFData (main.rs:527-539) of the listed cells under caller alpha/beta/mask: what get_cell_log_likelihoods pushes into
 * all_pmfs (main.rs:556-575), i.e. one record per entry at a USED locus, none at a masked one.  The arguments are those of
 * cellector_cell_log_likelihoods plus a cell list.
 *   rec_ptr is required and always written: rec_ptr[0] = 0, rec_ptr[j + 1] - rec_ptr[j] = the records of cells[j].  With all
 *   six record pointers NULL the call only counts and capacity is ignored (the two-call pattern of cellector_csr_rows);
 *   otherwise capacity >= rec_ptr[n_cells], else CELLECTOR_EINVAL with rec_ptr still valid.  A column whose pointer is NULL
 *   is not computed.
 *   Order: cells in the order of the list (a cell listed twice gets its records twice); inside a cell the by-cell CSR's row
 *   order: ascending locus index, repeated (locus, cell) lines in file order.  For a locus-major (vartrix) file that is the
 *   order of cell_loci_data; for any other file it is NOT file order.
 *   The other PMFData fields are implied: cell_id by rec_ptr, alpha / beta = the caller's arrays at locus_index, locus =
 *   cellector_locus_ids at locus_index, excluded = cellector_excluded.
 *   Cell ids are local cell indices (global ones on a multi-device ctx, like cellector_assign; local ones on a ctx with a
 *   communicator or a cellector_set_shard range).  Every id is checked before anything is written or launched: one out of
 *   range gives CELLECTOR_EINVAL and the message names it.  n_cells == 0 is legal; an empty row or an all-masked mask gives
 *   zero records.
 *   Needs a loaded matrix and no iteration in flight; works on engines 1 and 2.  The call uses scratch of its own and leaves
 *   the ctx exactly as it was; it runs on the ctx's stream and returns when the arrays are written.  Device scratch is
 *   allocated for exactly the counted records; a list whose records do not fit fails with CELLECTOR_ENOMEM before the fill
 *   pass is launched.
 *   Values: log_pmf is the product form of the cell pass (it does not change with option ref_arith); expected_log_pmf is
 *   ln sum_k pmf(k)^2 (stats.rs:19-22) by the ratio recurrence (totals up to 17 from pmf(0), above anchored at the mode);
 *   expected_log_variance follows stats.rs:23-28 to the letter: sum_k pmf(k) (ln pmf(k) - expected_log_pmf)^2, centred on the
 *   expected term, not on a mean.  A term whose pmf underflows adds 0.  An entry with alt + ref == 0 gives 0, 0, 0. */
cellector_status cellector_cell_pmfs(cellector_ctx *ctx, const double *alpha, const double *beta /*[L]*/,
                                     const uint8_t *mask /*[L] or NULL = all used*/,
                                     const uint32_t *cells, uint64_t n_cells,
                                     uint64_t *rec_ptr /*[n_cells + 1]*/, uint64_t capacity,
                                     uint32_t *locus_index, uint32_t *alt, uint32_t *ref, double *log_pmf,
                                     double *expected_log_pmf, double *expected_log_variance /*[capacity] each, any may be NULL*/);

/* ---- the fourth per-cell vector: expected_log_variances -------------------------------------------
 * get_cell_log_likelihoods (main.rs:541-591) returns log_likelihoods, loci_used_per_cell, expected_log_likelihoods and
 * expected_log_variances (main.rs:561, :581, :587): per cell, the sum over its entries at used loci of the variance of
 * stats.rs:23-28, sum_k pmf(k) (ln pmf(k) - expected_log_pmf)^2 — the expected_log_variance column of cellector_cell_pmfs
 * summed per cell.  It is the denominator of the z-score of main.rs:316-318 (option normalization).
 *   Totals up to 17 come from a per-locus table of that column's bits; a lane of the cell's wave adds every 64th entry of the
 *   by-cell CSR row in row order and the 64 partial sums are folded pairwise, so a cell's value depends on its row alone: it
 *   is the same to the bit on any shard, on either engine and under either bank_order.
 * cellector_cell_log_variances: the vector alone under caller alpha/beta/mask (host arrays), the arguments of
 * cellector_cell_log_likelihoods.  Needs a loaded matrix and no iteration in flight; engines 1 and 2.  Unlike
 * cellector_cell_log_likelihoods it uses scratch of its own and leaves the ctx exactly as it was (alpha/beta, tables,
 * iteration outputs).  An all-masked mask gives zeros, and so does an empty row.  Global cell order on a multi-device ctx; the
 * local cells of a ctx with a communicator or a cellector_set_shard range. */
cellector_status cellector_cell_log_variances(cellector_ctx *ctx, const double *alpha, const double *beta /*[L]*/,
                                              const uint8_t *mask /*[L] or NULL = all used*/,
                                              double *expected_log_variance /*[local cells]*/);
/* ... of the last finished iteration, formed under that iteration's alpha/beta and mask (options cell_variance or
 * normalization).  CELLECTOR_EINVAL ("not formed") when that iteration ran with both options 0, before the first iteration
 * and after cellector_em_reset until an iteration has finished.  Global cell order on a multi-device ctx, like
 * cellector_iter_cell_outputs. */
cellector_status cellector_iter_cell_variances(const cellector_ctx *ctx, double *out /*[local cells]*/);

/* ---- locus moments: the per-locus expected log-likelihood and its variance --------------------------
 * get_locus_log_likelihoods (main.rs:368-420) declares locus_expected_contribution_minority / _majority and fills them with a
 * copy of log_pmf (main.rs:394).  These calls return what main.rs:398/404 would hold had line 394 pushed
 * pmf_data.expected_log_pmf, and the matching sums of expected_log_variance.  For a used locus l and a class of cells (min: the
 * flagged cells, maj: the rest), one term per entry of a cell of the class at l (a repeated (locus, cell) line counts as often
 * as it occurs), with n = alt + ref of the entry:
 *   exp_c[l] = sum E(alpha_l, beta_l, n)    E = expected_log_pmf, stats.rs:19-22
 *   var_c[l] = sum V(alpha_l, beta_l, n)    V = expected_log_variance, stats.rs:23-28
 * E and V are the values cellector_cell_pmfs returns in those two columns (the same device functions, the same bits).  A
 * masked locus gives 0 in all four (no PMFData exists there, main.rs:556); an entry with n = 0 adds 0.
 *   Evaluation, fixed so that the result depends on the matrix, the flags and alpha/beta alone (not on the engine, bank_order
 *   or the grid): per locus and class s = 0; for n = 1..17 ascending s = s + (double)count_c[l][n] * T[l][n], a rounded product
 *   and a rounded sum (no fused multiply-add); then the locus' entries with n > 17 in ascending local cell index, a repeated
 *   pair in CSR row order, each adding its own E (V).  count_maj = count_all - count_min, as integers.
 * cellector_locus_moments: under caller alpha/beta/mask/flags (host arrays), the locus-side counterpart of
 * cellector_cell_log_variances.  Scratch of its own; the ctx is left exactly as it was (it may build and keep the all-cells
 * histogram and the list of the entries above 17 of this matrix: cache, not state).  Needs a loaded matrix and no iteration in
 * flight; engines 1 and 2; a single-device ctx that holds all cells (else CELLECTOR_EINVAL, like option locus_moments), with
 * fewer than 2^32 entries (the histograms count in 32 bits; else CELLECTOR_EINVAL). */
cellector_status cellector_locus_moments(cellector_ctx *ctx, const double *alpha, const double *beta /*[L]*/,
                                         const uint8_t *mask /*[L] or NULL = all used*/, const uint8_t *flags /*[local cells]*/,
                                         double *exp_min, double *exp_maj, double *var_min,
                                         double *var_maj /*[L] each, any may be NULL*/);
/* the histogram itself, a diagnostic like cellector_csr_rows: out[l][n] = entries of the flagged cells (NULL: all cells) at
 * used locus l with alt + ref = n for n = 0..17, out[l][18] = their entries with a larger total.  Mask-independent. */
cellector_status cellector_locus_total_counts(cellector_ctx *ctx, const uint8_t *flags /*[local cells] or NULL = all cells*/,
                                              uint32_t *out /*[L][19]*/);
/* ... the four vectors of the last finished iteration (option locus_moments): under the alpha/beta its cell pass used, its
 * mask and its NEW exclusion set, the inputs of main.rs:343 (quirk Q9).  CELLECTOR_EINVAL ("not formed") when that iteration
 * ran with the option at 0, before the first iteration and after cellector_em_reset until an iteration has finished.  After
 * cellector_set_excluded / cellector_set_loci_mask it keeps returning the last iteration's, like cellector_iter_cell_outputs. */
cellector_status cellector_iter_locus_moments(const cellector_ctx *ctx, double *exp_min, double *exp_maj, double *var_min,
                                              double *var_maj /*[L] each, any may be NULL*/);

/* ---- calculate_posteriors (main.rs:228-280) with the current exclusion set -------------------- */
/* the three distributions of calculate_posteriors for the current exclusion set (main.rs:239-254):
 * which = 0 minority, 1 majority (scaled by max(minority_fraction, 0.01)), 2 doublet.  With cellector_cell_pmfs they give the
 * per-locus log-likelihood ratio behind a cell's posterior.  Formed in scratch: the ctx is left as it was. */
cellector_status cellector_posterior_alpha_betas(cellector_ctx *ctx, int which, double *alpha, double *beta /*[L]*/);
cellector_status cellector_posteriors(cellector_ctx *ctx, double *posterior, double *doublet_posterior,
                                      double *ll_majority, double *ll_minority /*[local cells]*/);

/* calculate_posteriors (main.rs:228-280) + the rule of output_final_assignments (main.rs:141-171) in one call.
 * Any output pointer may be NULL.  codes: 0 "0", 1 "1", 2 "doublet", 3 "unassigned"; anomaly 0 = in the exclusion set;
 * qual = min(-10 log10(1 - max(p, 1 - p)), 255) as usize.  With option resolve_posteriors 0 this is cellector_posteriors plus
 * the rule on the device's values (also on a multi-device ctx, global cell order); with 1 / 2 the evaluated cells' four values,
 * label and qual replace the device's (see the option). */
cellector_status cellector_assign(cellector_ctx *ctx, double posterior_threshold, uint64_t min_loci_used,
                                  double *posterior, double *doublet_posterior, double *ll_majority, double *ll_minority,
                                  uint8_t *posterior_assignment, uint8_t *anomaly_assignment, uint64_t *qual /*[local cells]*/);
/* What option resolve_posteriors did in the last cellector_assign (all zero when it was off, and on a multi-device ctx). */
typedef struct {
    uint64_t n_evaluated;       /* cells evaluated with the reference's arithmetic                                    */
    uint64_t n_labels_changed;  /* ... of them whose label differs from the one the device's own values give          */
    uint64_t n_qual_changed;    /* ... whose qual does                                                                */
    uint32_t mode, reserved;    /* the option's value in that call (1 or 2; 0: nothing was resolved)                  */
} cellector_assign_resolution_t;
cellector_status cellector_assign_resolution(const cellector_ctx *ctx, cellector_assign_resolution_t *out);
/* ... and which cells it evaluated: n_evaluated local cell indices (order unspecified); nothing when it was off. */
cellector_status cellector_assign_resolved_cells(const cellector_ctx *ctx, uint32_t *ids /*[n_evaluated]*/);

/* ---- K-genotype classes: class tallies, posteriors, refine ------------------------------------------
 * calculate_posteriors (main.rs:228-280) is hard-wired to two classes and their doublet.  These calls score every cell of the
 * loaded matrix against K classes given as labels: cellector's own beta-binomial (init_alpha_betas, main.rs:598-611;
 * get_cell_log_likelihoods, main.rs:541-591; the prior / logsumexp chain of main.rs:264-276) generalised from {minority,
 * majority} to K.  The labels may come from peels (cellector_restage + cellector_cell_origin), from cellector_cell_source, from
 * cell hashing or from a clustering with k > 2.  These four calls form no doublet classes; the block after them
 * (cellector_class_doublets) adds the K (K - 1) / 2 pair distributions and their prior.
 *   labels [cells]: 0..K-1, or 255 = unlabelled; 1 <= K <= 16.  scale [K] or NULL = all 1.0; log_prior [K] or NULL = default;
 *   mask [L] or NULL = all L loci used, which is what the reference's posterior phase uses (main.rs:255, :303), not the loop's
 *   filtered mask.
 *   1 tallies: alt_k[l] / ref_k[l] = the sums of the allele counts of the entries of class k's cells at used-locus index l, u64; a
 *     repeated (locus, cell) line counts each time; tallies ignore the mask.  n_k = cells labelled k.  Unlabelled cells are in no
 *     tally: over the classes and the unlabelled cells the tallies add up to cellector_locus_counts.
 *   2 distributions (init_alpha_betas, main.rs:598-611): alpha_k[l] = (double)alt_k[l] * scale_k + 1.0, beta_k[l] likewise from
 *     ref_k: a rounded product and a rounded sum.  K = 2, class 0 the exclusion set, scale = {1, max(mf0, 0.01)}: the bits of
 *     cellector_posterior_alpha_betas(which = 0 / 1).
 *   3 ll_k[c] = get_cell_log_likelihoods (main.rs:541-591) under (alpha_k, beta_k, mask): the cell pass' product-form log-pmf
 *     summed over the cell's entries at used loci.  A cell's own counts are inside its own class's tallies.
 *   4 a class with n_k == 0 is dead: ll column -inf, posterior column 0, no part in 5-7, attracts no cell.  All classes dead
 *     (every cell unlabelled) is CELLECTOR_EINVAL.
 *   5 priors: log_prior as given, else lp_k = log((n_k + 1) / (N_lab + K_live)) with the host's log; N_lab = labelled cells.
 *   6 posterior (main.rs:264-276 over K terms), live classes in ascending k: x_k = lp_k + ll_k, m = max x_k, den = m +
 *     log(sum_k exp(x_k - m)), posterior_k = exp(x_k - den), best = the smallest k attaining m, qual = (uint64) min(-10 log10(rest),
 *     255) with rest = sum_{k != best} exp(x_k - den) (rest == 0: 255).  A cell with no entry at a used locus gets the prior.
 *   7 refine (hard EM), one step: 1-6 from the current labels; a labelled cell with at least min_loci (>= 1) entries at used loci
 *     (a repeated pair counts as often as it occurs, like loci_used_per_cell) takes the label best, every other cell keeps its
 *     label, 255 included; n_moved = labels changed.  Repeated until n_moved == 0 (converged) or max_iter steps have run;
 *     max_iter == 0 does 1-6 only.  scale and a caller's log_prior stay fixed; default priors and dead classes follow the
 *     current labels.  Between two steps the tallies are updated from the moved cells' rows (option class_delta).
 * Needs a loaded matrix and no iteration in flight; engines 1 and 2; a single-device ctx that holds all cells (else
 * CELLECTOR_EINVAL, like cellector_locus_moments).  CELLECTOR_EINVAL with a message, nothing written or launched, also for K
 * outside 1..16, a label that is neither < K nor 255 (the message names the first such cell), a non-finite or negative scale, a
 * NaN prior, min_loci == 0, NULL labels.  Device scratch is allocated before anything is written: on CELLECTOR_ENOMEM the ctx and
 * the caller's labels are as they were.
 * The calls never touch the EM state: the exclusion set, the loop's mask, the kept counts of option tally_delta, the per-cell
 * masked counts and the iteration number all stay, and an EM loop interrupted by a class call continues with the same bits.
 * cellector_class_posteriors and cellector_refine_classes overwrite exactly what cellector_cell_log_likelihoods overwrites (the
 * tables and the per-cell outputs of the last pass; the alpha/beta of the next em_begin are formed again from the state) and
 * invalidate the same caches (the tables built ahead by em_finish, the zeroed column counters). */
cellector_status cellector_class_tallies(cellector_ctx *ctx, const uint8_t *labels /*[cells]*/, uint32_t n_classes,
                                         uint64_t *cells /*[K]*/, uint64_t *alt /*[K][L]*/,
                                         uint64_t *ref /*[K][L]*/); /* any output may be NULL */
cellector_status cellector_class_alpha_betas(cellector_ctx *ctx, const uint8_t *labels, uint32_t n_classes,
                                             const double *scale, double *alpha /*[K][L]*/, double *beta /*[K][L]*/);
cellector_status cellector_class_posteriors(cellector_ctx *ctx, const uint8_t *labels, uint32_t n_classes, const double *scale,
                                            const double *log_prior, const uint8_t *mask, double *ll /*[K][cells]*/,
                                            double *posterior /*[K][cells]*/, uint8_t *best /*[cells]*/,
                                            uint64_t *qual /*[cells]*/); /* any output may be NULL */
typedef struct {
    uint32_t iterations, converged;  /* steps run; 1 = the last one moved no cell                                  */
    uint64_t n_moved_last, n_moved_total;
    uint64_t n_recounts;             /* steps whose tallies were counted from scratch (the others: delta updates)  */
    uint64_t class_cells[16];        /* cells per class under the returned labels                                  */
} cellector_refine_summary;
/* labels: in = the start, out = the result; ll / posterior / qual: of the last step (under the labels that step started from) */
cellector_status cellector_refine_classes(cellector_ctx *ctx, uint8_t *labels, uint32_t n_classes, const double *scale,
                                          const double *log_prior, const uint8_t *mask, uint32_t max_iter, uint64_t min_loci,
                                          cellector_refine_summary *out, double *ll, double *posterior,
                                          uint64_t *qual /*any output may be NULL*/);

/* ---- K-class doublets: pair distributions, calls, held-out refine ---------------------------------------
 * calculate_posteriors scores minority, majority and their doublet (main.rs:242-248, :259, :270-276), and
 * output_final_assignments lets doublet_posterior > 0.5 override the label (main.rs:150-152).  These calls do the same over K
 * classes: beside the K singlet distributions of the block above, one doublet distribution per unordered pair of classes, all
 * K + P hypotheses in one posterior chain, a doublet call, and a refine that keeps the called doublets out of every tally.
 *   labels [cells], 1 <= K <= 16, scale [K], log_prior [K], mask [L]: as cellector_class_posteriors.
 *   held [cells] or NULL = none: a non-zero entry marks a labelled cell that stays out of every tally and is scored like any other.
 *   pair_scale [K] or NULL = default; log_pair_prior [P] or NULL = default.
 *   Pairs are the unordered (a, b), 0 <= a < b < K: P = K (K - 1) / 2 of them, p(a, b) = a (2K - a - 1) / 2 + (b - a - 1).
 *   1 tallies: as step 1 above over the cells with a label < K and held == 0.  Held cells count with the unlabelled ones (slot K):
 *     over the classes and slot K the tallies still add up to cellector_locus_counts.  n_k = unheld cells of class k.  A class with
 *     n_k == 0 is dead; a pair with a dead member is dead: ll_pair column -inf, no part in the chain.  No live class (every
 *     labelled cell held) is CELLECTOR_EINVAL.
 *   2 singlet distributions: unchanged, alpha_k = (double)alt_k * scale_k + 1.0.
 *   3 pair distributions: alpha_ab[l] = ((double)alt_a[l] * ps_a + (double)alt_b[l] * ps_b) + 1.0, beta_ab likewise from the ref
 *     tallies: two rounded products, a rounded sum, then + 1.0, no contraction.  ps = pair_scale; NULL: ps_k = (double)n_min /
 *     (double)n_k with n_min the smallest live n_k (a dead class: 0), which brings every class to the weight of the smallest, as
 *     main.rs:245 does with minority_fraction.  cellector_class_pair_alpha_betas returns all P rows by this formula, dead pairs
 *     included.  K = 2, class 0 the exclusion set, pair_scale = {1, mf0}, mf0 = (n_excl + 1) / (N + 1) unclamped: the bits of
 *     cellector_posterior_alpha_betas(which = 2).
 *   4 ll_k as above; ll_ab = the same cell pass under (alpha_ab, beta_ab, mask).
 *   5 priors.  Singlets: log_prior as given, else log(f_k), f_k = (n_k + 1) / (N_lab + K_live) from the unheld counts.  Pairs:
 *     log_pair_prior as given, else log(((double)N / 1000.0 / 100.0) * fmax(fmin(f_a, f_b), 0.1)) with N = all cells of the matrix
 *     and the host's log: main.rs:259 with the smaller class of the pair in the place of the minority.  Like the reference's, these
 *     priors are NOT normalised: the doublet rate N / 100 000 passes 1 at 10^5 cells, and a caller with 10^6 cells should pass
 *     priors of their own.
 *   6 chain.  Terms: the live singlets in ascending k, then the live pairs in ascending p.  x_t = prior + ll, m = max over all
 *     terms, S = sum exp(x_t - m) in that order, den = m + log S; posterior_k = exp(x_k - den); q_p = exp(y_p - den) with y_p the x
 *     of pair p; doublet_posterior = sum_p q_p in ascending p (0 without a live pair); best = the smallest k attaining the singlet
 *     maximum; best_pair = the (a, b) of the smallest p attaining the pair maximum, (255, 255) without one; call = 1 iff
 *     doublet_posterior > 0.5 (strict, main.rs:150); qual = (uint64) min(-10 log10(rest), 255), 255 where rest == 0, with rest =
 *     (sum_{k != best} posterior_k in ascending k) + doublet_posterior for call 0 and rest = sum_k posterior_k for call 1 (a sum,
 *     never 1 - x).  Dead columns: posterior 0.
 *   7 held-out refine, one step: 1-6 from the current (labels, held); a labelled cell with at least min_loci entries at used loci
 *     takes label = best and held = doublet_posterior > doublet_threshold; every other cell keeps both its label and its flag;
 *     n_moved = cells whose label or flag changed.  Repeated until n_moved == 0 or max_iter steps have run (max_iter == 0: 1-6
 *     only).  A held cell keeps being scored and comes back when its doublet posterior falls.  Between two steps the tallies are
 *     updated from the rows of the moved cells, each leaving its effective class (held ? slot K : label) and joining its new one;
 *     the recount rule and option class_delta are those of cellector_refine_classes, over the effective classes.
 * Scope, refusals and what the calls leave alone and overwrite: exactly as the class calls above.  CELLECTOR_EINVAL with a
 * message, nothing written or launched, also for a non-finite or negative pair_scale, a NaN pair prior, a doublet_threshold outside
 * [0, 1] or NaN.  K = 1 is legal: P = 0, doublet_posterior 0, best_pair (255, 255), call 0.  Every device buffer is allocated before
 * the first write; the caller's labels and held are written once, at the end (held flags come back as 0 / 1).
 * Device scratch beyond the class calls' own: P * 8 B per cell (the pair columns), 16 B per locus (ONE pair distribution at a time),
 * 2 B per cell (the held flags and their successors), and the outputs' 8 + 2 + 1 B per cell (doublet_posterior, best_pair, call). */
cellector_status cellector_class_pair_alpha_betas(cellector_ctx *ctx, const uint8_t *labels, const uint8_t *held, uint32_t n_classes,
                                                  const double *pair_scale, double *alpha /*[P][L]*/, double *beta /*[P][L]*/);
cellector_status cellector_class_doublets(cellector_ctx *ctx, const uint8_t *labels, const uint8_t *held, uint32_t n_classes,
                                          const double *scale, const double *pair_scale, const double *log_prior,
                                          const double *log_pair_prior, const uint8_t *mask, double *ll /*[K][cells]*/,
                                          double *ll_pair /*[P][cells]*/, double *posterior /*[K][cells]*/,
                                          double *doublet_posterior /*[cells]*/, uint8_t *best /*[cells]*/,
                                          uint8_t *best_pair /*[cells][2]*/, uint8_t *call /*[cells]*/,
                                          uint64_t *qual /*[cells]*/); /* any output may be NULL */
typedef struct {
    uint32_t iterations, converged;  /* steps run; 1 = the last one moved no cell                                  */
    uint64_t n_moved_last, n_moved_total; /* cells whose label or held flag changed                                */
    uint64_t n_recounts;             /* steps whose tallies were counted from scratch (the others: delta updates)  */
    uint64_t class_cells[16];        /* unheld cells per class under the returned labels and flags                 */
    uint64_t n_held;                 /* labelled cells held under the returned flags                               */
} cellector_refine_doublets_summary;
/* labels: in = the start, out = the result; held: likewise, NULL in = none held and then not returned; the other outputs: of the
 * last step (under the labels and flags that step started from) */
cellector_status cellector_refine_class_doublets(cellector_ctx *ctx, uint8_t *labels, uint8_t *held, uint32_t n_classes,
                                                 const double *scale, const double *pair_scale, const double *log_prior,
                                                 const double *log_pair_prior, const uint8_t *mask, double doublet_threshold,
                                                 uint32_t max_iter, uint64_t min_loci, cellector_refine_doublets_summary *out,
                                                 double *ll, double *ll_pair, double *posterior, double *doublet_posterior,
                                                 uint8_t *best_pair, uint64_t *qual /*any output may be NULL*/);

/* ---- class genotypes: per-class allele tallies over ALL loci and the genotype call ---------------------------
 * output_final_vcf (main.rs:52-131) re-reads both matrices over all loci (load_mtx_final, load_data.rs:109-132), also those that
 * failed min_alt / min_ref, and calls one of three genotypes per locus for its two classes under an ambient mix.  This call does
 * the same for the K classes of a labelling: what a cluster is matched to a donor with.
 *   labels [cells], 1 <= K <= 16: as cellector_class_posteriors; 255 = in no class.  A caller that holds doublets out (the held
 *   flags of cellector_refine_class_doublets, or call) passes them as 255: there is no held argument.
 *   1 tallies: alt_s[t] / ref_s[t] = the sums of the allele counts of the staged entries at locus t (0 <= t < total_loci, the
 *     matrix' own locus index, not the used-locus index) whose cell has slot s; slot k < K = label k, slot K = the cells labelled
 *     255; u64, exact; a repeated (locus, cell) line counts each time.  cells[s] = the cells of slot s.  Over the K + 1 slots the
 *     planes add up to the locus' totals (the four planes of cellector_final_allele_tallies summed); at a used locus the first K
 *     are cellector_class_tallies'.  One pass over the staged COO whatever K, in any entry order.
 *   2 per locus: A, R = the sums over ALL K + 1 slots; soup = A + R > 0 ? (double)A / (double)(A + R) : 0.5;
 *     p_g = (1.0 - ambient) * e_g + ambient * soup with e = {0.99, 0.5, 0.01} for g = hom-alt, het, hom-ref (main.rs:79-92).
 *   3 per class k with tallies (a, r): l_g = Binomial(a + r, p_g).pmf(a) (statrs; the host's exp and log);
 *     den = 1.0/3.0 * l_alt + 1.0/3.0 * l_het + 1.0/3.0 * l_ref; q_g = l_g * 1.0 / 3.0 / den; gp = fmax(fmax(q_alt, q_het), q_ref);
 *     gt = q_alt > gt_threshold ? 1 : q_het > gt_threshold ? 2 : q_ref > gt_threshold ? 3 : 0 (1 = 1/1, 2 = 0/1, 3 = 0/0, 0 = ./.)
 *     (main.rs:93-124).  ambient 0.03 and gt_threshold 0.99 are the reference's; with them and K = 2, class 0 the exclusion set,
 *     gt and gp are the two sample columns of cellector.vcf.
 *   4 a class without a cell has zero planes: its three pmfs are 1, gp is 1/3 and gt is 0, like a locus without reads.
 *   5 the reference's quirk is kept: at deep tallies all three pmfs can underflow to 0; then den is 0, every q and gp are NaN and
 *     gt is 0.
 * The rule runs on one host thread, in the library, and not at all when gt, gp and gp3 are all NULL.
 * Needs a loaded matrix, no iteration in flight, the staged COO (option keep_coo = 1 at the ingest) and a single-device ctx that
 * holds all cells.  CELLECTOR_EINVAL with a message, nothing written or launched, for these, for the labels cellector_class_posteriors
 * refuses, and for an ambient or a gt_threshold that is NaN or outside [0, 1].  Device scratch ((K + 1) * 16 B per locus of the
 * matrix, 1 B per cell) is allocated before anything is written: on CELLECTOR_ENOMEM the ctx is as it was.
 * The call reads the staged COO and the labels only: it touches nothing of the EM state, overwrites no table and invalidates no
 * cache, and an EM loop interrupted by it continues with the same bits. */
cellector_status cellector_class_genotypes(cellector_ctx *ctx, const uint8_t *labels /*[cells]*/, uint32_t n_classes,
                                           double ambient, double gt_threshold,
                                           uint64_t *cells /*[K+1]*/, uint64_t *alt /*[K+1][total_loci]*/, uint64_t *ref /*[K+1][total_loci]*/,
                                           uint8_t *gt /*[K][total_loci]*/, double *gp /*[K][total_loci]*/,
                                           double *gp3 /*[K][total_loci][3]: q_alt, q_het, q_ref*/);   /* any output may be NULL */

/* ---- genotype clusters without labels: a binomial mixture fitted by annealed soft EM ----------------------------
 * Every class call above starts from labels the caller brings.  These calls make a labelling from the loaded matrix alone: K
 * clusters, each a vector of per-locus alt-allele fractions, fitted by soft EM from random starts; a temperature that grows with a
 * cell's depth flattens the first stages (deep cells would otherwise freeze the first partition they meet) and is annealed away;
 * R restarts run side by side and the best is returned.  The result feeds cellector_refine_classes, cellector_class_doublets and
 * cellector_class_genotypes.  The model below is the specification (cellector_amd/cluster.py repeats it in numpy); no parity with
 * any other program is claimed.
 *   K clusters, 2 <= K <= 16; R restarts, R >= 1; J = K R <= 64 columns, column j = r K + k; L used loci; mask [L] or NULL = all
 *   loci, as in cellector_class_posteriors.  The entries of a cell are those of its by-cell CSR row (cellector_csr_rows) at used,
 *   unmasked loci, in row order; a repeated (locus, cell) pair counts each time.  All arithmetic is f64 without contraction: every
 *   product and every sum below rounds once.
 *   1 depth: n_c = sum (alt + ref) over the cell's entries, an integer; e_c = the number of those entries.
 *   2 start: u(l, j) = (mix64(mix64(seed GOLD + GOLD) + (l J + j + 1) GOLD) >> 11) 2^-53 with l the used-locus index, u64
 *     arithmetic that wraps, mix64 = the splitmix64 finaliser and GOLD = 0x9E3779B97F4A7C15 (csrc/mix64.h);
 *     theta_j[l] = theta_floor + (1.0 - 2.0 theta_floor) u.
 *   3 tables: la_j[l] = log(theta_j[l]), lb_j[l] = log(1.0 - theta_j[l]) with the device's log, stored interleaved as [L][J][2].  A
 *     masked locus takes no part anywhere: its table row is (0, 0), its A and T are 0, its theta is 0.5, and no sum visits it.
 *   4 E step: s_cj = sum over the cell's entries in row order of ((alt la_j[l]) + (ref lb_j[l])): both products rounded, then their
 *     sum, then that added to the accumulator, strictly sequential per (cell, column) from 0.0; the binomial coefficient is the same
 *     in every column and is left out.  Within restart r: x_k = s_{c, rK+k} / T_c (IEEE division), m = max_k x_k, den = sum_k
 *     exp(x_k - m) in ascending k from 0.0, w_{c, rK+k} = exp(x_k - m) / den, o_c = m + log(den).  Uniform priors (the class calls
 *     add theirs later).  A cell without entries has s = 0, w = 1 / K.  obj_r = sum_c o_c: thread t of 256 adds the cells t, t + 256,
 *     ... in ascending order, the 256 partial sums are folded pairwise (h = 128, 64, ... 1: p[t] += p[t + h]): the same bits from
 *     run to run.
 *   5 M step: A_j[l] = sum w_cj alt, T_j[l] = sum w_cj (alt + ref) over the locus' entries in ascending cell order, file order among
 *     the repeats of a pair: the product rounded, then added, strictly sequential per (locus, column) from 0.0, no floating-point
 *     atomics.  theta = min(max((A + 1.0) / (T + 2.0), theta_floor), 1.0 - theta_floor); a locus with no entry gets 0.5.
 *   6 anneal: S = anneal_steps stages.  In stage s < S - 1, T_c = max(1.0, (double)n_c / (anneal_base 2^s)); in the last stage T_c =
 *     1 for every cell.  A stage repeats the iteration (3 tables, 4 E step, 5 M step) until, from its second iteration on, every
 *     restart's |obj_r - obj_r of the stage's previous iteration| < tol, or max_iter iterations have run (max_iter 0: none).  theta
 *     carries over from stage to stage.  The host reads R doubles per iteration.
 *   7 result: tables from the final theta and one E step at T = 1; l_r = obj_r - (double)N log((double)K) (the host's log, N = all
 *     cells); best = the smallest r attaining the maximum.  Of that restart: ll [K][cells] = s, posterior [K][cells] = w,
 *     labels [cells] = argmax_k s (the smallest k on ties), 255 for a cell with e_c < min_loci; theta [K][L].  objective [R] = l_r.
 * Defaults (cellector_cluster_default_params): theta_floor 0.01, anneal_base 20, anneal_steps 9, tol 0.01, max_iter 50, min_loci 1.
 * cellector_cluster_m_step and cellector_cluster_e_step are the two halves cellector_cluster iterates, for a caller's own EM (a
 * start from a partial labelling, say): the M step takes weights w [cells][J] (any J in 1..64) and returns A, T, theta [J][L] and
 * the tables of that theta [L][J][2]; the E step takes tables and returns s, w [cells][J] and obj [R], under temp [cells] or NULL
 * = 1 for every cell.
 * Scope as cellector_class_posteriors: a loaded matrix, no iteration in flight, engines 1 and 2, a single-device ctx that holds
 * all cells.  CELLECTOR_EINVAL with a message, nothing written or launched, for these and for K outside 2..16, R == 0, K R > 64,
 * J != K R (the E step; the M step: J outside 1..64), a theta_floor outside (0, 0.5), anneal_steps outside 1..16, a non-finite or
 * non-positive anneal_base or tol, min_loci == 0, a NaN or negative value in w or temp, a temp < 1, NULL w / tab.  All device scratch
 * is allocated before anything is launched: J * 40 B per cell and per locus and 8 B per entry for the by-locus list (a stable sort
 * of the by-cell CSR by locus, 24 B per entry while it is built, released when the call returns; the step calls build it per
 * call); on CELLECTOR_ENOMEM the ctx is as it was.  The calls never touch the EM state (the exclusion set, the loop's mask, the kept
 * tallies, the iteration number: an interrupted EM loop continues with the same bits) and overwrite nothing of the ctx; they
 * invalidate the caches cellector_cell_log_likelihoods invalidates. */
typedef struct {
    double theta_floor;     /* 0.01: theta stays in [floor, 1 - floor]                                              */
    double anneal_base;     /* 20:   stage s divides a cell's depth by anneal_base 2^s                              */
    double tol;             /* 0.01: a stage ends when no restart's objective moved by this much                   */
    uint32_t anneal_steps;  /* 9:    stages, the last one at T = 1                                                  */
    uint32_t max_iter;      /* 50:   iterations per stage at most                                                   */
    uint64_t min_loci;      /* 1:    a cell with fewer entries at used, unmasked loci is labelled 255               */
} cellector_cluster_params;
typedef struct {
    uint32_t best_restart, iterations, stages, reserved;  /* iterations: over all stages                           */
    uint32_t iterations_per_stage[16];
    uint64_t cluster_cells[16];  /* labelled cells per cluster of the best restart                                  */
    uint64_t n_unlabelled;       /* cells labelled 255                                                              */
} cellector_cluster_summary;
cellector_status cellector_cluster_default_params(cellector_cluster_params *out);
cellector_status cellector_cluster(cellector_ctx *ctx, uint32_t n_clusters, uint32_t n_restarts, uint64_t seed,
                                   const cellector_cluster_params *p /*NULL = defaults*/, const uint8_t *mask /*[L] or NULL*/,
                                   uint8_t *labels /*[cells]*/, double *ll /*[K][cells]*/, double *posterior /*[K][cells]*/,
                                   double *theta /*[K][L]*/, double *objective /*[R]*/,
                                   cellector_cluster_summary *out); /* any output may be NULL */
cellector_status cellector_cluster_m_step(cellector_ctx *ctx, const double *w /*[cells][J]*/, uint32_t J, const uint8_t *mask,
                                          double theta_floor, double *A /*[J][L]*/, double *T /*[J][L]*/, double *theta /*[J][L]*/,
                                          double *tab /*[L][J][2]*/); /* any output may be NULL */
cellector_status cellector_cluster_e_step(cellector_ctx *ctx, const double *tab /*[L][J][2]*/, uint32_t K, uint32_t R,
                                          const double *temp /*[cells] or NULL = 1*/, const uint8_t *mask, double *s /*[cells][J]*/,
                                          double *w /*[cells][J]*/, double *objective /*[R]*/); /* any output may be NULL */

/* ---- donor demultiplexing: cells and classes against KNOWN genotypes ---------------------------------------------
 * The calls above find genotypes nobody told them about.  When the donors of a pool have been genotyped (a SNP array or a WGS VCF
 * per donor) these calls answer "which donor is this barcode, or is it a doublet of two", and name the classes of a labelling by
 * donor.  The model below is the specification (cellector_amd/donors.py repeats it in numpy); no parity with any other
 * demultiplexer is claimed.
 *   D donors, 1 <= D <= 64.  gt [D][total_loci] u8, indexed by the matrix' own locus index (as the planes of
 *   cellector_class_genotypes): 0 = 0/0, 1 = 0/1, 2 = 1/1, 3 = no call; any other value is CELLECTOR_EINVAL.  mask [L] or NULL = all
 *   loci, as in cellector_class_posteriors.  The entries of a cell are those of its by-cell CSR row (cellector_csr_rows) at used,
 *   unmasked loci, in row order; a repeated (locus, cell) pair counts each time.  All arithmetic is f64 without contraction: every
 *   product and every sum below rounds once.
 *   1 packing: gt is uploaded once and packed on the device over the used loci (cellector_locus_ids) into W = ceil(D / 32) u64 words
 *     per locus, packed [L][W]: donor d at bits 2 (d & 31) of word d >> 5; the bits above the last donor are 0.
 *   2 per used, unmasked locus l: A, R = the alt and ref sums over all of the locus' entries (whole numbers: what
 *     cellector_locus_counts returns); soup = ((double)A + 1.0) / ((double)(A + R) + 2.0); e_0 = err, e_1 = 0.5, e_2 = 1.0 - err,
 *     e_3 = soup; theta_g = ((1.0 - ambient) e_g) + (ambient soup).  A donor without a call is scored at the pool's allele fraction.
 *   3 tables, with the device's log: tab1 [L][4][2] = (log theta_g, log(1.0 - theta_g)); tab2 [L][16][2] at index 4 g_a + g_b from
 *     theta = 0.5 (theta_{g_a} + theta_{g_b}).  (x + x) 0.5 is x: tab2[l][5 g] carries the bits of tab1[l][g].  A masked locus' rows
 *     are (0, 0) and no sum visits it.
 *   4 singlets: s_cd = the sum over the cell's entries in row order of ((alt la) + (ref lb)), (la, lb) = tab1[l][g_d(l)]: both
 *     products rounded, then their sum, then that added to the accumulator, strictly sequential per (cell, donor) from 0.0 (step 4
 *     of the cluster model).  u_d = s_cd + log_prior[d] (NULL: + 0.0).  best = the d that maximises u_d, second = the d != best
 *     that does (255 with D = 1), the smallest d on ties.
 *   5 anchor: a_c = anchor[c] if given (< D), else best.
 *   6 pairs: p_cd = the same sequential sum with tab2[l][4 g_{a_c}(l) + g_d(l)], for every d; column d = a_c is the bits of
 *     s_{c, a_c} by step 3 and takes no part in the chain.
 *   7 chain: one softmax over 2 D - 1 hypotheses: the D singlets x_d = u_d + log_singlet, then the D - 1 pairs (a_c, d), d
 *     ascending, y_d = p_cd + log_pair; log_singlet = log(1.0 - doublet_rate), log_pair = log(doublet_rate / (double)(D - 1)) with
 *     the host's log (D = 1: no pairs).  m = the maximum of all terms; den = sum exp(t - m) in that order from 0.0;
 *     posterior_d = exp(x_d - m) / den; pair_posterior_d = exp(y_d - m) / den, 0 at d = a_c; doublet_posterior = the sum of the pair
 *     posteriors in ascending d from 0.0; best_pair = the d of the largest y_d, the smallest on ties (255 with D = 1).
 *   8 status: 255 = unassigned when n_entries < min_loci; else 1 = doublet when doublet_posterior > 0.5 (strict, main.rs:150); else
 *     0 = singlet when posterior[best] >= posterior_threshold; else 2 = ambiguous.  n_entries = the cell's entries at used, unmasked
 *     loci.  The summary counts the four and, for status 0, the cells per donor.
 *   Why anchored pairs: all D (D - 1) / 2 pairs are 2016 columns at D = 64.  The chain is exact whenever the best pair contains the
 *   best singlet; a caller who doubts that sweeps any other donor through the anchor argument (anchor_out returns the one used).
 *   cellector_match_donors: (a_kl, r_kl) = the tallies of cellector_class_tallies under (labels, K); ll_kd = the sum over ascending
 *   unmasked l of (((double)a la) + ((double)r lb)) from tab1, strictly sequential from 0.0; best = argmax_d, the smallest d on ties,
 *   255 for a class without a cell; margin = ll[best] minus the runner-up (+inf with D = 1, 0 for a class without a cell).  It
 *   solves no assignment problem: two classes may name the same donor, and the caller sees that.
 * Defaults (cellector_donor_default_params): err 0.01, ambient 0.03, doublet_rate 0.1, posterior_threshold 0.999, min_loci 1.
 * Scope as cellector_class_posteriors: a loaded matrix, no iteration in flight, engines 1 and 2, a single-device ctx that holds all
 * cells.  CELLECTOR_EINVAL with a message, nothing written or launched, for these and for D outside 1..64, NULL gt, a gt value above
 * 3 (the message names the donor and the locus), err outside (0, 0.5), ambient outside [0, 1), doublet_rate outside [0, 1), a
 * posterior_threshold outside [0, 1], min_loci == 0, a log_prior that is NaN or +inf or -inf for every donor, an anchor >= D, and
 * the labels cellector_class_tallies refuses.  All device scratch is allocated before anything is launched (D bytes per locus of the
 * matrix, 8 W + 321 B per used locus, 32 D + 17 B per cell; match: 16 K B per used locus): on CELLECTOR_ENOMEM the ctx is as it
 * was.  The calls never touch the EM state (an interrupted EM loop continues with the same bits) and overwrite nothing of the ctx;
 * they invalidate the caches cellector_cell_log_likelihoods invalidates. */
typedef struct {
    double err;                  /* 0.01:  the allele fraction of a homozygous-reference donor                  */
    double ambient;              /* 0.03:  the share of a cell's reads that come from the pool                  */
    double doublet_rate;         /* 0.1:   prior mass of the D - 1 anchored pairs together                      */
    double posterior_threshold;  /* 0.999: a singlet is called at this posterior of its best donor              */
    uint64_t min_loci;           /* 1:     a cell with fewer entries at used, unmasked loci is unassigned (255) */
} cellector_donor_params;
typedef struct {
    uint64_t n_singlet, n_doublet, n_ambiguous, n_unassigned;  /* status 0, 1, 2, 255                            */
    uint64_t donor_cells[64];    /* status-0 cells per best donor                                               */
} cellector_donor_summary;
cellector_status cellector_donor_default_params(cellector_donor_params *out);
cellector_status cellector_donor_tables(cellector_ctx *ctx, const uint8_t *gt /*[D][total_loci]*/, uint32_t n_donors,
                                        const cellector_donor_params *p /*NULL = defaults*/, const uint8_t *mask /*[L] or NULL*/,
                                        double *tab1 /*[L][4][2]*/, double *tab2 /*[L][16][2]*/,
                                        uint64_t *packed /*[L][W]*/); /* any output may be NULL */
cellector_status cellector_donor_posteriors(cellector_ctx *ctx, const uint8_t *gt /*[D][total_loci]*/, uint32_t n_donors,
                                            const cellector_donor_params *p /*NULL = defaults*/, const double *log_prior /*[D] or NULL*/,
                                            const uint8_t *anchor /*[cells] or NULL*/, const uint8_t *mask /*[L] or NULL*/,
                                            double *ll /*[cells][D]*/, double *pair_ll /*[cells][D]*/, double *posterior /*[cells][D]*/,
                                            double *pair_posterior /*[cells][D]*/, double *doublet_posterior /*[cells]*/,
                                            uint8_t *best /*[cells]*/, uint8_t *second /*[cells]*/, uint8_t *best_pair /*[cells]*/,
                                            uint32_t *n_entries /*[cells]*/, uint8_t *status /*[cells]*/, uint8_t *anchor_out /*[cells]*/,
                                            cellector_donor_summary *out, double *tab1 /*[L][4][2]*/,
                                            double *tab2 /*[L][16][2]*/); /* any output may be NULL */
cellector_status cellector_match_donors(cellector_ctx *ctx, const uint8_t *labels /*[cells]*/, uint32_t n_classes,
                                        const uint8_t *gt /*[D][total_loci]*/, uint32_t n_donors,
                                        const cellector_donor_params *p /*NULL = defaults*/, const uint8_t *mask /*[L] or NULL*/,
                                        double *ll /*[K][D]*/, uint8_t *best /*[K]*/, double *margin /*[K]*/,
                                        uint64_t *cells /*[K]*/); /* any output may be NULL */

/* ---- donor panels: cells and classes against up to 4096 genotyped donors ---------------------------------------------
 * The donor calls above stop at 64 donors.  A cell village of 100+ lines holds more, and so does the question "which of the 500
 * genotyped individuals of this facility are in this pool".  These calls score every cell against all D donors of a panel in one pass
 * and one softmax; the pairs are those of the anchor with a SHORTLIST of the cell's M best singlets.  Everything not stated here is
 * the donor model above, steps 1 - 8, operation for operation, f64 without contraction.
 *   D donors, 1 <= D <= 4096; gt [D][total_loci] u8 coded as there.  shortlist, 1 <= shortlist <= 64; M = min(shortlist, D).  Donor
 *   indices are uint16_t; 65535 means "none" where the 64-donor calls say 255.
 *   1 - 3 packing, theta, tab1, tab2: unchanged; the tables are cellector_donor_tables' bits; packed [L][W] has W = ceil(D / 32) up to
 *     128.  The u8 genotypes are uploaded and packed in slabs of 256 donors: they never sit on the device whole.
 *   4 singlets: s_cd for all D donors, the same strictly sequential sum; u_d = s_cd + log_prior[d] (NULL: + 0.0); best and second by the
 *     same rule (second 65535 with D = 1).  The bits of s_cd depend on donor d's genotypes alone: column d of ll equals column j of
 *     cellector_donor_posteriors' ll on any subset S of <= 64 donors with S[j] = d, and the ll of cellector_match_donors_panel equals
 *     cellector_match_donors' likewise.
 *   4b the shortlist: the donors ordered by (u_d descending, d ascending); the first M; cand[c][0..M) lists them in ascending d.  The
 *     selection is a function of the bits of u alone.  cand_ll[c][j] = s_{c, cand[c][j]}.
 *   5 anchor: a_c = anchor[c] if given (< D), else best.  A given anchor need not be in the shortlist.
 *   6 pairs: p_cd as there, for d in cand[c] only: cand_pair_ll[c][j].  The slot where cand == a_c carries the bits of s_{c, a_c} and
 *     takes no part in the chain.
 *   7 chain: one softmax over D + (the shortlisted donors other than a_c) hypotheses: the D singlets x_d = u_d + log_singlet in
 *     ascending d, then the pairs (a_c, d), d over cand[c] ascending, d != a_c, y_d = p_cd + log_pair.  log_singlet = log(1.0 -
 *     doublet_rate), log_pair = log(doublet_rate / (double)(D - 1)) with the host's log (D = 1: no pairs): the prior of a pair does not
 *     depend on M.  PAIRS OUTSIDE THE SHORTLIST ARE NOT EVALUATED AND ARE NOT IN den: the posteriors are those of the model that holds
 *     only the listed hypotheses.  m = the maximum of all terms; den = sum exp(t - m) in that order from 0.0; cand_posterior[c][j] =
 *     exp(x_d - m) / den and cand_pair_posterior[c][j] = exp(y_d - m) / den at d = cand[c][j], 0 at d = a_c; best_posterior =
 *     exp(x_best - m) / den; doublet_posterior = the sum of the pair posteriors in ascending d from 0.0; best_pair = the d of the
 *     largest y_d, the smallest on ties, 65535 when the chain has no pair term (D = 1, or M = 1 and the one shortlisted donor is a_c).
 *   8 status: unchanged, from doublet_posterior and best_posterior.  The summary counts the four; donor_cells[d] = the status-0 cells
 *     whose best is d; n_present = the donors with at least one.
 *   With D <= 64 and shortlist >= D, cand[c] is 0 ... D - 1 and every common output equals cellector_donor_posteriors' bit for bit
 *   (indices widened, 255 <-> 65535).
 *   cellector_match_donors_panel: cellector_match_donors for D <= 4096; best is uint16_t, 65535 for a class without a cell.
 * Scope and refusals as cellector_donor_posteriors, with D outside 1..4096, shortlist outside 1..64 and an anchor >= D refused with
 * CELLECTOR_EINVAL and a message, nothing written or launched.  The soft calls (GP / GL / PL), cellector_donor_fit, the ambient, pair
 * fraction and genotype refinement calls stay at D <= 64: a panel call names the donors that are present (donor_cells), and those calls
 * take that subset.  All device scratch is allocated before anything is launched (min(D, 256) bytes per locus of the matrix, 8 W + 321
 * B per used locus, 8 D B, 34 M + 31 B per cell, and 8 D B per cell more only where ll is asked for; match: 16 K B per used locus and
 * 8 K D B): on CELLECTOR_ENOMEM the ctx is as it was.  The calls never touch the EM state and overwrite nothing of the ctx; they
 * invalidate the caches cellector_cell_log_likelihoods invalidates. */
typedef struct {
    uint64_t n_singlet, n_doublet, n_ambiguous, n_unassigned;  /* status 0, 1, 2, 255                            */
    uint64_t n_present;          /* donors with at least one status-0 cell                                      */
} cellector_donor_panel_summary;
cellector_status cellector_donor_panel(cellector_ctx *ctx, const uint8_t *gt /*[D][total_loci]*/, uint32_t n_donors, uint32_t shortlist,
                                       const cellector_donor_params *p /*NULL = defaults*/, const double *log_prior /*[D] or NULL*/,
                                       const uint16_t *anchor /*[cells] or NULL*/, const uint8_t *mask /*[L] or NULL*/,
                                       uint16_t *cand /*[cells][M]*/, double *cand_ll /*[cells][M]*/, double *cand_pair_ll /*[cells][M]*/,
                                       double *cand_posterior /*[cells][M]*/, double *cand_pair_posterior /*[cells][M]*/,
                                       double *doublet_posterior /*[cells]*/, double *best_posterior /*[cells]*/, uint16_t *best /*[cells]*/,
                                       uint16_t *second /*[cells]*/, uint16_t *best_pair /*[cells]*/, uint16_t *anchor_out /*[cells]*/,
                                       uint32_t *n_entries /*[cells]*/, uint8_t *status /*[cells]*/,
                                       uint64_t *donor_cells /*[D]: status-0 cells per best donor*/, cellector_donor_panel_summary *out,
                                       double *ll /*[cells][D] or NULL*/, uint64_t *packed /*[L][W] or NULL*/, double *tab1 /*[L][4][2]*/,
                                       double *tab2 /*[L][16][2]*/); /* any output may be NULL */
cellector_status cellector_match_donors_panel(cellector_ctx *ctx, const uint8_t *labels /*[cells]*/, uint32_t n_classes,
                                              const uint8_t *gt /*[D][total_loci]*/, uint32_t n_donors,
                                              const cellector_donor_params *p /*NULL = defaults*/, const uint8_t *mask /*[L] or NULL*/,
                                              double *ll /*[K][D]*/, uint16_t *best /*[K]*/, double *margin /*[K]*/,
                                              uint64_t *cells /*[K]*/); /* any output may be NULL */

/* ---- donor calls from genotype probabilities: GP / GL / PL in place of a hard call --------------------------------
 * An imputed array or a low-coverage genome gives a donor three weights per locus, and often the heaviest holds little more than
 * half of the mass.  These calls are the donor calls above with a mixture over a donor's three genotypes in every entry's term.
 * Everything not stated here is the donor model above, step for step.
 *   gp [D][total_loci][3] f32, indexed as gt is: entry g = the weight of genotype g (0 = 0/0, 1 = 0/1, 2 = 1/1).  A row of three NaN
 *   is a no-call.  Any other row must be finite, >= 0 and not all zero, else CELLECTOR_EINVAL (the message names the donor and the
 *   locus).  Rows need not sum to 1: w_g = (double)gp_g / (((double)gp_0 + (double)gp_1) + (double)gp_2), and P = { g : w_g > 0 }
 *   (w_g > 0 exactly where gp_g > 0: the quotient cannot underflow).  1 <= D <= 64.  mask, log_prior, anchor and the params are
 *   those of cellector_donor_posteriors.
 *   kind [L][D] u8 over the used loci: 0, 1, 2 = a one-hot row of that genotype (one positive weight: w_g = x / x = 1.0), 3 = a
 *   no-call, 4 = a soft row.  cellector_donor_weights returns w [L][D][3] (0.0 in a no-call's row) and kind as the device holds
 *   them.
 *   tab1 / tab2 are cellector_donor_tables' own, bit for bit: the same kernel, the same theta; nothing of them depends on the donors.
 *   Singlet term of donor d at an entry (alt a, ref r, locus l): t_g = ((double)a la_g) + ((double)r lb_g) from tab1[l][g], the bits
 *   the hard path forms.  m = the maximum of t_g over P; z = the sum over g in P, ascending, from 0.0, of w_g exp(t_g - m), every
 *   difference, product and sum rounded once, exp and log the device's; term = m + log(z).  Genotypes outside P take no part: no
 *   0 exp(+big), and m is never the value of a genotype the row rules out.  A no-call's term is (a la_3) + (r lb_3).  A one-hot row
 *   has z = 1.0 exp(0.0) = 1.0 and log(1.0) = 0.0: its term IS t_g, the hard call's bits, and the library takes the lookup for
 *   kind < 4.  The terms are added strictly in row order from 0.0, as step 4.
 *   Pair term of (anchor a_c, donor d): t_gh from tab2[l][4 g + h], g over the anchor row's P (a no-call: {3} at weight 1.0), h over
 *   the donor row's likewise; m = the maximum over that product set; z = the sum over g ascending, then h ascending, of
 *   (w_g w_h) exp(t_gh - m); term = m + log(z); the lookup tab2[l][4 g + h] when both rows have kind < 4.  Column d = a_c takes no
 *   part in the chain, and pair_ll[c][a_c] is a copy of ll[c][a_c].
 *   best, second, the anchor, the softmax chain over the 2 D - 1 hypotheses, status and the summary: steps 4 to 8, unchanged.
 *   cellector_match_donors_gp: the singlet term with the class tallies ((double)a_kl, (double)r_kl) as counts, over ascending
 *   unmasked loci; best / margin / cells as cellector_match_donors.
 *   With gp the one-hot of a gt (and three NaN for its no-calls) every output equals the hard call's, byte for byte.
 * Scope and errors as cellector_donor_posteriors: a single-device ctx that holds all cells, a loaded matrix, no iteration in flight,
 * engines 1 and 2; CELLECTOR_EINVAL with a message and nothing written or launched (the rows of gp are checked on the host; the
 * weights kernel counts any row it would refuse itself, and a count above 0 is CELLECTOR_EDEVICE).  All device scratch is allocated
 * before anything is launched: 12 D bytes per locus of the matrix, 25 D + 321 B per used locus, 32 D + 17 B per cell (match: 16 K B
 * per used locus more, nothing per cell); on CELLECTOR_ENOMEM the ctx is as it was.  The EM state is never touched; the caches
 * cellector_cell_log_likelihoods invalidates are invalidated. */
cellector_status cellector_donor_posteriors_gp(cellector_ctx *ctx, const float *gp /*[D][total_loci][3]*/, uint32_t n_donors,
                                               const cellector_donor_params *p /*NULL = defaults*/, const double *log_prior /*[D] or NULL*/,
                                               const uint8_t *anchor /*[cells] or NULL*/, const uint8_t *mask /*[L] or NULL*/,
                                               double *ll /*[cells][D]*/, double *pair_ll /*[cells][D]*/, double *posterior /*[cells][D]*/,
                                               double *pair_posterior /*[cells][D]*/, double *doublet_posterior /*[cells]*/,
                                               uint8_t *best /*[cells]*/, uint8_t *second /*[cells]*/, uint8_t *best_pair /*[cells]*/,
                                               uint32_t *n_entries /*[cells]*/, uint8_t *status /*[cells]*/, uint8_t *anchor_out /*[cells]*/,
                                               cellector_donor_summary *out, double *tab1 /*[L][4][2]*/,
                                               double *tab2 /*[L][16][2]*/); /* any output may be NULL */
cellector_status cellector_donor_weights(cellector_ctx *ctx, const float *gp /*[D][total_loci][3]*/, uint32_t n_donors,
                                         double *w /*[L][D][3]*/, uint8_t *kind /*[L][D]*/); /* any output may be NULL */
cellector_status cellector_match_donors_gp(cellector_ctx *ctx, const uint8_t *labels /*[cells]*/, uint32_t n_classes,
                                           const float *gp /*[D][total_loci][3]*/, uint32_t n_donors,
                                           const cellector_donor_params *p /*NULL = defaults*/, const uint8_t *mask /*[L] or NULL*/,
                                           double *ll /*[K][D]*/, uint8_t *best /*[K]*/, double *margin /*[K]*/,
                                           uint64_t *cells /*[K]*/); /* any output may be NULL */

/* ---- the fit of the called hypothesis: cells no genotyped donor explains ----------------------------------------------
 * The softmax of cellector_donor_posteriors sums to 1 over the 2 D - 1 hypotheses whoever the cell is: a cell of a donor missing from
 * gt (a failed array, a sample swap, a pool member nobody genotyped) receives a confident call for something else, usually a doublet
 * of two other donors.  These calls measure how well the CALLED hypothesis explains the cell: the statistic the reference's author
 * left commented out at main.rs:317-318, (ll - expected) / sqrt(variance), for the donor model, and the loop's own robust rule
 * (main.rs:324-331) over it.  Everything not stated here is the donor model above, step for step; all arithmetic is f64 without
 * contraction, every product, quotient and sum rounds once.  cellector_amd/donors.py (moment_tables, fit_sums, fit) is the twin.
 *   An entry's term is a log theta + r log(1 - theta) with no binomial coefficient.  Under Binomial(n = a + r, theta) its mean is
 *   n (theta log theta + (1 - theta) log(1 - theta)) and its variance n theta (1 - theta) (log theta - log(1 - theta))^2: both are n
 *   times a constant of (locus, genotype).
 *   1 moment tables, with the device's log: mom1 [L][4][2] and mom2 [L][16][2] = (h, v).  th and rest = 1.0 - th are formed by exactly
 *     the operations of steps 2 and 3 of the donor model for that (l, 4 g_a + g_b) (mom1: g_a = g_b); la = log(th), lb = log(rest);
 *     h = (th la) + (rest lb); d = la - lb; v = (th rest) (d d).  mom2[l][5 g] carries the bits of mom1[l][g].  A masked locus' rows
 *     are (0, 0).  tab1 / tab2 of the donor call are untouched by this: the same kernel makes them, the same bytes.
 *   2 per-cell sums, over the cell's entries at used, unmasked loci in row order, strictly sequential from 0.0, n = (double)(alt +
 *     ref): E_cd += n h, V_cd += n v with (h, v) = mom1[l][g_d(l)]; PE_cd, PV_cd likewise with mom2[l][4 g_{a_c}(l) + g_d(l)], a_c
 *     the anchor the donor call used.  Column d = a_c of the pair sums is the bits of the singlet sums.
 *   3 z_cd = (s_cd - E_cd) / sqrt(V_cd), pz_cd = (p_cd - PE_cd) / sqrt(PV_cd) with the device's sqrt; s and p are the donor call's
 *     own ll and pair_ll (the call runs it internally: the same bits).  Where the variance is 0.0 (no entry, or only entries of
 *     total 0) the z is 0.0.
 *   4 the called hypothesis: status 1: (hyp_a, hyp_b) = (a_c, best_pair), call_z = pz[c][best_pair]; otherwise (best, 255) and
 *     call_z = z[c][best].  A status-255 cell has call_z = 0.0 and is never judged.
 *   5 keys = the call_z of the status-0 cells in ascending cell order; {median, iqr, threshold} are what
 *     cellector_order_statistics(keys, n_keys, iqr_multiple) returns for them, bit for bit (the library's select).  With fewer than
 *     min_cells keys the select is not run: median and iqr are NaN, threshold is -inf and nothing is flagged.
 *   6 unmatched[c] = 1 when status != 255 and call_z < threshold (strict, main.rs:331).  The summary carries n_keys, the three
 *     statistics, the unmatched cells in all and by status 0 / 1 / 2, and per best donor (the donor call's best) their number.
 *   The z is not standard normal (theta is not the cell's true allele fraction at every locus): the threshold is the robust rule
 *   over the pool's own singlets, not a fixed cut.  A doublet one of whose parents is missing can score inside the kept range.
 *   Genotype probabilities (GP / GL / PL) are not in this model: a mixture's moments have no closed form.  A caller with soft calls
 *   scores the most probable genotype of every row (donors.hard_codes), as --estimate_ambient does.
 * Defaults (cellector_donor_fit_default_params): iqr_multiple 3.0, min_cells 8.
 * Scope, errors and scratch as cellector_donor_posteriors (a single-device ctx that holds all cells, a loaded matrix, no iteration
 * in flight, engines 1 and 2; CELLECTOR_EINVAL with a message, nothing written or launched), and CELLECTOR_EINVAL too for an
 * iqr_multiple that is NaN or negative and for min_cells < 4.  All device scratch is allocated before anything is launched (the
 * donor call's, and 320 B per used locus and 48 D + 18 B per cell more); on CELLECTOR_ENOMEM the ctx is as it was.  The EM state is
 * never touched; the caches cellector_cell_log_likelihoods invalidates are invalidated, and the select's scratch is used as
 * cellector_order_statistics uses it. */
typedef struct {
    double iqr_multiple;  /* 3.0: threshold = q1 - iqr_multiple * iqr over the status-0 cells' z */
    uint64_t min_cells;   /* 8:   with fewer status-0 cells no threshold is formed (>= 4)       */
} cellector_donor_fit_params;
typedef struct {
    uint64_t n_keys;                  /* status-0 cells                                          */
    double median, iqr, threshold;    /* of their call_z; NaN, NaN, -inf below min_cells keys    */
    uint64_t n_unmatched, n_unmatched_singlet, n_unmatched_doublet, n_unmatched_ambiguous; /* all; status 0, 1, 2 */
    uint64_t donor_unmatched[64];     /* unmatched cells per best donor                          */
} cellector_donor_fit_summary;
cellector_status cellector_donor_fit_default_params(cellector_donor_fit_params *out);
cellector_status cellector_donor_moment_tables(cellector_ctx *ctx, const cellector_donor_params *p /*NULL = defaults*/,
                                               const uint8_t *mask /*[L] or NULL*/, double *mom1 /*[L][4][2]*/,
                                               double *mom2 /*[L][16][2]*/); /* any output may be NULL */
cellector_status cellector_donor_fit(cellector_ctx *ctx, const uint8_t *gt /*[D][total_loci]*/, uint32_t n_donors,
                                     const cellector_donor_params *p /*NULL = defaults*/,
                                     const cellector_donor_fit_params *fit /*NULL = defaults*/, const double *log_prior /*[D] or NULL*/,
                                     const uint8_t *anchor /*[cells] or NULL*/, const uint8_t *mask /*[L] or NULL*/,
                                     double *fit_e /*[cells][D]*/, double *fit_v /*[cells][D]*/, double *pair_e /*[cells][D]*/,
                                     double *pair_v /*[cells][D]*/, double *z /*[cells][D]*/, double *pair_z /*[cells][D]*/,
                                     double *call_z /*[cells]*/, uint8_t *hyp_a /*[cells]*/, uint8_t *hyp_b /*[cells]*/,
                                     uint8_t *status /*[cells]*/, uint8_t *unmatched /*[cells]*/, cellector_donor_fit_summary *out,
                                     double *mom1 /*[L][4][2]*/, double *mom2 /*[L][16][2]*/); /* any output may be NULL */

/* ---- ambient fraction estimation: a profile likelihood over a grid of rho ------------------------------------------
 * The donor calls above and cellector_class_genotypes take the ambient fraction (the share of a barcode's reads that come from the
 * pool and not from its own cell) as a number the caller supplies.  These calls measure it: every cell is scored under the
 * genotypes of the source it is assigned to at G values of rho at once, the sums are added over the cells, and the maximum of
 * that profile is the estimate.  The log-likelihood is a sum of logs of functions affine in rho: it is concave, a grid that zooms
 * in finds its one maximum, and a parabola through the last three points gives the estimate and its standard error.  The model
 * below is the specification (cellector_amd/ambient.py repeats it in numpy); no parity with any other demultiplexer is claimed.
 *   S sources, 1 <= S <= 64.  gt [S][total_loci] u8 is coded and packed exactly as for cellector_donor_posteriors (0 = 0/0, 1 = 0/1,
 *   2 = 1/1, 3 = no call; step 1 there).  A source is a donor, or a class whose genotypes came from cellector_class_genotypes.
 *   assign [cells] u8: the source a cell is scored under; 255 = the cell takes no part (how the caller passes doublets and
 *   unassigned cells); any other value >= S is CELLECTOR_EINVAL.  rho [G], 4 <= G <= 32, every value finite and in [0, 1).  mask [L]
 *   or NULL = all loci.  The entries of a cell are those of its by-cell CSR row at used, unmasked loci, in row order.  All arithmetic
 *   is f64 without contraction: every product, quotient and sum below rounds once.
 *   1 tables: per used, unmasked locus soup and e_g are those of step 2 of the donor model: soup = ((double)A + 1.0) /
 *     ((double)(A + R) + 2.0), e = {err, 0.5, 1.0 - err, soup}.  theta_{g,j} = ((1.0 - rho_j) e_g) + (rho_j soup);
 *     tab [L][4][G][2] = (log theta, log(1.0 - theta)) with the device's log.  A masked locus' rows are (0, 0) and no sum visits it.
 *     Where rho_j == ambient, tab[l][g][j] carries the bits of cellector_donor_tables' tab1[l][g].
 *   2 cell sums: ll_cj = the sum over the cell's entries in row order of ((alt la) + (ref lb)), (la, lb) = tab[l][g_{assign[c]}(l)][j]:
 *     both products rounded, then their sum, then that added to the accumulator, strictly sequential per (cell, j) from 0.0 (step 4
 *     of the donor model).  n_entries[c] = the number of those entries.  A cell with assign 255 has a row of 0.0 and n_entries 0.
 *     ll[c][j] is bit for bit the ll[c][assign[c]] of cellector_donor_posteriors(..., ambient = rho_j).
 *   3 totals: total[j] = the sum of ll_cj over the cells with assign != 255, folded as the objective of the cluster model: thread t
 *     of 256 adds its cells t, t + 256, ... in ascending order from 0.0, skipping the cells that take no part; the 256 partial sums
 *     are then folded pairwise, p_t = p_t + p_{t+h} for t < h, h = 128, 64 ... 1.  source_total[s][j]: the same fold over the cells
 *     of source s; source_cells[s]: their number.
 *   4 the vertex rule, per cell on the device: j* = the smallest j that maximises ll_cj; jj = min(max(j*, 1), G - 2);
 *     x0, x1, x2 = rho[jj - 1], rho[jj], rho[jj + 1]; y0, y1, y2 = ll_c at those.  The parabola through three points that need not
 *     be equally spaced, in this order of operations:
 *       h0 = x1 - x0; h1 = x2 - x1; d0 = (y1 - y0) / h0; d1 = (y2 - y1) / h1; c = (2.0 (d1 - d0)) / (h0 + h1)    (the curvature)
 *       unresolved: where |y1 - y0| <= 2^-40 |y1| and |y2 - y1| <= 2^-40 |y1|, c = 0.0 instead
 *       c < 0:  v = (0.5 (x0 + x1)) - (d0 / c); cell_rho = min(max(v, x0), x2); cell_se = 1.0 / sqrt(-c)
 *       else (a flat or degenerate cell, e.g. one whose every entry lies at a no-call locus; a NaN from a grid that repeats a
 *       value lands here too): cell_rho = rho[j*], cell_se = +inf.
 *     Why "unresolved": at a no-call locus theta is ((1.0 - rho) soup) + (rho soup), which is soup only up to a rounding that
 *     differs with rho, so a profile that is flat in exact arithmetic arrives as noise of a few ulps and of either sign, and a
 *     parabola through noise has whatever curvature the noise gives it.  The sums themselves carry (n + 1) u of rounding per row and
 *     (cells / 256 + 8) u per fold, near 2^-41 of the value at 10^6 cells: two steps that both stay below 2^-40 of the value cannot
 *     be told from rounding, and the rule says so (se = +inf) rather than report a standard error made of it.  A profile with signal
 *     moves by c h^2 / 2 per step, many orders above that on every grid this library builds from data that bear on rho.
 *     A cell with n_entries < min_loci or assign 255 gets NaN for both.
 *   5 cellector_estimate_ambient: parameters {err 0.01, lo 0.0, hi 0.5, grid 16, rounds 3, min_loci 1}
 *     (cellector_ambient_default_params).  lo_0, hi_0 = lo, hi.  Round r builds rho_j = lo_r + ((double)j ((hi_r - lo_r) /
 *     (double)(G - 1))), runs steps 1 to 3, takes j* = the smallest argmax of total, and sets lo_{r+1} = rho[max(j* - 1, 0)],
 *     hi_{r+1} = rho[min(j* + 1, G - 1)].  After the last round the pooled rho, se and curvature are the vertex rule of step 4
 *     applied on the host to total, rho then clamped into [lo, hi] of the parameters; at_boundary = 1 when it lies at lo or hi of
 *     the parameters.  The same rule gives source_rho[s], source_se[s] from source_total[s]; a source without a cell, and every s
 *     >= S, gets NaN.  log_likelihood = total at the last round's j*; lo, hi, j_star are the last round's; n_cells_used = the cells
 *     with assign != 255.  The per-cell outputs are those of ROUND 0, the wide grid: a cell's maximum lies anywhere in it, and its se
 *     is tens of grid steps of the last round.  The host reads G + S G doubles per round and nothing per cell but the outputs asked for.
 * Scope as cellector_donor_posteriors: a loaded matrix, no iteration in flight, engines 1 and 2, a single-device ctx that holds all
 * cells.  CELLECTOR_EINVAL with a message, nothing written or launched, for these and for S outside 1..64, NULL gt / assign / rho, a
 * gt value above 3, an assign that is neither 255 nor below S, G outside 4..32, a rho value that is NaN or outside [0, 1), err
 * outside (0, 0.5), lo / hi not satisfying 0 <= lo < hi < 1, rounds outside 1..8, min_loci == 0.  All device scratch is allocated
 * before anything is launched: S bytes per locus of the matrix, 64 G + 8 W + 1 B per used locus (W = ceil(S / 32)), 8 G + 21 B
 * per cell and 8 (S + 2) G + 8 (S + 1) B beside them (cellector_ambient_tables: 64 G + 1 B per used locus and 8 G B): on
 * CELLECTOR_ENOMEM the ctx is as it was.  The calls never touch the EM state (an interrupted EM loop continues with the same bits)
 * and overwrite nothing of the ctx; they invalidate the caches cellector_cell_log_likelihoods invalidates, as the donor calls do. */
typedef struct {
    double err;         /* 0.01: the allele fraction of a homozygous-reference source               */
    double lo, hi;      /* 0.0, 0.5: the first round's grid spans [lo, hi]; the estimate stays in it */
    uint32_t grid;      /* 16:   G, the grid points of a round (4..32)                                */
    uint32_t rounds;    /* 3:    each round's grid spans the two steps around the last one's maximum   */
    uint64_t min_loci;  /* 1:    a cell with fewer entries at used, unmasked loci gets no cell_rho     */
} cellector_ambient_params;
typedef struct {
    double rho, se, curvature, log_likelihood; /* the pooled estimate, 1 / sqrt(-curvature), total at j_star  */
    double lo, hi;                             /* the last round's grid                                        */
    uint32_t j_star, at_boundary, rounds, reserved;
    uint64_t n_cells_used;                     /* cells with assign != 255                                     */
    double source_rho[64], source_se[64];      /* NaN for a source without a cell and for s >= S               */
    uint64_t source_cells[64];
} cellector_ambient_summary;
cellector_status cellector_ambient_default_params(cellector_ambient_params *out);
cellector_status cellector_ambient_tables(cellector_ctx *ctx, const double *rho /*[G]*/, uint32_t n_grid, double err,
                                          const uint8_t *mask /*[L] or NULL*/, double *tab /*[L][4][G][2]*/);
cellector_status cellector_ambient_profile(cellector_ctx *ctx, const uint8_t *gt /*[S][total_loci]*/, uint32_t n_sources,
                                           const uint8_t *assign /*[cells]*/, const double *rho /*[G]*/, uint32_t n_grid, double err,
                                           uint64_t min_loci, const uint8_t *mask /*[L] or NULL*/, double *ll /*[cells][G]*/,
                                           double *total /*[G]*/, double *source_total /*[S][G]*/, uint64_t *source_cells /*[S]*/,
                                           uint32_t *n_entries /*[cells]*/, double *cell_rho /*[cells]*/, double *cell_se /*[cells]*/,
                                           double *tab /*[L][4][G][2]*/); /* any output may be NULL */
cellector_status cellector_estimate_ambient(cellector_ctx *ctx, const uint8_t *gt /*[S][total_loci]*/, uint32_t n_sources,
                                            const uint8_t *assign /*[cells]*/, const cellector_ambient_params *params /*NULL = defaults*/,
                                            const uint8_t *mask /*[L] or NULL*/, cellector_ambient_summary *summary,
                                            double *cell_rho /*[cells]*/, double *cell_se /*[cells]*/,
                                            uint32_t *n_entries /*[cells]*/); /* any output may be NULL */

/* ---- donor pair fractions: a doublet's mixing share, profiled over a grid of f -----------------------------------------------
 * Every doublet hypothesis of the donor calls mixes its two genotypes at equal weight (step 3 there: theta = 0.5 (theta_{g_a} +
 * theta_{g_b})).  A droplet rarely obeys that: a large cell caught with a small one gives 80 / 20, a singlet carrying a clump of
 * another donor's RNA 95 / 5, and the 0.5 hypothesis is the best the softmax has for both.  These calls measure the share: a cell is
 * scored under a PAIR of donors (a, b) at G values of f, the share of its reads that come from donor a, at once; the maximum of that
 * profile is the estimate.  The log-likelihood is a sum of logs of functions affine in f: it is concave, and the vertex rule of the
 * ambient model (step 4 there) carries over unchanged.  Everything not stated here is the donor model above, step for step; all
 * arithmetic is f64 without contraction: every product, quotient and sum below rounds once.  cellector_amd/pair_fraction.py is the
 * twin; no parity with any other demultiplexer is claimed.
 *   gt [D][total_loci] u8 is coded and packed exactly as for cellector_donor_posteriors (step 1 there), 1 <= D <= 64.  pair_a, pair_b
 *   [cells] u8: the pair a cell is scored under; pair_a == 255 = the cell takes no part and its pair_b is ignored; otherwise both are
 *   below D and differ.  frac [G], 4 <= G <= 32, every value finite and in [0, 1], strictly ascending; NULL = the default grid
 *   j / 16.0, j = 0 ... 16 (n_grid is then ignored: G = 17), which holds 0, 0.5 and 1 exactly.  mask [L] or NULL = all loci.  The
 *   cellector_donor_params are the donor call's; err and ambient are used.
 *   1 tables: theta_g is step 2 of the donor model, ambient mix included.  theta_{g_a,g_b,j} = (f_j theta_{g_a}) + ((1.0 - f_j)
 *     theta_{g_b}); tab [L][16][G][2] = (log theta, log(1.0 - theta)) at index 4 g_a + g_b with the device's log.  A masked locus'
 *     rows are (0, 0) and no sum visits it.  256 G bytes per used locus; an entry reads one row of 16 G bytes.  Scaling by a power of
 *     two is exact, so where f_j == 0.5 the column carries the bits of cellector_donor_tables' tab2[l][4 g_a + g_b] ((0.5 x) + (0.5 y)
 *     is 0.5 (x + y)), where f_j == 1.0 it carries tab1[l][g_a] ((1.0 x) + (0.0 y) is x) and where f_j == 0.0 tab1[l][g_b].
 *   2 cell sums: ll[c][j] = the sum over the cell's entries in row order of ((alt la) + (ref lb)), (la, lb) =
 *     tab[l][4 g_{a_c}(l) + g_{b_c}(l)][j]: both products rounded, then their sum, then that added to the accumulator, strictly
 *     sequential per (cell, j) from 0.0 (step 4 of the donor model).  n_entries[c] = the number of those entries.  A cell that takes
 *     no part has a row of 0.0 and n_entries 0.  By step 1, ll[c][j] at f_j == 0.5, 1.0 and 0.0 is, bit for bit, pair_ll[c][b],
 *     ll[c][a] and ll[c][b] of cellector_donor_posteriors run with anchor[c] = a.
 *   3 the vertex rule: step 4 of the ambient model verbatim (the same function on the device), its "unresolved" rule included, on
 *     (frac, ll[c]): j_star [cells] u8 = the smallest j that maximises ll[c][j] (0 for a cell that takes no part), cell_frac = the
 *     vertex clamped into the three points' span, cell_se = 1 / sqrt(-curvature); a flat or convex profile gives frac[j_star] and
 *     +inf.
 *   4 kind [cells] u8: 255 = no part, or n_entries < min_loci: cell_frac and cell_se are NaN; else 3 = flat (cell_se == +inf, e.g. no
 *     entry at a locus where the two genotypes differ); else 1 = toward a (cell_frac > 1.0 - min_fraction); else 2 = toward b
 *     (cell_frac < min_fraction); else 0 = balanced.  The summary counts the five kinds, and per donor the kind-1 cells under their a
 *     and the kind-2 cells under their b: the donor they lean to.
 *   One grid per call and no zoom: each cell's maximum lies somewhere else, so a zoomed grid could not be shared across cells, and
 *   one wide grid with one parabola is within the cell's own standard error at droplet depth.
 * Defaults (cellector_pair_fraction_default_params): min_fraction 0.1, min_loci 1.
 * Scope and errors as cellector_donor_posteriors: a single-device ctx that holds all cells, a loaded matrix, no iteration in flight,
 * engines 1 and 2.  CELLECTOR_EINVAL with a message, nothing written or launched, for the donor call's own errors, NULL pair_a /
 * pair_b, a pair_a that is neither 255 nor below D, a pair_b >= D or equal to pair_a where pair_a != 255 (the message names the first
 * offending cell), G outside 4..32, a frac value that is NaN, outside [0, 1] or not above the one before it, min_fraction outside
 * [0, 0.5], min_loci == 0.  All device scratch is allocated before anything is launched: D bytes per locus of the matrix, 256 G + 8 W
 * + 1 B per used locus (W = ceil(D / 32)), 8 G + 24 B per cell and 8 G B beside them (cellector_pair_fraction_tables: 256 G + 1 B per
 * used locus and 8 G B): on CELLECTOR_ENOMEM the ctx is as it was.  The EM state is never touched (an interrupted EM loop continues
 * with the same bits) and nothing of the ctx is overwritten; the caches cellector_cell_log_likelihoods invalidates are invalidated. */
typedef struct {
    double min_fraction;  /* 0.1: a cell whose share lies within this of 1 or 0 leans to a or to b ([0, 0.5]) */
    uint64_t min_loci;    /* 1:   a cell with fewer entries at used, unmasked loci gets kind 255              */
} cellector_pair_fraction_params;
typedef struct {
    uint64_t n_balanced, n_toward_a, n_toward_b, n_flat, n_none;  /* kind 0, 1, 2, 3, 255                      */
    uint64_t donor_cells[64];  /* the kind-1 cells per pair_a and the kind-2 cells per pair_b                   */
} cellector_pair_fraction_summary;
cellector_status cellector_pair_fraction_default_params(cellector_pair_fraction_params *out);
cellector_status cellector_pair_fraction_tables(cellector_ctx *ctx, const cellector_donor_params *donor_params /*NULL = defaults*/,
                                                const double *frac /*[G] or NULL*/, uint32_t n_grid, const uint8_t *mask /*[L] or NULL*/,
                                                double *tab /*[L][16][G][2]*/);
cellector_status cellector_donor_pair_fractions(cellector_ctx *ctx, const uint8_t *gt /*[D][total_loci]*/, uint32_t n_donors,
                                                const cellector_donor_params *donor_params /*NULL = defaults*/,
                                                const cellector_pair_fraction_params *params /*NULL = defaults*/,
                                                const uint8_t *pair_a /*[cells]*/, const uint8_t *pair_b /*[cells]*/,
                                                const double *frac /*[G] or NULL*/, uint32_t n_grid, const uint8_t *mask /*[L] or NULL*/,
                                                double *ll /*[cells][G]*/, uint32_t *n_entries /*[cells]*/, double *cell_frac /*[cells]*/,
                                                double *cell_se /*[cells]*/, uint8_t *j_star /*[cells]*/, uint8_t *kind /*[cells]*/,
                                                cellector_pair_fraction_summary *summary,
                                                double *tab /*[L][16][G][2]*/); /* any output may be NULL */

/* ---- donor genotype refinement: fill and correct the donors' calls from the pool ----------------------------------------------
 * The donor calls above carry genotypes to the cells; this call carries the cells' reads back to the genotypes.  A donor VCF from an
 * array or a low-coverage genome has no call at many loci of the matrix, some wrong calls, and soft rows; the reads of the cells
 * called for a donor say what that donor is at every covered locus, with far more depth than any single cell.  The model below is the
 * specification (cellector_amd/donor_genotypes.py repeats it in numpy); it is the library's own, no parity with any other program is
 * claimed.  All arithmetic is f64 without contraction: every product, quotient and sum below rounds once.
 *   assign [cells] u8: the donor (< D) a cell's reads are counted for, or 255 = the cell takes no part (a caller passes best where
 *   status == 0).  prior [D][total_loci][3] f32 or NULL, indexed by the matrix' own locus index: validated and normalised exactly as
 *   the gp of cellector_donor_posteriors_gp (a row of three NaN is a no-call; any other row finite, >= 0, not all zero; w_g =
 *   (double)p_g / (((double)p_0 + (double)p_1) + (double)p_2)); NULL = every row is a no-call.  1 <= D <= 64.  params: err and ambient
 *   as in cellector_donor_params; gt_threshold (0.99, the reference's, main.rs:93-124) within [0, 1]; prior_floor (0.01) within
 *   [0, 1]: the chance that a stated call is wrong, the meaning and the default of err.  At prior_floor 0 a one-hot row can never be
 *   overturned.
 *   1 tallies over ALL total_loci loci of the matrix, not only the used ones: alt[s][t], ref[s][t] u64 for s = 0 ... D = the sums of
 *     the staged entries' counts at locus t over the cells of slot s; slot D holds the cells assigned 255.  Exact in any entry order;
 *     a repeated (locus, cell) pair counts each time.  cells[s] = the number of cells in slot s.
 *   2 per locus t: A, R = the sums over all D + 1 slots; soup = ((double)A + 1.0) / ((double)(A + R) + 2.0); e = {err, 0.5,
 *     1.0 - err}; theta_g = ((1.0 - ambient) e_g) + (ambient soup); la_g = log(theta_g), lb_g = log(1.0 - theta_g) with the device's
 *     log: tab [total_loci][3][2].  These are steps 2 and 3 of the donor model: at a used locus (la_g, lb_g) carries the bits of
 *     cellector_donor_tables' tab1[l][g].
 *   3 per (donor d, locus t) with tallies (a, r): lam_g = ((double)a la_g) + ((double)r lb_g); w_g = the normalised prior weight,
 *     1.0 / 3.0 each in a no-call row; v_g = ((1.0 - prior_floor) w_g) + (prior_floor / 3.0); a g with v_g == 0 takes no part (its
 *     q_g is 0); x_g = lam_g + log(v_g); m = the maximum of the x_g; den = the sum of exp(x_g - m) in ascending g from 0.0; q_g =
 *     exp(x_g - m) / den, exp and log the device's.  Everything stays in log space: no depth underflows to NaN.  call = the argmax
 *     of q, the smallest g on ties; gt_out = call if q_call > gt_threshold (strict), else 3.
 *   4 kind [D][total_loci] u8, with prior_call = the argmax of w (the smallest g on ties), 3 for a no-call row: 0 = a + r == 0, so q
 *     is the floored prior; else 4 = withdrawn: gt_out == 3 although there are reads; else 2 = filled: the prior is a no-call and
 *     gt_out is a call; else 1 = confirmed: gt_out == prior_call; else 3 = changed: both are calls and they differ.
 *   5 the summary: per donor its cells, the loci with reads (kind != 0) and the number of loci of each kind 1 ... 4.
 * Limits.  The cells were called WITH the prior, so the tallies lean toward it: a wrong call that drew the wrong cells is confirmed
 * by them.  A donor with few cells gets withdrawn, not a call.  Doublets must stay out of assign: their reads are another donor's.
 * Defaults (cellector_donor_genotypes_default_params): err 0.01, ambient 0.03, gt_threshold 0.99, prior_floor 0.01.
 * Scope as cellector_class_genotypes: the staged COO (option keep_coo), a loaded matrix, no iteration in flight, a single-device ctx
 * that holds all cells and fewer than 2^32 used entries (the scope check all donor calls share; the planes themselves are u64).  The
 * staged COO of a loaded matrix is locus-major whatever order it was ingested in, which is what the tally pass is fast on.  CELLECTOR_EINVAL with a message, nothing written or launched, for these and for D outside 1..64, NULL
 * assign, an assign value that is neither below D nor 255 (the message names the cell), a refused row of prior (the message names
 * the donor and the locus), err outside (0, 0.5), ambient outside [0, 1), gt_threshold or prior_floor outside [0, 1].  All device
 * scratch is allocated before the first launch: 16 (D + 1) + 48 B per locus of the matrix, 2 D B more, 24 D B with q, 12 D B with a
 * prior, and 1 B per cell; on CELLECTOR_ENOMEM the ctx is as it was.  With no output past ref asked for only the tallies run.  The EM
 * state is never touched (an interrupted EM loop continues with the same bits) and nothing of the ctx is overwritten.  pass_ms [2],
 * if given, receives the device time of the tally pass and of the table and posterior pass in milliseconds. */
typedef struct {
    double err;           /* 0.01: the allele fraction of a homozygous-reference donor                    */
    double ambient;       /* 0.03: the share of a cell's reads that come from the pool                    */
    double gt_threshold;  /* 0.99: a genotype is called when its posterior exceeds this                   */
    double prior_floor;   /* 0.01: the chance that a stated call is wrong, spread over the three genotypes */
} cellector_donor_genotypes_params;
typedef struct {
    uint64_t cells[64];            /* cells assigned to the donor                         */
    uint64_t loci_with_reads[64];  /* kind != 0                                           */
    uint64_t confirmed[64], filled[64], changed[64], withdrawn[64];  /* kind 1, 2, 3, 4 */
} cellector_donor_genotypes_summary;
cellector_status cellector_donor_genotypes_default_params(cellector_donor_genotypes_params *out);
cellector_status cellector_donor_genotypes(cellector_ctx *ctx, const uint8_t *assign /*[cells]*/,
                                           const float *prior /*[D][total_loci][3] or NULL*/, uint32_t n_donors,
                                           const cellector_donor_genotypes_params *params /*NULL = defaults*/,
                                           uint64_t *cells /*[D + 1]*/, uint64_t *alt /*[D + 1][total_loci]*/,
                                           uint64_t *ref /*[D + 1][total_loci]*/, double *q /*[D][total_loci][3]*/,
                                           uint8_t *gt_out /*[D][total_loci]*/, uint8_t *kind /*[D][total_loci]*/,
                                           cellector_donor_genotypes_summary *summary, double *tab /*[total_loci][3][2]*/,
                                           double *pass_ms /*[2]*/); /* any output may be NULL */

/* ---- load_mtx_final (load_data.rs:109-132): per-locus allele tallies over ALL loci split by the
 * current exclusion set, for output_final_vcf (main.rs:52-131).  This shard's cells only; sum
 * across shards on the host. */
cellector_status cellector_final_allele_tallies(cellector_ctx *ctx, uint64_t *alt_min, uint64_t *ref_min,
                                                uint64_t *alt_maj, uint64_t *ref_maj /*[total_loci]*/);

/* layout facts of the loaded shard (benchmark accounting) */
typedef struct {
    uint64_t engine;
    uint64_t nnz_regular;   /* entries with 1 <= alt+ref <= 4: handled by table lookup in the tiled passes */
    uint64_t nnz_overflow;  /* the rest: evaluated individually                                           */
    uint64_t tile_bytes;    /* bytes of the tiled cell-pass layout                                        */
    uint64_t cell_blocks, locus_chunks, chunk_groups;
    uint64_t tile_lookups;  /* table lookups one pass of the tile kernel performs: the regular entries plus the padding
                               of the sliced-ELLPACK rows (each lookup = one or two 8-byte LDS reads)              */
} cellector_engine_info_t;
cellector_status cellector_engine_info(const cellector_ctx *ctx, cellector_engine_info_t *out);

/* ---- the order statistics by themselves ----------------------------------------------------- */
/* Median, interquartile range and threshold (statrs Data::median / quantile and main.rs:324-329) of n caller-supplied keys
 * (host array, no NaN): what the scoring loop computes from the normalised log-likelihoods, as a call of its own (tests of the
 * select on keys no run produces; no matrix needs to be loaded).  A multi-device ctx spreads the keys over its shards the
 * way it spreads cells and runs the sharded select (see option sharded_select).  out3 = {median, iqr, threshold}. */
cellector_status cellector_order_statistics(cellector_ctx *ctx, const double *keys, uint64_t n, double iqr_multiple,
                                            double *out3);

/* ---- timing of the dominant kernels (HIP events on the ctx stream; option "timing") ---------- */
typedef enum {
    CELLECTOR_K_CELL_LL = 0,     /* per-cell log-likelihood pass over the CSR  */
    CELLECTOR_K_LOCUS_STATS = 1, /* per-locus pass over the CSC                */
    CELLECTOR_K_SELECT = 2,      /* order statistics                           */
    CELLECTOR_K_POSTERIOR = 3,   /* fused 3-distribution pass + posteriors     */
    CELLECTOR_K_TILE_LL = 4,     /* engine 2: the tiled table-lookup kernel alone (inside K_CELL_LL) */
    CELLECTOR_K_CELL_VAR = 5,    /* options cell_variance / normalization: k_var_tables + k_cell_variance (not inside K_CELL_LL; k_zscore not inside) */
    CELLECTOR_K_LOCUS_MOM = 6,   /* option locus_moments: k_lm_count + k_lm_finalize of the loop's pass (not inside K_LOCUS_STATS) */
    CELLECTOR_K_COUNT = 7
} cellector_kernel_id;
cellector_status cellector_kernel_time(cellector_ctx *ctx, cellector_kernel_id which,
                                       double *total_ms, uint64_t *launches);
cellector_status cellector_reset_timing(cellector_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif
