// Internal state of a cellector_ctx (one shard on one GPU) and the launch wrappers that the
// C-ABI layer (ctx_core.cpp, api_*.cpp, cellector_restage.cpp) calls.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/cellector_ffi.h"
// Device memory goes through a small caching layer (dev_cache.cpp): mapping fresh VRAM costs ~30-50 ms per GB on
// this platform once the footprint is large, and the ingest allocates and frees tens of GB of temporaries several times
// over (measured at 2e9 entries: 3.1 s of hipMalloc for 64 GB in the CSR build alone).  Freed blocks of >= 64 MB are kept
// and handed out again to requests of at least half their size; dev_cache_trim() returns them to the driver.
hipError_t dev_cache_malloc(void **p, size_t bytes);
void dev_cache_free(void *p);
void dev_cache_trim(int device = -1);  // -1: the cached blocks of every device
void dev_cache_park(void *p, size_t bytes, int device);  // a fresh, unused hipMalloc block for later requests of its size

// Owner of one block of that cache (dev_alloc below).  It frees the block on destruction, on reset() and when another block
// is moved in over it.  It converts to T* like the raw pointer it replaces: kernel arguments, pointer arithmetic and the
// hipMemcpy* / hipMemsetAsync calls take it as it is.  It cannot be copied, so nothing that forwards arguments by value
// (hipExtLaunchKernelGGL's tuple) or deduces a kernel's template argument from a pointer can take it: pass get() there.
template <typename T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) {
            reset();
            p_ = o.p_;
            o.p_ = nullptr;
        }
        return *this;
    }
    ~DevBuf() { reset(); }
    void reset()
    {
        if (p_) dev_cache_free((void *)p_);
        p_ = nullptr;
    }
    hipError_t alloc(size_t bytes)  // (the block held before is released first)
    {
        reset();
        void *q = nullptr;
        const hipError_t e = dev_cache_malloc(&q, bytes);
        if (e == hipSuccess) p_ = static_cast<T *>(q);
        return e;
    }
    T *get() const { return p_; }
    operator T *() const { return p_; }

private:
    T *p_ = nullptr;
};

#include "comm.h"

// ---- packed matrix entry -------------------------------------------------------------------
// CSR (by cell):  bits 0..31 compact locus index, 32..47 alt count, 48..63 ref count
// CSC (by locus): bits 0..31 local cell index,    32..47 alt count, 48..63 ref count
#define ENT_IDX(e) ((uint32_t)((e) & 0xffffffffull))
#define ENT_ALT(e) ((uint32_t)(((e) >> 32) & 0xffffull))
#define ENT_REF(e) ((uint32_t)((e) >> 48))
#define CELLECTOR_MAX_COUNT 65535u

// LOCUS exchange buffer layout (f64): 5 planes of L then 8 counters
enum { LB_CONTRIB_MIN = 0, LB_CONTRIB_MAJ = 1, LB_CELLS_MIN = 2, LB_ALT_MIN = 3, LB_REF_MIN = 4, LB_PLANES = 5 };
enum { LC_N_NEW = 0, LC_N_RESCUED = 1, LC_N_EXCLUDED = 2, LC_N_NEAR = 3 /* cells within the near-tie band of the threshold */,
       LC_COUNTERS = 8 };
#define CELLECTOR_NEAR_TIE_REL 1e-9  // |norm - thr| <= band * max(1, |thr|) counts as a near-tie (cellector_iter_summary); the band's floor
// PASS1 exchange buffer layout (f64): 5 planes of total_loci
enum { P1_CELLS_REF = 0, P1_CELLS_ALT = 1, P1_SUM_REF = 2, P1_SUM_ALT = 3, P1_ENTRIES = 4, P1_PLANES = 5 };

// d_counters slots (u32)
enum { DC_N_FILTERED = 0, DC_N_MIN = 4 /* members of this shard's new exclusion set (k_flag) */,
       DC_N_ADD = 5 /* ... of them not in the old set (k_flag's change list, front) */,
       DC_N_RES = 6 /* cells of the old set not in the new one (rescued; the change list's back end) */ };

#define T_ROWS_PER_TILE 1024  // rows (cells) of a tile of the tiled layout (= T_BC in tiled.h)
#define CELLECTOR_TILE_WORK_STRIDE 64  // column counters per table set of the persistent tile kernel (= T_GROUPS_MAX)

#define LF_TABLE_N 171  // ln(FCACHE[0..170]) — statrs ln_factorial cache, SURVEY Appendix B.2

struct KernelTimer {
    std::vector<hipEvent_t> start, stop;  // pending pairs
    double total_ms = 0.0;
    uint64_t launches = 0;
    uint64_t calls = 0;  // launches seen since the timing level was set (level 3 samples every fourth)
    bool open = false;   // timer_begin recorded a start event for the launch in progress
};

// A staged COO: the entries of a shard before the CSC / CSR build (all loci; cell index local, or global while a multi-device
// text ingest still routes them), in file order.  Move-only, like its buffers.
struct CooView { const uint32_t *locus, *cell; const uint16_t *alt, *ref; uint64_t n; };  // not owning: for offset pointers
struct StagedCoo {
    DevBuf<uint32_t> locus, cell;
    DevBuf<uint16_t> alt, ref;
    uint64_t n = 0;
    bool sorted = false;  // locus-major
    cellector_status alloc(cellector_ctx *c, uint64_t n_entries);  // the four arrays for n_entries (defined behind dev_alloc)
    void reset() { locus.reset(); cell.reset(); alt.reset(); ref.reset(); n = 0; }
    CooView view() const { return {locus, cell, alt, ref, n}; }
    // m entries of src (on src_dev) to entry `at` of this one, on the receiving shard c's stream, complete on return
    hipError_t copy_from(const cellector_ctx *c, uint64_t at, const StagedCoo &src, int src_dev, uint64_t m);
};

struct MultiCtx;  // multi.cpp: the shards and worker threads of a ctx made by cellector_create_multi

// ---- the state of a ctx, grouped by lifetime ------------------------------------------------------------------------------
// CtxOptions and the four groups behind it are base structs of cellector_ctx, so the code names every field as c->field.  A group
// is dropped as a whole, by assigning a default-constructed one: its device buffers go back to the cache, every other field returns
// to its default.  READY -> STAGED (drop_built: cellector_restage, _combine, _add_doublets) drops CtxBuilt, CtxTiled and CtxCarry;
// a reload (begin_ingest) drops those and CtxStaged.  A field goes where its lifetime is: nothing is saved around a drop, and what
// outlives a reload (the options, the caller's PASS1 binding, streams, workspaces) is in none of the four.

// the caller's option values (cellector_set_option, cellector_set_shard): kept across reloads
struct CtxOptions {
    int engine = 2;   // option "engine": 1 = v1 CSR/CSC kernels, 2 = tiled (default)
    int overlap = 1;  // option "overlap": 1 = the overflow kernels run on the side stream next to the tile kernel, 0 = in front
    bool compute_expected = true;
    bool ref_arith = false;  // option ref_arith (engine 1): evaluate stats.rs:41-53 with ln_gamma differences, the reference's own rounding
    bool gz_device = false;        // option gz_device: a BGZF .gz input stays compressed on the host and is inflated on the device
    int64_t parse_window_opt = 0;  // option parse_window: 0 = whole file below 1 GB, 256 MB windows above; else the window in bytes
    int64_t write_window_opt = 0;  // option write_window: entries per window of cellector_write_mtx / _format_mtx; 0 = 2^23
    bool fuse_filter = true;   // option "fuse_filter": an unsharded ctx applies the -80 locus filter inside k_locus_finalize (A/B)
    bool tally_delta = true;    // option "tally_delta": engine 2 keeps the exclusion set's per-(locus, code) counts across
                                // iterations and updates them from the set's change (0: recounts every iteration; A/B)
    bool class_delta = true;    // option "class_delta": cellector_refine_classes updates the class tallies from the cells that moved
                                // between two steps (0: recounts every step; A/B)
    bool bank_order = true;  // option "bank_order": the tile builder orders every row's entries against LDS bank conflicts (tile_bank_order)
    int tile_groups_opt = 0;  // option tile_groups: 0 = chosen per matrix (tile_groups_for), else forced (multiple of 8)
    int tile_sb_opt = 0;  // option tile_sb: 0 = cell blocks per column of the tile kernel chosen per launch (tile_geometry), 2 or 4 forced (tests)
    // option sharded_select: a ctx with a communicator exchanges digit histograms (1) or all-gathers NORM (0); -1 = by the
    // number of ranks (use_sharded_select)
    int sharded_select = -1;
    bool norm_zero = true;  // option: clear the other shards' slices of NORM before the cell pass (needed by a sum exchange)
    int timing = 0;  // 0 off, 1 every timed region, 2 only the dominant kernel of the engine, 3 ... around every fourth launch
    bool keep_coo = true;
    int synth_continue_pct = 30;  // option synth_continue_pct: the synthetic generator's n = 1 + Geometric(1 - pct/100)
    // option resolve_ties (kernels_resolve.hip; single device): 0 off, 1 the cells next to an order statistic or the
    // threshold get the reference's arithmetic, 2 every cell does (diagnostic).  Buffers made on first use.
    int resolve_ties = 0;
    // option resolve_posteriors (kernels_assign.hip; single device): cellector_assign evaluates the cells whose label or qual
    // could differ from the reference's (1) or every cell (2) with the reference's arithmetic.  0 off.
    int resolve_posteriors = 0;
    // option cell_variance (kernels_variance.hip): every cell pass of the loop also forms expected_log_variances (main.rs:587)
    bool cell_variance = false;
    // option normalization: 0 = ll / loci_used (main.rs:316), 1 = the z-score of main.rs:317-318 (implies the variance pass);
    // read by em_begin
    int normalization = 0;
    // option locus_moments (kernels_locus_moments.hip; single device, all cells): cellector_em_threshold also forms the per-locus
    // expected contribution and variance of the new exclusion set and of the rest
    bool locus_moments = false;
    int side_lds = -1;               // option "side_lds": dynamic LDS bytes requested by the cell-side overflow kernel (residency
                                     // throttle; -1 = automatic)
    int ovf_deep_opt = -1;           // option "ovf_deep": -1 = decided per matrix (tiled_build), 0 / 1 = forced
    bool ovf_deep_wide = true;       // option "ovf_deep_wide": deep form with 16 lanes per row (0: a thread per row; A/B)
    int t2_opt = -1;                 // option "t2": -1 = decided per matrix (tiled_build: on unless the matrix is ovf_deep), 0 / 1 = forced
    int t2_waves = 0;                // option "t2_waves": one-wave blocks of k_t2_cell when it runs beside the tile kernel; 0 = automatic
                                     // (512, or 256 beside a helper grid)
    int t2_helper = -1;              // option "t2_helper": blocks of k_t2_cell's helper grid per CU the tile grid leaves free; -1 = automatic
                                     // (EM pass only), 0 = none, n = forced, on one CU's worth when none is free (tests)
    int t2_cache = -1;               // option "t2_cache": the EM pass' tier-2 lookups keep their values per entry (t2_val) and gather
                                     // again only at loci whose (alpha, beta) bits moved; 0 = off, 1 = on, -1 = automatic (t2_cache_on)
    int t2_fill = -1;                // option "t2_fill": what a caching pass does with dirty loci: 1 = gather and store (fill), 0 = gather
                                     // without storing (bypass), -1 = decided on the device from the loci that moved since the last pass
    int t2_tiles_opt = -1;           // option "t2_tiles":-1 = automatic (8 on an ovf_deep matrix), 0 = off, 6 / 8 = totals 5..6 / 5..8
    int c4_bits_opt = 0;             // option "compact_bits": 0 = automatic, 32 = force the 32-bit entries
    int locus_mode = 0;              // option "locus_mode": 0 = chosen on the device per iteration, 1 = stream the compact CSC,
                                     // 2 = minority-driven tally over the by-cell CSR
    // the cell range cellector_set_shard asked for (default: all cells); every ingest clamps it to its matrix (cell_begin, cell_end)
    uint64_t req_cell_begin = 0, req_cell_end = UINT64_MAX;
};

// what a staging call makes: an ingest from outside, or cellector_restage / _combine / _add_doublets on the entries held
struct CtxStaged {
    // dims
    uint64_t total_loci = 0, total_cells = 0, nloc = 0;
    enum { ST_EMPTY, ST_STAGED, ST_READY } state = ST_EMPTY;
    // this shard's cells: the requested range, the communicator's or all of them (ingest_all_cells), clamped to the matrix
    uint64_t cell_begin = 0, cell_end = UINT64_MAX;

    StagedCoo coo;  // staged COO of this shard (all loci; cell index local)

    // PASS1 exchange buffer: the library's own or the one the caller bound (pass1_bound); the staged matrix uses n_pass1 values of it
    double *x_pass1 = nullptr;
    DevBuf<double> x_pass1_own;
    uint64_t n_pass1 = 0;

    // cellector_cell_origin: per current cell its index in the matrix of the last ingest from outside; null = identity
    // (cellector_restage composes it)
    DevBuf<uint32_t> cell_origin;
    // cellector_cell_source: per current cell 0 = from the last ingest from outside, k = brought in by the k-th cellector_combine
    // since; null = all 0.  n_combines counts the combines since that ingest (at most 255)
    DevBuf<uint8_t> cell_source;
    uint32_t n_combines = 0;
};

// what cellector_ingest_finish builds from the staged matrix, and what later calls make from that
struct CtxBuilt {
    uint64_t L = 0, nnz = 0;  // used loci, their entries

    // matrix
    DevBuf<uint64_t> csr_ptr, csr_ent;   // [nloc+1], [nnz]
    DevBuf<uint64_t> csc_ptr, csc_ent;   // [L+1], [nnz]
    DevBuf<uint64_t> locus_ids;          // [L]
    DevBuf<double> s_alt, s_ref, n_ent;  // [L] global totals
    DevBuf<uint64_t> to_used;            // [total_loci] compact index or ~0

    // per-locus loop state
    DevBuf<double2> ab;    // [L] alpha,beta for the running pass; alpha < 0 => locus masked
    DevBuf<double> ab6;    // [8L] posterior alpha/beta sets (min, maj, dbl, pad)
    DevBuf<uint8_t> mask;  // [L] loci_used for the current iteration
    DevBuf<uint8_t> mask_next;
    // per-cell state
    DevBuf<uint8_t> flags, flags_new;  // [nloc] exclusion set
    DevBuf<double> ll, ell, nloci;     // [nloc]
    DevBuf<double> post;               // [4*nloc] posterior, doublet, ll_maj, ll_min
    DevBuf<double> var;                // [nloc] expected_log_variances of the last cell pass that formed them (made on first use)
    DevBuf<double> var_tab;            // [L][18] that pass' per-locus variances of the totals 0..17, then [L][4] a compact copy of 1..4 (k_var_tables)
    // locus moments (kernels_locus_moments.hip), made on first use.  Static per matrix (cache, not state):
    bool lm_static_ready = false;
    DevBuf<uint32_t> lm_hist_all;      // [L][18] entries per (locus, total 0..17), all cells
    DevBuf<uint64_t> lm_far_ptr;       // [L+1] the locus' segment of lm_far_ent
    DevBuf<uint64_t> lm_far_ent;       // the entries with a total above 17: local cell << 32 | total; by locus, ascending cell inside
    uint64_t lm_far_n = 0;
    // ... and the loop's pass (option locus_moments):
    DevBuf<uint32_t> lm_hist_min;      // [L][18] ... of the cells of the new exclusion set
    DevBuf<double> lm_out;             // [4][L] expected minority / majority, variance minority / majority of the last pass

    // NORM / LOCUS exchange buffers: the library's own (x_*_own) or one the caller bound (forgotten with the built matrix)
    double *x_norm = nullptr, *x_locus = nullptr;
    DevBuf<double> x_norm_own, x_locus_own;
    uint64_t n_norm = 0, n_locus = 0;

    double near_rel = CELLECTOR_NEAR_TIE_REL;  // near-tie band of this matrix, relative to max(1, |threshold|) (cellector_ingest_finish)
    // option resolve_ties (kernels_resolve.hip)
    DevBuf<uint64_t> res_ent;   // [nnz] csr_ent's rows in file order (the ingest builds it when the option is set)
    uint64_t res_nnz = 0;
    DevBuf<uint32_t> res_cand;  // [nloc] candidate cells
    DevBuf<double> res_key;     // [nloc] their device keys
    DevBuf<uint8_t> res_done;   // [nloc] evaluated in the order-statistic bands
    uint64_t res_n = 0;         // cells the three were made for
    // option resolve_posteriors (kernels_assign.hip): made by the first cellector_assign that resolves
    DevBuf<double> pa_sdbl;     // [nloc] the doublet set's per-cell sum of the last posterior phase (the mark kernel reads it)
    DevBuf<uint32_t> pa_cand;   // [nloc] cells to evaluate
    DevBuf<double> pa_den;      // [3][L] log_beta_calc(alpha_s, beta_s) of the three posterior sets
    DevBuf<double> pa_ll;       // [3][n evaluated] minority, majority, doublet LL in the reference's arithmetic
    uint64_t pa_ll_cap = 0;

    // iteration bookkeeping
    uint64_t iteration = 0;
    uint64_t n_excluded_global = 0;
    double last_median = 0, last_iqr = 0, last_thr = 0;
    bool have_iter = false;
    uint64_t n_masked_loci = 0;
};

// ---- engine v2: table-driven tiled layout: what tiled_build (kernels_tiled_build.hip) makes for the passes of kernels_tiled.hip ----
struct CtxTiled {
    bool tiled_ready = false;
    uint32_t t_nb = 0, t_nj = 0, t_groups = 0, t_cpg = 0;  // cell blocks, locus chunks, chunk groups, chunks/group
    uint64_t t_npad = 0;             // nb * T_BC
    DevBuf<uint64_t> tile_ptr;       // [nb*nj+1] offsets into tiles, in u16 elements (multiples of 128)
    DevBuf<uint16_t> tiles;          // SELL-64-1024 slices: per tile 16 slices of 64 rows of K u16 entries and their cell ids (tiled.h: tile_entry)
    DevBuf<uint16_t> thdr;           // [nb*nj][T_HDR] tile headers: 16 x {first u16 of the slice, K}
    uint64_t t_elems = 0;            // entries (u16) in the stream, padding included
    double *tab_em = nullptr;        // table the last EM cell pass built, inside tab (the locus pass reads its log-pmfs)
    int tab_em_stride = 1;           // 2 when that table holds (log-pmf, expected) pairs
    DevBuf<uint64_t> ovf_ptr, ovf_ent;  // overflow CSR (alt+ref == 0 or > 4), packed like csr_ent
    uint64_t ovf_n = 0;
    DevBuf<double> ovf_tab;          // [L][128] per-locus cumulative-log / expected tables for overflow entries
    DevBuf<double> ovf_etab;         // [L][8] alpha, beta, E(n) for n = 5..8, pad: the cell side's 64-byte record per locus
    bool ovf_deep = false;           // the overflow entries are a large share of the matrix (deep coverage): their cell side runs
                                     // the full form of the direct kernel (totals up to 17 in one kernel), never throttled
    DevBuf<double> ovf_lp;           // [ovf_n] shallow coverage: the EM pass' overflow log-pmfs, by-locus order (k_ovf_values -> k_locus_finalize)
    DevBuf<uint32_t> ovc_locus;      // [ovf_n] compact locus index of every overflow entry, by-locus order (k_ovf_values)
    DevBuf<double> ovf_sum;          // [3][2][nloc] per-cell sums of the overflow values (ll, expected) per table set
    DevBuf<uint64_t> ovf_ell_ptr, ovf_ell;  // 64-row ELLPACK copy of the overflow CSR (cell side): [groups+1], slots
    DevBuf<uint32_t> ovf_tier_row[2];  // the overflow entries with alt+ref in 9..17 (tier 0) / above (tier 1):
    DevBuf<uint64_t> ovf_tier_ent[2];  //   their rows and packed entries, in row order
    uint64_t ovf_n_tier[2] = {0, 0};
    DevBuf<double> ovf_tier_val;     // [2][ovf_n_tier[1]] per pass: log-pmf / expected term of the tier-1 entries (k_ovf_listed_values)
    DevBuf<uint32_t> ovf_nmask;      // [L] which alt+ref totals (4..17) occur among the locus' overflow entries
    // tier 2 (kernels_tiled.hip, k_t2_tables): the overflow entries with totals 5..8 are table-driven as well
    bool t2 = false;
    DevBuf<uint32_t> hist_all2;      // [L][32] tier-2 entries per (locus, pair), all cells of the shard (static)
    DevBuf<uint32_t> t2_plist, t2_slist;  // the pairs (locus << 5 | pair) / table sectors (locus << 3 | sector) that occur, locus order (static)
    uint32_t t2_np = 0, t2_ns = 0;
    DevBuf<uint32_t> t2_pmask;       // [L] bit c2: the pair occurs at the locus (static)
    DevBuf<uint32_t> cnt2;           // [L][32] ... of the cells of the exclusion set (k_t2_minority; kept across iterations, see tally_valid)
    DevBuf<double> tab2;             // [L][48] per pass: log-pmfs of the pairs that occur + expected terms, six 64-byte sectors per locus
    // the EM pass' lookup values kept per entry (option t2_cache; k_t2_cell<.., CACHE>): made with the ELLPACK copy, gone with it
    uint64_t ovf_ell_slots = 0;      // slots of ovf_ell
    DevBuf<double2> t2_val;          // [ovf_ell_slots] (log-pmf, expected term) per slot of ovf_ell, same layout; 0 where no tier-2 entry
    DevBuf<double2> ab_t2;           // [L] the (alpha, beta) bits a locus' kept values were written under (all-ones: none yet)
    DevBuf<double2> ab_last;         // [L] the (alpha, beta) bits of the last caching pass (the fill rule counts what moved since)
    DevBuf<uint32_t> t2_dirty;       // [(L + 63) / 64 * 2] bit l: ab differs from ab_t2 in this pass (k_t2_tables writes every word)
    bool t2_val_exp = false;         // every kept value has its expected term (a pass without the column stores none)
    // tier-2 TILES (deep coverage; tiled.h, geo_t2): the cell side of the totals 5..t2_tiles walks a second tile set with
    // its own chunk tables in LDS instead of evaluating those entries one by one (k_ovf_cell_wide keeps the other totals)
    int t2_tiles = 0;                // 0, 6 or 8: in use (tiled_build)
    uint32_t t2_nj = 0, t2_groups = 0, t2_cpg = 0;  // chunks of geo_t2::BLU loci, chunk groups, chunks per group
    DevBuf<uint64_t> tile2_ptr;      // [nb * t2_nj + 1]
    DevBuf<uint16_t> tiles2, thdr2;
    DevBuf<double> tab2c;            // [t2_nj][geo_t2::BL][geo_t2::LROW] per pass: the chunked tier-2 tables (+ tail pad)
    DevBuf<double> part2;            // [3][2][t2_groups][npad] per-group partial sums of the tier-2 tile passes
    DevBuf<uint32_t> tile_work2;     // [T_GROUPS_MAX] column counters of a tier-2 tile pass
    DevBuf<uint64_t> ovr_ptr, ovr_ent;  // by-cell CSR of the overflow entries the tier-2 tiles leave out (totals 0, above t2_tiles)
    uint64_t ovr_n = 0;
    DevBuf<uint64_t> ovx_ptr, ovx_ent;  // by-locus CSC of the overflow entries outside tier 2 (totals 0 and above 8)
    DevBuf<uint32_t> ovx_locus;      // [ovx_n] their compact locus index
    DevBuf<double> ovx_lp;           // [ovx_n] the EM pass' log-pmfs of those entries (k_ovx_values -> k_locus_finalize)
    uint64_t ovx_n = 0;
    DevBuf<uint64_t> c4_ptr;         // [L+1] compact CSC of regular entries
    DevBuf<uint32_t> c4_ent;         // 32-bit entries cell_local | code << 28, or 24-bit cell | code << 20 (c4_bits)
    int c4_bits = 32;
    DevBuf<uint64_t> ovc_ptr, ovc_ent;  // overflow CSC, packed like csc_ent
    DevBuf<uint32_t> hist_all;       // [L][14] regular entries per code
    DevBuf<double> tab;              // [3 + 2][nj][15][384] log-pmf tables of the posterior sets, then the EM pass' (log-pmf, expected) pairs
    DevBuf<double> part;             // [3][2][groups][npad] per-group partial sums (ll, ell)
    DevBuf<double2> ab3;             // [3][L] posterior alpha/beta sets as double2
    DevBuf<uint32_t> masked_cnt;     // [nloc] entries of the cell at masked loci
    DevBuf<uint32_t> flag_bits;      // [ceil(nloc/32)] new exclusion set as a bitmask
    DevBuf<uint32_t> tile_work;      // [3][T_GROUPS_MAX] column counters of the persistent tile kernel, one set per table set
    DevBuf<uint32_t> minlist;        // [nloc] local ids of the cells of the new exclusion set (arbitrary order)
    DevBuf<uint32_t> chg;            // [nloc] the set's change (k_flag): newly excluded cells from the front, rescued ones from the back
    DevBuf<uint32_t> tally;          // [L][16] regular entries of the exclusion set's cells per (locus, code), u32 (kept across iterations)
    DevBuf<uint32_t> hist_min;       // [2 * lr_sub][L][16] u16 partial planes of this iteration's counts (k_minority_ranges)
    DevBuf<uint32_t> mroff;          // [R+1][mroff_cap] the excluded cells' offset rows, transposed (per iteration)
    DevBuf<uint64_t> mbeg;           // [mroff_cap] start of the excluded cells' rows in csr_ent
    uint64_t mroff_cap = 0;
    uint32_t lr_sub = 1;             // subsets of the exclusion set = partial planes of hist_min
    uint32_t lr_cap = 32767;         // cells of a subset: 65535 / (most entries of a cell at one locus), at most 32767 (u16 counters)
    DevBuf<uint16_t> c4r;            // [nnz] compact by-cell entries: locus inside its 4096-locus range | code << 12 (code 15: overflow entry)
    DevBuf<uint32_t> roff;           // [nloc][R+1] offsets of the locus ranges inside each by-cell CSR row
};

// what one call leaves for the next
struct CtxCarry {
    int em_phase = 0;  // 0 idle, 1 after begin, 2 after threshold
    bool tables_prebuilt = false;    // the next iteration's k_build_tables is already queued / done (em_finish)
    bool prebuilt_expected = false;  // ... with this value of compute_expected
    bool work_zeroed = false;        // tile_work was reset by this iteration's k_alpha_beta
    bool cell_join_pending = false;  // the main stream still has to wait for the side stream's cell-side overflow sums (ev_join)
    bool ovf_locus_pending = false;  // the side stream still owes this iteration's locus-side overflow tables / values (event ev_join2)
    bool tab_event_valid = false;    // ev_tab marks the table kernel queued ahead by em_finish, and nothing the side stream
                                     // depends on has been queued behind it since
    bool filter_fused = false;  // this iteration's locus pass applied the locus filter (em_finish then launches no k_locus_filter);
                                // cleared by em_finish, a reload, em_begin and the engine option
    bool tally_valid = false;   // tally / cnt2 hold the counts of the current exclusion set (flags): set by em_finish, cleared by
                                // the locus pass (until its flag swap), a reload and an engine switch
    int res_last_mode = 0;      // resolve_ties of the last iteration (cellector_iter_resolution)
    bool iter_var = false;      // the iteration in flight formed c->var (em_begin)
    bool var_formed = false;    // ... and so did the last finished one (cellector_iter_cell_variances); cleared by em_reset
    bool iter_lm = false;       // the iteration in flight formed c->lm_out (em_threshold)
    bool lm_formed = false;     // ... and so did the last finished one (cellector_iter_locus_moments); cleared by em_reset
    // what the last cellector_assign resolved (cellector_assign_resolution / _resolved_cells)
    int pa_last_mode = 0;
    uint64_t pa_labels_changed = 0, pa_qual_changed = 0;
    std::vector<uint32_t> pa_ids;
};

struct cellector_ctx : CtxOptions, CtxStaged, CtxBuilt, CtxTiled, CtxCarry {
    // a ROOT ctx (cellector_create_multi with more than one shard) owns no device state of its own: every entry point
    // fans out to its shards (multi.cpp) and returns arrays in global cell order
    MultiCtx *multi = nullptr;
    // the exchange transport of a shard that is part of a sharded run (n = 1: single shard, nothing is exchanged)
    Comm comm;
    bool owns_stream = false;  // the stream was created by the library (a shard of a root ctx)
    bool ingest_all_cells = false;  // begin_ingest: this shard stages ALL cells for now (multi-device text ingest parses once)
    int device = 0;
    int n_cu = 256;  // the device's compute units (read once, with the device): persistent grids are sized by it
    hipStream_t stream = nullptr;
    // side stream for the small overflow kernels that run next to the tile kernel (fork/join with events)
    hipStream_t side = nullptr;
    hipStream_t side2 = nullptr;  // ... and one for the helper grid of the tier-2 lookups, which runs BESIDE the side stream's grid
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_join2 = nullptr, ev_sum = nullptr;
    hipEvent_t ev_t2tab = nullptr, ev_help = nullptr;  // k_t2_tables done (rides on its dispatch) -> helper grid -> its end (side stream waits)
    hipEvent_t ev_tab = nullptr;   // completion of the table kernel queued ahead by em_finish, attached to its dispatch (no barrier packet)
    mutable std::string err;
    // the PASS1 buffer the caller bound (cellector_bind_exchange_buffer) and its capacity in f64 values; null = none.  It outlives
    // reloads: begin_ingest points x_pass1 at it again
    double *pass1_bound = nullptr;
    uint64_t pass1_bound_cap = 0;

    DevBuf<double> lf;            // [LF_TABLE_N] ln factorial table
    DevBuf<uint32_t> d_counters;  // [8] device scratch counters
    DevBuf<uint32_t> t2_ctr;      // [T2_CTR_N] [0..2] next 64-row group of the tier-2 lookups, per table set (reset by k_t2_tables);
                                  // [4 + 2p], [5 + 2p] dirty loci / loci moved since the last pass, of the caching passes of parity p
                                  // (a pass' k_t2_tables adds to its own pair and clears the other)
    uint32_t t2_pass = 0;         // caching passes launched so far
    // cellector_assign's host arrays, kept between calls: a device-to-host copy into memory the process has not touched
    // before costs milliseconds, into a buffer used before microseconds
    struct AssignHost {
        std::vector<double> p, d, lmaj, lmin;
        std::vector<uint8_t> excl, pa;
        std::vector<uint32_t> ent;
        std::vector<uint64_t> q;
    } pa_host;
    DevBuf<uint32_t> pa_cnt;      // [2] resolve_posteriors: candidates, the evaluation kernel's cell counter
    DevBuf<uint32_t> res_cnt;     // [4] resolve_ties: band candidates, threshold-band candidates, changed flags, changed-summary bits
    DevBuf<double> res_dev;       // [4] the device keys' median, iqr, threshold

    // order-statistic workspace
    DevBuf<uint32_t> sel_hist;    // [4096] top-bits histogram, [SEL_T][1024] next-bits histograms, [1] list length (+ pad)
    DevBuf<uint64_t> sel_state;   // [2][SEL_T][2] prefix, remaining rank after the first / second step
    DevBuf<uint64_t> sel_list;    // keys that carry a target's 22-bit prefix (capacity: all keys)
    uint64_t sel_list_cap = 0;
    DevBuf<double> sel_out;       // [16] device: [0..5] order statistics, [8..10] median, iqr, threshold
    DevBuf<uint32_t> seld_hist;   // sharded run: [6 levels][SEL_T][2048] digit histograms (select_threshold_sharded), made on first use
    DevBuf<uint64_t> seld_state;  // ... [7][SEL_T][2] prefix, remaining rank before / after every level
    double *h_sel = nullptr;      // pinned [32]: iteration summary written by k_iter_summary, read in em_finish
    double *h_sum_dev = nullptr;  // the device's address of h_sel
    uint64_t sum_seq = 0;         // number of summaries queued; h_sel[CELLECTOR_SUM_SEQ] = the last one that arrived

    KernelTimer timers[CELLECTOR_K_COUNT];
    std::vector<hipEvent_t> ev_pool;  // collected timer events, reused (creating a pair costs microseconds before a launch)
};

// READY -> STAGED, and the first half of a reload: what was built from the staged matrix goes as a whole
inline void drop_built(cellector_ctx *c)
{
    static_cast<CtxCarry &>(*c) = CtxCarry();
    static_cast<CtxTiled &>(*c) = CtxTiled();
    static_cast<CtxBuilt &>(*c) = CtxBuilt();
}

// A reload (and cellector_destroy) drops what was built and what was staged, each group as a whole.
static inline void drop_matrix(cellector_ctx *c)
{
    drop_built(c);
    static_cast<CtxStaged &>(*c) = CtxStaged();
}

// what cellector_cell_log_likelihoods invalidates, for the calls that run beside the EM state on scratch of their own
inline void invalidate_cell_ll_state(cellector_ctx *c)
{
    c->tables_prebuilt = false;
    c->work_zeroed = false;
}

#define SEL_T 6
#define T2_CTR_N 8
#define CELLECTOR_SUM_SEQ 31
#define CELLECTOR_SEL_HIST_WORDS (4096 + SEL_T * 1024 + 64)

// ---- error plumbing ---------------------------------------------------------------------------
cellector_status ctx_fail(const cellector_ctx *c, cellector_status s, const char *fmt, ...);
#define HIPCHK(c, expr)                                                                          \
    do {                                                                                         \
        hipError_t e__ = (expr);                                                                 \
        if (e__ != hipSuccess)                                                                   \
            return ctx_fail((c), CELLECTOR_EDEVICE, "%s failed: %s (%s:%d)", #expr,              \
                            hipGetErrorString(e__), __FILE__, __LINE__);                         \
    } while (0)
#define CHK(expr)                                                                                \
    do {                                                                                         \
        cellector_status s__ = (expr);                                                           \
        if (s__ != CELLECTOR_OK) return s__;                                                     \
    } while (0)

#define REQUIRE(c, cond, msg)                                        \
    do {                                                             \
        if (!(cond)) return ctx_fail((c), CELLECTOR_EINVAL, "%s", msg); \
    } while (0)
#define SETDEV(c) HIPCHK((c), hipSetDevice((c)->device))

static inline cellector_status d2h(const cellector_ctx *c, void *dst, const void *src, size_t bytes)
{
    if (!bytes) return CELLECTOR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CELLECTOR_OK;
}

// n elements of T into *p (the block *p held before is released first)
template <typename T>
static inline cellector_status dev_alloc(cellector_ctx *c, DevBuf<T> *p, uint64_t n)
{
    hipError_t e = p->alloc((n ? n : 1) * sizeof(T));
    if (e != hipSuccess)
        return ctx_fail(c, CELLECTOR_ENOMEM, "hipMalloc(%llu bytes) failed: %s",
                        (unsigned long long)(n * sizeof(T)), hipGetErrorString(e));
    return CELLECTOR_OK;
}

// Device-to-device copy between two shards (one device, or peers) on the RECEIVING shard's stream, complete on return.  (On the
// null stream such a copy may return before it is done, and the shards' non-blocking streams do not order against that stream:
// a kernel launched right behind it could read stale bytes.)
static inline hipError_t dev_copy_sync(hipStream_t st, void *dst, int dst_dev, const void *src, int src_dev, size_t bytes)
{
    if (!bytes) return hipSuccess;
    hipError_t e = dst_dev == src_dev ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st)
                                      : hipMemcpyPeerAsync(dst, dst_dev, src, src_dev, bytes, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e;
}

inline cellector_status StagedCoo::alloc(cellector_ctx *c, uint64_t n_entries)
{
    n = n_entries;
    CHK(dev_alloc(c, &locus, n)); CHK(dev_alloc(c, &cell, n));
    CHK(dev_alloc(c, &alt, n)); CHK(dev_alloc(c, &ref, n));
    return CELLECTOR_OK;
}
inline hipError_t StagedCoo::copy_from(const cellector_ctx *c, uint64_t at, const StagedCoo &src, int src_dev, uint64_t m)
{
    hipError_t e = dev_copy_sync(c->stream, locus + at, c->device, src.locus, src_dev, m * 4);
    if (e == hipSuccess) e = dev_copy_sync(c->stream, cell + at, c->device, src.cell, src_dev, m * 4);
    if (e == hipSuccess) e = dev_copy_sync(c->stream, alt + at, c->device, src.alt, src_dev, m * 2);
    if (e == hipSuccess) e = dev_copy_sync(c->stream, ref + at, c->device, src.ref, src_dev, m * 2);
    return e;
}

// ---- timing -----------------------------------------------------------------------------------
struct LapTimer {  // CELLECTOR_TIMING=1: phase wall times of the ingest on stderr; lap() = seconds since the last one
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    double lap()
    {
        const auto was = t;
        t = std::chrono::steady_clock::now();
        return std::chrono::duration<double>(t - was).count();
    }
};
struct CallLaps {  // ... and of a re-staging call, under the call's name (every phase ends synchronised)
    const char *call;
    const bool on = getenv("CELLECTOR_TIMING") != nullptr;
    LapTimer t;
    void operator()(const char *what) { if (on) fprintf(stderr, "[timing]   %s: %-22s %8.4f s\n", call, what, t.lap()); }
};
void timer_begin(cellector_ctx *c, int which);
void timer_end(cellector_ctx *c, int which);
bool timer_take(cellector_ctx *c, int which, hipEvent_t *start, hipEvent_t *stop);
void timer_collect(cellector_ctx *c);

// ---- launch wrappers (kernels_*.hip) ------------------------------------------------------------
// EM loop
cellector_status launch_alpha_beta(cellector_ctx *c);
cellector_status launch_cell_ll(cellector_ctx *c, const double2 *ab, double *norm_out /*may be null*/);
cellector_status launch_flag(cellector_ctx *c, const double *d_thr);
cellector_status launch_locus_stats(cellector_ctx *c);
cellector_status launch_locus_filter(cellector_ctx *c);
cellector_status launch_iter_summary(cellector_ctx *c);
cellector_status launch_ab_from_host(cellector_ctx *c, const double *alpha, const double *beta,
                                     const uint8_t *mask);
// sdbl: [nloc] or null — the doublet set's per-cell sums as well (option resolve_posteriors' mark kernel reads them)
cellector_status launch_posteriors(cellector_ctx *c, double mf0, double lp_min, double lp_maj,
                                   double lp_dbl, double *sdbl);
cellector_status launch_ab_posterior_into(cellector_ctx *c, double mf0, double *ab6 /*[8 L] device scratch*/);
// cellector_cell_pmfs on one device (kernels_pmfs.hip): validated ids; scratch of its own, the ctx's state stays
cellector_status pmfs_run(cellector_ctx *c, const double *alpha, const double *beta, const uint8_t *mask, const uint32_t *cells,
                          uint64_t n_cells, uint64_t *rec_ptr, uint64_t capacity, uint32_t *locus_index, uint32_t *alt, uint32_t *ref,
                          double *log_pmf, double *expected_log_pmf, double *expected_log_variance);
// expected_log_variances (kernels_variance.hip): the loop's pass into c->var under c->ab, with zscore also main.rs:317-318 over
// norm_out; and cellector_cell_log_variances on one device, scratch of its own
cellector_status launch_cell_variance(cellector_ctx *c, bool zscore, double *norm_out);
cellector_status variance_run(cellector_ctx *c, const double *alpha, const double *beta, const uint8_t *mask, double *out /*[nloc] host*/);
// locus moments (kernels_locus_moments.hip): the loop's pass into c->lm_out under c->ab and flags_new; cellector_locus_moments
// and cellector_locus_total_counts on one device, scratch of their own (host arrays; out: [L][19])
cellector_status launch_locus_moments(cellector_ctx *c);
cellector_status locus_moments_run(cellector_ctx *c, const double *alpha, const double *beta, const uint8_t *mask, const uint8_t *flags,
                                   double *exp_min, double *exp_maj, double *var_min, double *var_maj);
cellector_status locus_total_counts_run(cellector_ctx *c, const uint8_t *flags, uint32_t *out);
// K-genotype classes (kernels_classes.hip) on one device holding all cells; validated arguments, host arrays, scratch of their own.
// The tallies / alpha-betas of a labelling (any output may be null) ...
cellector_status classes_tallies_run(cellector_ctx *c, const uint8_t *labels, uint32_t K, const double *scale, uint64_t *cells, uint64_t *alt,
                                     uint64_t *ref, double *alpha, double *beta);
// ... and the posterior chain (max_iter 0) or the hard-EM loop over it; labels_out / sum: refine only
cellector_status classes_run(cellector_ctx *c, const uint8_t *labels, uint32_t K, const double *scale, const double *log_prior,
                             const uint8_t *mask, uint32_t max_iter, uint64_t min_loci, uint8_t *labels_out, cellector_refine_summary *sum,
                             double *ll, double *posterior, uint8_t *best, uint64_t *qual);
// ... and with the doublet classes of the K (K - 1) / 2 pairs: the pair distributions of a (labels, held) state, and the chain with
// the call (max_iter 0) or the held-out refine; labels_out / held_out / sum: refine only
cellector_status class_pairs_run(cellector_ctx *c, const uint8_t *labels, const uint8_t *held, uint32_t K, const double *pair_scale,
                                 double *alpha, double *beta);
cellector_status class_doublets_run(cellector_ctx *c, const uint8_t *labels, const uint8_t *held, uint32_t K, const double *scale,
                                    const double *pair_scale, const double *log_prior, const double *log_pair_prior, const uint8_t *mask,
                                    double threshold, uint32_t max_iter, uint64_t min_loci, uint8_t *labels_out, uint8_t *held_out,
                                    cellector_refine_doublets_summary *sum, double *ll, double *ll_pair, double *posterior,
                                    double *doublet_posterior, uint8_t *best, uint8_t *best_pair, uint8_t *call, uint64_t *qual);
// genotype clusters without labels (kernels_cluster.hip) on one device holding all cells; validated arguments, host arrays, scratch
// of their own (the by-locus list included), nothing of the ctx written: one M step + tables, one E step, the annealed EM over R restarts
cellector_status cluster_m_step_run(cellector_ctx *c, const double *w, uint32_t J, const uint8_t *mask, double floor, double *A, double *T,
                                    double *theta, double *tab);
cellector_status cluster_e_step_run(cellector_ctx *c, const double *tab, uint32_t K, uint32_t R, const double *temp, const uint8_t *mask,
                                    double *s, double *w, double *objective);
cellector_status cluster_run(cellector_ctx *c, uint32_t K, uint32_t R, uint64_t seed, const cellector_cluster_params *p, const uint8_t *mask,
                             uint8_t *labels, double *ll, double *posterior, double *theta, double *objective,
                             cellector_cluster_summary *out);
// donor demultiplexing (kernels_donors.hip) on one device holding all cells; validated arguments, host arrays, scratch of their own,
// nothing of the ctx written: the packed genotypes and the tables alone, the cell passes with the posterior chain (log_prior never
// null), the class tallies against the donors
cellector_status donor_tables_run(cellector_ctx *c, const uint8_t *gt, uint32_t D, const cellector_donor_params *prm, const uint8_t *mask,
                                  double *tab1, double *tab2, uint64_t *packed);
cellector_status donor_posteriors_run(cellector_ctx *c, const uint8_t *gt, const float *gp /*or null: then gt*/, uint32_t D, const cellector_donor_params *prm, const double *log_prior,
                                      const uint8_t *anchor, const uint8_t *mask, double log_singlet, double log_pair, double *ll,
                                      double *pair_ll, double *posterior, double *pair_posterior, double *doublet_posterior, uint8_t *best,
                                      uint8_t *second, uint8_t *best_pair, uint32_t *n_entries, uint8_t *status, uint8_t *anchor_out,
                                      cellector_donor_summary *out, double *tab1, double *tab2, uint64_t *packed);
cellector_status donor_match_run(cellector_ctx *c, const uint8_t *labels, uint32_t K, const uint8_t *gt, const float *gp /*or null*/, uint32_t D,
                                 const cellector_donor_params *prm, const uint8_t *mask, double *ll, uint8_t *best, double *margin,
                                 uint64_t *cells);
cellector_status donor_weights_run(cellector_ctx *c, const float *gp /*[D][total_loci][3]*/, uint32_t D, double *w, uint8_t *kind);
cellector_status donor_pack_launch(cellector_ctx *c, uint32_t D, const uint8_t *d_gt /*[D][total_loci]*/, uint64_t *d_packed /*[L][W]*/);
cellector_status donor_tables_launch(cellector_ctx *c, const uint8_t *d_mask /*[L] or null*/, const cellector_donor_params *prm,
                                     double2 *d_tab1 /*[L][4]*/, double2 *d_tab2 /*[L][16]*/);
// donor panels (kernels_donor_panel.hip): the same calls for up to 4096 donors, a shortlist of M pairs per cell; indices are u16
cellector_status donor_panel_run(cellector_ctx *c, const uint8_t *gt, uint32_t D, uint32_t M, const cellector_donor_params *prm,
                                 const double *log_prior, const uint16_t *anchor, const uint8_t *mask, double log_singlet, double log_pair,
                                 uint16_t *cand, double *cand_ll, double *cand_pair_ll, double *cand_posterior, double *cand_pair_posterior,
                                 double *doublet_posterior, double *best_posterior, uint16_t *best, uint16_t *second, uint16_t *best_pair,
                                 uint16_t *anchor_out, uint32_t *n_entries, uint8_t *status, uint64_t *donor_cells,
                                 cellector_donor_panel_summary *out, double *ll, uint64_t *packed, double *tab1, double *tab2);
cellector_status donor_panel_match_run(cellector_ctx *c, const uint8_t *labels, uint32_t K, const uint8_t *gt, uint32_t D,
                                       const cellector_donor_params *prm, const uint8_t *mask, double *ll, uint16_t *best, double *margin,
                                       uint64_t *cells);
// the fit of the called hypothesis: the moment tables alone; the donor call into scratch, then the fit pass, the keys' order statistics
// (select_threshold) and the flags
cellector_status donor_moment_tables_run(cellector_ctx *c, const cellector_donor_params *prm, const uint8_t *mask, double *mom1, double *mom2);
cellector_status donor_fit_run(cellector_ctx *c, const uint8_t *gt, uint32_t D, const cellector_donor_params *prm, const cellector_donor_fit_params *fp,
                               const double *log_prior, const uint8_t *anchor, const uint8_t *mask, double log_singlet, double log_pair,
                               double *fit_e, double *fit_v, double *pair_e, double *pair_v, double *z, double *pair_z, double *call_z,
                               uint8_t *hyp_a, uint8_t *hyp_b, uint8_t *status, uint8_t *unmatched, cellector_donor_fit_summary *out,
                               double *mom1, double *mom2);
// ambient fraction estimation (kernels_ambient.hip) on one device holding all cells; validated arguments, host arrays, scratch of their
// own, nothing of the ctx written: the tables of a grid alone, one profile over a grid, the zooming grid search
cellector_status ambient_tables_run(cellector_ctx *c, const double *rho, uint32_t G, double err, const uint8_t *mask, double *tab);
cellector_status ambient_profile_run(cellector_ctx *c, const uint8_t *gt, uint32_t S, const uint8_t *assign, const double *rho, uint32_t G,
                                     double err, uint64_t min_loci, const uint8_t *mask, double *ll, double *total, double *source_total,
                                     uint64_t *source_cells, uint32_t *n_entries, double *cell_rho, double *cell_se, double *tab);
cellector_status ambient_estimate_run(cellector_ctx *c, const uint8_t *gt, uint32_t S, const uint8_t *assign, const cellector_ambient_params *p,
                                      const uint8_t *mask, cellector_ambient_summary *out, double *cell_rho, double *cell_se,
                                      uint32_t *n_entries);
// donor pair fractions (kernels_pair_fraction.hip) on one device holding all cells; validated arguments, host arrays, scratch of their own
cellector_status pair_fraction_tables_run(cellector_ctx *c, const cellector_donor_params *prm, const double *frac, uint32_t G,
                                          const uint8_t *mask, double *tab);
cellector_status pair_fractions_run(cellector_ctx *c, const uint8_t *gt, uint32_t D, const cellector_donor_params *prm,
                                    const cellector_pair_fraction_params *fp, const uint8_t *pair_a, const uint8_t *pair_b, const double *frac,
                                    uint32_t G, const uint8_t *mask, double *ll, uint32_t *n_entries, double *cell_frac, double *cell_se,
                                    uint8_t *j_star, uint8_t *kind, cellector_pair_fraction_summary *out, double *tab);
cellector_status launch_final_tallies(cellector_ctx *c, uint64_t *d_out /*[4*total_loci]*/);
// the same over the K classes of a labelling (kernels_genotypes.hip): d_lab [nloc] on the device, slot K = the cells labelled 255
cellector_status launch_genotype_tallies(cellector_ctx *c, const uint8_t *d_lab, uint32_t K, uint64_t *d_acc /*[K+1][2][total_loci]*/);
// donor genotype refinement (kernels_donor_genotypes.hip): validated arguments, host arrays, scratch of its own
cellector_status donor_genotypes_run(cellector_ctx *c, const uint8_t *assign, const float *prior, uint32_t D,
                                     const cellector_donor_genotypes_params *p, uint64_t *cells, uint64_t *alt, uint64_t *ref, double *q,
                                     uint8_t *gt_out, uint8_t *kind, cellector_donor_genotypes_summary *summary, double *tab, double *pass_ms);
// placed state (kernels_state.hip): host_flags into c->flags, the set's minority tallies and member count into c->x_locus
cellector_status launch_state_tallies(cellector_ctx *c, const uint8_t *host_flags /*[nloc], 0 / 1*/);
// order statistics: exact values at SEL_T 0-based ranks of n keys
cellector_status select_threshold(cellector_ctx *c, const double *keys, uint64_t n, double iqr_multiple);
cellector_status ffi_order_statistics(cellector_ctx *c, const double *keys, uint64_t n_local, uint64_t n_total, double iqr_multiple,
                                      double *out3);  // (api_em.cpp; a shard's slice of cellector_order_statistics)
// ... over the keys of all shards of a sharded run (this shard holds n_local of the n_total), exchanged as digit histograms
cellector_status select_threshold_sharded(cellector_ctx *c, const double *keys, uint64_t n_local, uint64_t n_total, double iqr_multiple);
// option resolve_ties (kernels_resolve.hip): after select_threshold, before launch_flag
cellector_status resolve_ties(cellector_ctx *c, double iqr_multiple);
cellector_status resolve_build_file_order(cellector_ctx *c);  // (ingest_build, option set)
// option resolve_posteriors (kernels_assign.hip): after a posterior phase that wrote pa_sdbl.  The cells to evaluate
// (mode 1: those whose label or qual could differ; 2: all) and their three LLs in the reference's arithmetic, on the host:
// ids [n], ll3 [3][n] = minority | majority | doublet
cellector_status assign_resolve(cellector_ctx *c, int mode, double threshold, double lp_min, double lp_maj, double lp_dbl,
                                std::vector<uint32_t> *ids, std::vector<double> *ll3);
// ingest
cellector_status ingest_stage_host_coo(cellector_ctx *c, uint64_t nnz, const uint32_t *locus0,
                                       const uint32_t *cell0, const uint32_t *alt, const uint32_t *ref);
cellector_status ingest_pass1(cellector_ctx *c);
// the entries of cells [cb, ce) out of the staged ones of ALL cells (cell index global), into a new COO on c's device: cell
// index made local, order kept; `keep` is caller scratch of all.n + 1 words
cellector_status ingest_split_coo(cellector_ctx *c, const CooView &all, uint64_t cb, uint64_t ce, uint64_t *keep, StagedCoo *out);
cellector_status ingest_cell_histogram(cellector_ctx *c, const uint32_t *d_cell, uint64_t n, uint64_t total_cells, std::vector<uint32_t> *out);
// multi-device text ingest (api_ingest.cpp): stage the whole pair on one shard / hand a shard its routed entries
// the EM state a load leaves, queued on the stream (api_em.cpp): cellector_ingest_finish and cellector_em_reset
__attribute__((visibility("hidden"))) cellector_status em_state_clear(cellector_ctx *c);
cellector_status ffi_stage_mtx_all_cells(cellector_ctx *c, const char *alt_path, const char *ref_path, cellector_ctx *helper);
cellector_status ffi_adopt_staged(cellector_ctx *c, uint64_t total_loci, uint64_t total_cells, StagedCoo &&coo);
cellector_status ingest_build(cellector_ctx *c, uint64_t min_alt, uint64_t min_ref);
// cellector_restage (kernels_restage.hip).  host_keep [tc] with n_keep non-zero bytes -> keep01 [tc] 0 / 1, rank [tc] the new
// index of a kept cell (~0u: dropped), origin [n_keep] = old_origin (device, null: identity) at the kept cells
cellector_status restage_cell_ranks(cellector_ctx *c, const uint8_t *host_keep, uint64_t tc, uint64_t n_keep, const uint32_t *old_origin,
                                    DevBuf<uint8_t> *keep01, DevBuf<uint32_t> *rank, DevBuf<uint32_t> *origin);
// ... the entries of the kept cells into a new COO, order kept, cells renumbered, counts thinned (T = 0: copied)
cellector_status restage_select(cellector_ctx *c, const CooView &in, uint64_t tc, const uint8_t *keep01, const uint32_t *rank, uint64_t T,
                                uint64_t seed, StagedCoo *out);
// ... all cells: the two counts thinned where they are
cellector_status restage_thin(cellector_ctx *c, StagedCoo *coo, uint64_t T, uint64_t seed);
// cellector_combine (kernels_combine.hip).  The selected src entries renumbered where they are: locus through d_map [n_map]
// (device; null: identity), cell + cell_add
cellector_status combine_map(cellector_ctx *c, StagedCoo *coo, const uint32_t *d_map, uint64_t n_map, uint32_t cell_add);
// ... is the key locus << 32 | cell strictly ascending over the entries of a, of b?  (one launch, one round trip)
cellector_status combine_ascending(cellector_ctx *c, const CooView &a, const CooView &b, bool *a_ascending, bool *b_ascending);
// ... the entries sorted by (locus, cell, ref, alt) into a new COO
cellector_status combine_sort(cellector_ctx *c, const CooView &v, StagedCoo *out);
// ... two sides, each ascending by (locus, cell), merged by that key into a new COO (side a first among equals)
cellector_status combine_merge(cellector_ctx *c, const CooView &a, const CooView &b, StagedCoo *out);
// ... origin / source [n_ctx + n_kept]: the ctx's own (null: identity / 0), then src_origin [n_kept] / k
cellector_status combine_cells(cellector_ctx *c, uint64_t n_ctx, uint64_t n_kept, const uint32_t *old_origin, const uint32_t *src_origin,
                               const uint8_t *old_source, uint8_t k, DevBuf<uint32_t> *origin, DevBuf<uint8_t> *source);
// ... a restage's source [n_keep]: old_source [tc] at the kept cells (rank as restage_cell_ranks made it)
cellector_status combine_source_select(cellector_ctx *c, uint64_t tc, uint64_t n_keep, const uint32_t *rank, const uint8_t *old_source,
                                       DevBuf<uint8_t> *source);
// the joined ingests (kernels_join.hip).  One stream's tokens on the device: (locus, cell, count) per entry, stream order
struct JoinTokens {
    DevBuf<uint32_t> locus, cell, count;
    uint64_t n = 0;
};
struct JoinPhases { double tokens_first = 0, tokens_second = 0, checks = 0, sorts = 0, join = 0 /*wall s*/, join_kernels_ms = -1 /*events*/; };
// ... two streams (indices index_base-based: 1 text, 0 COO) checked against the ctx's dims, put in key order and joined into `out`
// (CELLECTOR_JOIN_REF / _DEPTH); the tokens are released on the way.  A refusal leaves its words in c->err, nothing in the ctx
cellector_status join_stage(cellector_ctx *c, JoinTokens *first, JoinTokens *second, uint32_t index_base, int mode, StagedCoo *out,
                            cellector_join_summary *sum /*may be null*/, JoinPhases *ph);
// cellector_add_doublets (kernels_doublets.hip).  The doublet side: for every value 2 j + s of host_fan_val [n_fan] in the range
// host_fan_ptr [tc + 1] gives cell c, every staged entry of c summed into (locus, tc + j), thinned per (entry, pair, side);
// strictly ascending by (locus, cell).  *overflow: a sum exceeds CELLECTOR_MAX_COUNT; the first one in output order is named
cellector_status doublets_build(cellector_ctx *c, const CooView &in, uint64_t tc, uint64_t total_loci, const uint64_t *host_fan_ptr,
                                const uint64_t *host_fan_val, uint64_t n_fan, uint64_t T, uint64_t seed, StagedCoo *out,
                                bool *overflow, uint64_t *over_pair, uint32_t *over_locus, int *over_allele);
// ... origin [n_pairs] of the new cells: old_origin (device, null: identity) at host_cell_a
cellector_status doublets_origin(cellector_ctx *c, const uint32_t *host_cell_a, uint64_t n_pairs, uint64_t tc, const uint32_t *old_origin,
                                 DevBuf<uint32_t> *origin);
// cellector_write_mtx / cellector_format_mtx (kernels_mtx_write.hip) behind their checks: the staged entries as mtx text, window by
// window (option write_window); only reads the ctx
uint64_t mtx_write_window(const cellector_ctx *c);
cellector_status mtx_write_pair(cellector_ctx *c, const char *first_path, const char *second_path, int mode, uint32_t flags,
                                cellector_write_summary *sum, cellector_write_bgzf_summary *gz = nullptr /*non-null: BGZF files*/);
cellector_status mtx_format_range(cellector_ctx *c, int which, int mode, uint8_t sep, uint64_t first, uint64_t n, uint8_t *out,
                                  uint64_t capacity, uint64_t *n_bytes, uint64_t *n_lines);
// BGZF compression on the device (kernels_bgzf.hip; the format: bgzf_format.h).  bz_compress turns device text into members, one
// launch per call; cellector_write_mtx_bgzf feeds it the writer's windows, cellector_bgzf_compress host bytes.
struct BzScratch {
    DevBuf<uint8_t> tables;               // BgzfTables
    DevBuf<uint8_t> slots;                // [cap_blocks] members, one fixed slot each, before the compaction
    DevBuf<uint64_t> sizes;               // [cap_blocks + 1] member sizes, then their offsets
    DevBuf<unsigned long long> stored;    // [1] stored blocks of a launch
    uint64_t cap_blocks = 0;
    // CELLECTOR_TIMING=1: the two kernels' GPU time between events, summed over the calls (the compaction is then awaited)
    bool timed = false;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    double ms_block = 0, ms_compact = 0;
    BzScratch() = default;
    BzScratch(const BzScratch &) = delete;
    BzScratch &operator=(const BzScratch &) = delete;
    ~BzScratch();
};
uint64_t bz_blocks(uint64_t text_bytes);    // blocks of that many bytes of text
uint64_t bz_out_capacity(uint64_t blocks);  // bytes a device buffer needs to take the members of that many blocks
cellector_status bz_scratch(cellector_ctx *c, BzScratch *s, uint64_t cap_blocks);
cellector_status bz_compress(cellector_ctx *c, BzScratch *s, const uint8_t *text, uint64_t n, uint8_t *out, uint64_t *bytes,
                             uint64_t *blocks, uint64_t *stored);
cellector_status bgzf_compress_host(cellector_ctx *c, const uint8_t *in, uint64_t n, uint8_t *out, uint64_t capacity, uint64_t *n_out,
                                    uint64_t *n_blocks);
// BGZF inflation on the device (kernels_inflate.hip; the format: inflate_format.h).  inf_launch queues one launch over a run of
// members; cellector_bgzf_decompress feeds it host bytes, the mtx ingest (option gz_device) the windows of a file.
struct InfMember {       // one member for k_bgzf_inflate: its deflate body in the launch's input, its text in the launch's output
    uint64_t in_off;
    uint64_t out_off;
    uint32_t in_len, isize, crc, pad;
};
struct BgzfBlock;
struct InfScratch {
    DevBuf<uint8_t> tables;            // InfCrcTables
    DevBuf<InfMember> members;         // [cap_members]
    DevBuf<unsigned long long> status;       // [1] the status word
    unsigned long long *h_status = nullptr;  // pinned: where the status word arrives behind every launch
    uint64_t cap_members = 0;
    uint64_t n_members = 0, bytes_in = 0, bytes_out = 0;  // summed over the launches
    // CELLECTOR_TIMING=1: the kernel's GPU time between events, summed by inf_launch_timed
    bool timed = false;
    hipEvent_t ev[2] = {nullptr, nullptr};
    double ms_kernel = 0;
    InfScratch() = default;
    InfScratch(const InfScratch &) = delete;
    InfScratch &operator=(const InfScratch &) = delete;
    ~InfScratch();
};
uint64_t inf_chunk_members();  // members per launch (CELLECTOR_INFLATE_CHUNK: fewer, for tests)
cellector_status inf_scratch(cellector_ctx *c, InfScratch *s, uint64_t cap_members);
cellector_status inf_launch(cellector_ctx *c, InfScratch *s, hipStream_t st, const std::vector<BgzfBlock> &blocks, uint64_t k0, uint64_t k1,
                            InfMember *host, const uint8_t *file, const uint8_t *dev_in, uint64_t in_first, uint64_t n_in, uint8_t *dev_out,
                            uint64_t out_first, uint64_t out_cap, bool reset);
void inf_launch_timed(InfScratch *s);
cellector_status inf_refused(const cellector_ctx *c, const char *what, unsigned long long status);
cellector_status bgzf_decompress_host(cellector_ctx *c, const uint8_t *in, uint64_t n, uint8_t *out, uint64_t capacity, uint64_t *n_out,
                                      uint64_t *n_blocks);
cellector_status synth_generate(cellector_ctx *c, double density, uint64_t seed, double minority_fraction,
                                double doublet_fraction);
cellector_status synth_write_mtx(cellector_ctx *c, const char *alt_path, const char *ref_path);
// device helpers
cellector_status dev_exclusive_scan_u64(cellector_ctx *c, uint64_t *data, uint64_t n, uint64_t *total_out_host);
cellector_status dev_sort_pairs_u32_u64(cellector_ctx *c, uint32_t *keys_in, uint32_t *keys_out,
                                        uint64_t *vals_in, uint64_t *vals_out, uint64_t n, int end_bit);
// engine v2 (kernels_tiled_build.hip, once per ingest; then kernels_tiled.hip)
cellector_status tiled_build(cellector_ctx *c);
// masked_cnt: [nloc] entries of every cell at the pass' masked loci; null = the ctx's own (the loop's mask)
cellector_status tiled_cell_pass(cellector_ctx *c, const double2 *ab, double *norm_out, bool for_em, const uint32_t *masked_cnt = nullptr);
cellector_status tiled_locus_pass(cellector_ctx *c);
cellector_status tiled_masked_update(cellector_ctx *c);
// masked_cnt from scratch under c->mask (cellector_set_loci_mask); ones: [L] device scratch, allocated before the mask was written
cellector_status tiled_masked_recount(cellector_ctx *c, uint8_t *ones);
// ... under the mask of one call, into the caller's scratch cnt [nloc] (host_mask [L] or null = all used); the ctx's own stay
cellector_status tiled_call_masked_count(cellector_ctx *c, const uint8_t *host_mask, uint32_t *cnt);
cellector_status tiled_prebuild_tables(cellector_ctx *c);
// the store of option t2_cache for the ELLPACK copy the ctx holds, empty (kernels_tiled_build.hip; no-op where k_t2_cell does not run)
cellector_status t2_cache_alloc(cellector_ctx *c);
// option t2_cache resolved for the shard the ctx holds.  Automatic: on a big shard, whose lookups miss the L2 (a 77 MB table at
// 200k loci) and whose tile kernel streams through their traffic; a small shard's lookups hit it and gain nothing
inline bool t2_cache_on(const cellector_ctx *c) { return c->t2_cache > 0 || (c->t2_cache < 0 && c->nloc >= (1ull << 19)); }
cellector_status tiled_posteriors(cellector_ctx *c, double mf0, double lp_min, double lp_maj, double lp_dbl, double *sdbl);
// device-side mtx text parse (kernels_parse.hip); the pair's bytes and header: mtx_bytes.h
struct MtxInput;
cellector_status ctx_mtx_open(const cellector_ctx *c, const char *alt_path, const char *ref_path, MtxInput **out,
                              uint64_t *total_loci, uint64_t *total_cells, bool single_device = false /*option gz_device applies*/);  // mtx_input_open, its failure into c->err
void mtx_input_close(MtxInput *in);
// split ingest of a multi-device ctx (kernels_parse.hip): every shard tokenises a range of windows of both files
struct MtxSplit;
MtxSplit *mtx_split_new(int n_shards, LocalGroup *thread_barrier, bool balance /*cut the cells by entries, not by count*/);
void mtx_split_delete(MtxSplit *s);
bool mtx_input_windowed(const MtxInput *in, int64_t parse_window_opt);
cellector_status ingest_stage_mtx_split(cellector_ctx *c, MtxInput *in, MtxSplit *s, int rank, uint64_t parse_window, StagedCoo *out);
cellector_status ingest_stage_mtx_device(cellector_ctx *c, MtxInput *in, cellector_ctx *helper = nullptr /*parses the ref file*/);
// the joined text ingest: FIRST's size line against SECOND's (whose dims the MtxInput carries), then all three tokens of every line
// of both files, each file windowed exactly when the aligned ingest would window it
cellector_status join_size_lines(const cellector_ctx *c, const MtxInput *in, uint64_t *first_hint);
cellector_status join_parse_pair(cellector_ctx *c, MtxInput *in, uint64_t first_hint, JoinTokens *first, JoinTokens *second, JoinPhases *ph);
