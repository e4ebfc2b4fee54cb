// Engine v2: table-driven passes over a tiled 16-bit matrix layout (gfx950, wave64).  This file: what an iteration runs;
// kernels_tiled_build.hip: tiled_build, which makes the layout once per ingest; tiled.h: what the two share.
//
// Observation: under one (alpha_l, beta_l) the log-pmf of an entry depends only on (alt, ref), and vartrix counts
// are tiny (n = alt+ref <= 4 for ~99 % of entries).  So per EM iteration and locus we tabulate the 14 log-pmfs of
// n = 1..4 and the 4 expected terms (18 doubles per locus) and the matrix passes become pure table lookups:
//
//   cell pass   (get_cell_log_likelihoods, main.rs:541-591): the matrix is cut into (1024-cell block x 639-locus
//               chunk) tiles, stored in a sliced-ELLPACK form with a sorting window of one tile (SELL-64-1024): the
//               cells of a tile are ordered by their entry count, every 64 of them form a slice whose rows (one per
//               cell) are padded to the slice's longest cell, K entries of either parity (the cell ids ride in the rows when K
//               is odd and in a block of their own when K is even: tiled.h), so that all lanes of a wave run the
//               SAME number of lookups — no divergence and ~9 % padding instead of the ~55 % idle lanes of a
//               cell-per-lane walk in file order — and a lane fetches its row with one or two 16-byte loads.
//               A u16 entry carries where its two table values sit: the expected term's element << 4 | how many planes behind it
//               the log-pmf lies (tiled.h, offset entries); padding points at an all-zero slot.
//               A persistent 1024-thread workgroup takes columns of four cell blocks and a group of chunks: the chunk's
//               table lives in LDS code-major (18 planes of 640 slots: the log-pmf and the expected term of an entry are two
//               8-byte reads on the SAME bank pair, slot mod 32, whatever the code; tiled.h); a lane keeps its cell's entries of the tile in registers (prefetched two
//               tiles ahead) and adds the tile's sum to the cell's accumulator in LDS (the lane <-> cell assignment
//               changes from tile to tile).  No transcendental, no atomics; a cell's sum runs over its chunks in order
//               and inside a chunk in ascending-locus order: bit-deterministic (the number of chunk groups fixes how
//               the partials associate).
//   locus pass  (get_locus_log_likelihoods, main.rs:368-420): all outputs follow from the minority cells' entry counts per
//               (locus, code): contributions are count x table value; the majority side is (static histogram - minority).
//               The counts come either from walking only the excluded cells' CSR rows into LDS range histograms
//               (k_minority_ranges: the usual case, a few percent of the matrix) or from streaming a compact CSC of
//               24/32-bit entries (cell | code) past the exclusion bitmask in LDS (k_locus_stats2); chosen on the device.
//   overflow    entries with n == 0 or n > 4 (~1 %) live in a small CSR/CSC in the v1 packed format; the cell side
//               evaluates them itself, the locus side from per-locus cumulative-log tables (see below).
#include <hip/hip_ext.h>

#include "tiled.h"

// code = n(n+1)/2 - 1 + ref:  n=1: (1,0)(0,1)  n=2: (2,0)(1,1)(0,2)  n=3: (3,0)..(0,3)  n=4: (4,0)..(0,4)
__device__ __constant__ uint8_t T_A_OF[T_NCODE] = {1, 0, 2, 1, 0, 3, 2, 1, 0, 4, 3, 2, 1, 0};
__device__ __constant__ uint8_t T_R_OF[T_NCODE] = {0, 1, 0, 1, 2, 0, 1, 2, 3, 0, 1, 2, 3, 4};

// ---------------------------------------------------------------------------------------------------------
// tables, laid out [chunk][the chunk's image] so that a chunk is one contiguous block the tile kernel copies straight into
// LDS.  The image is the geometry's (tiled.h, tab_pmf / tab_exp): code-major for the regular entries, i.e. 18 planes of T_BL
// doubles, the 4 expected terms' (PAIRS; else zero) before the 14 log-pmfs'.  All zero for masked loci (alpha < 0), for the
// padding beyond L and in the last slot of every chunk (the padding entries' target).
// ---------------------------------------------------------------------------------------------------------
// In an EM iteration the kernel is the iteration's FIRST one: it then also forms alpha/beta (init_alpha_betas,
// main.rs:598-611: alpha_l = (S_alt_l + 1) - sum over excluded cells, the subtrahend being the all-reduced ALT_MIN plane of
// the previous iteration; masked loci get alpha = -1), stores them for the other kernels and resets the iteration's counters.
struct ab_src_t {
    const double *s_alt, *s_ref, *alt_min, *ref_min;  // null s_alt: alpha/beta are read from `ab`
    const uint8_t *mask;
    double2 *ab_out;
    double *xl_counters;
    uint32_t *d_counters, *tile_work;
    uint32_t n_work;
};
// Six waves per 64 loci, each with its share of a locus' 18 values (about equal arithmetic): one thread per locus left
// three waves per SIMD, too few to hide the dependent divisions and logs (75 us at 200k loci).
template <bool PAIRS>
__global__ __launch_bounds__(64 * TB_PARTS) void k_build_tables(uint64_t L, uint32_t nj, const double2 *__restrict__ ab,
                                                                const double *__restrict__ lf, double *__restrict__ tab,
                                                                ab_src_t src)
{
    if (src.s_alt && blockIdx.x == 0) {
        if (threadIdx.x < LC_COUNTERS) src.xl_counters[threadIdx.x] = 0.0;
        if (threadIdx.x < 8) src.d_counters[threadIdx.x] = 0u;
        for (uint32_t i = threadIdx.x; i < src.n_work; i += blockDim.x) src.tile_work[i] = 0u;
    }
    const int part = threadIdx.x >> 6;  // wave-uniform
    const uint64_t t = (uint64_t)blockIdx.x * 64 + (threadIdx.x & 63);  // (chunk, slot)
    if (t >= (uint64_t)nj * T_BL) return;
    const uint64_t chunk = t / T_BL, slot = t % T_BL;
    const uint64_t l = chunk * T_BLU + slot;
    double2 p = make_double2(-1.0, -1.0);
    if (slot < T_BLU && l < L) {
        if (src.s_alt) {
            p.x = (src.s_alt[l] + 1.0) - src.alt_min[l];
            p.y = (src.s_ref[l] + 1.0) - src.ref_min[l];
            if (!src.mask[l]) p.x = p.y = -1.0;
            if (part == 0) src.ab_out[l] = p;
        } else {
            p = ab[l];
        }
    }
    const bool live = p.x >= 0.0;
    double *img = tab + chunk * TAB_ELEMS;  // (code-major: a wave's 64 slots of a plane are one contiguous store)
    // code w <-> (alt, ref) as in T_A_OF / T_R_OF, written out so that the products unroll
#define TB_PMF(W, A, R) img[tab_pmf<geo_reg>((uint32_t)slot, W)] = live ? dm_log_bb_pmf(lf, p.x, p.y, A, R) : 0.0
#define TB_EXP(N) img[tab_exp<geo_reg>((uint32_t)slot, N - 1)] = (PAIRS && live) ? dm_expected_log_pmf(lf, p.x, p.y, N) : 0.0
    switch (part) {
    case 0: TB_EXP(4u); TB_PMF(0, 1u, 0u); break;
    case 1: TB_EXP(3u); TB_PMF(1, 0u, 1u); break;
    case 2: TB_EXP(2u); TB_PMF(2, 2u, 0u); TB_PMF(3, 1u, 1u); break;
    case 3: TB_EXP(1u); TB_PMF(4, 0u, 2u); TB_PMF(5, 3u, 0u); break;
    case 4: TB_PMF(6, 2u, 1u); TB_PMF(7, 1u, 2u); TB_PMF(8, 0u, 3u); TB_PMF(9, 4u, 0u); break;
    default: TB_PMF(10, 3u, 1u); TB_PMF(11, 2u, 2u); TB_PMF(12, 1u, 3u); TB_PMF(13, 0u, 4u); break;
    }
#undef TB_PMF
#undef TB_EXP
}

// ---------------------------------------------------------------------------------------------------------
// cell pass over the tiles
// ---------------------------------------------------------------------------------------------------------
#ifndef TILE_ABL
#define TILE_ABL 0  // ablation builds of the tile kernel (tools/gpu_ab.sh; wrong values, timings only): 1 no lookups, 2 rows loaded once, 3 no table
                    // re-staging, 4 conflict-free lookups, 5 = 1 + 3, 6 conflict-free accumulator updates, 7 no barriers and no re-staging, 8 no
                    // accumulator access, 9 rows and slice headers loaded once, 10 header loads of the column's first chunk only (cache hits)
#endif
// Workgroup barrier that waits for this wave's LDS traffic only.  __syncthreads() also drains vmcnt, i.e. it would wait
// for the prefetch loads in flight and make them synchronous.
#ifndef TILE_PFD
// Prefetch distance of the tile rows in steps (a column of four blocks; two blocks: always 2) = number of row buffers.
// 4 (a whole chunk ahead), round 2 at cfg4: the kernel itself 1.955 -> 1.87 ms, but at 123 VGPRs (97 with two buffers) its four
// waves per SIMD take the whole register file, the overflow kernels of the side stream find no room beside it and run behind it
// instead: cell pass 2.02 -> 2.26 ms.  3: three buffers rotating over the four steps of a chunk, the chunk loop written out three
// times (the buffer of a step must be known at compile time).
#define TILE_PFD 2
#endif
#ifndef TILE_PFD_T2
#define TILE_PFD_T2 2  // ... of the tier-2 tiles (deep coverage): short rows, little work per step
#endif
#ifndef TILE_PINNED
#define TILE_PINNED 1
#endif
#if TILE_ABL == 7  /* ablation: no chunk barriers (and the table staged once) */
#define TILE_BARRIER() do { } while (0)
#else
#define TILE_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
#endif

struct __attribute__((packed, aligned(4))) tile_u4 { uint32_t x, y, z, w; };  // 16-byte load at a 4-byte aligned address

template <bool EXPECTED, int T_SB, class G = geo_reg>
__global__ __launch_bounds__(T_THREADS, 4) void k_tile_ll(uint32_t nb, uint32_t nj, uint32_t cpg, uint32_t groups,
                                                          uint32_t n_cols, uint32_t *__restrict__ work /*[groups], zeroed*/,
                                                          const uint16_t *__restrict__ thdr,
                                                          const uint16_t *__restrict__ tiles,
                                                          const double *__restrict__ tab, uint64_t npad,
                                                          double *__restrict__ part_ll, double *__restrict__ part_ell)
{
    // PERSISTENT workgroups, one per CU (the LDS footprint allows no second one): a workgroup belongs to one group of locus
    // chunks and keeps fetching columns of T_SB consecutive 1024-cell blocks from the group's
    // counter until none is left.  A grid of short-lived workgroups instead leaves a CU idle whenever the next one cannot
    // start because waves of the small overflow kernels running beside this one still hold registers there (measured:
    // 2.2 ms alone, 2.7 ms next to them).
    // Per chunk the table is staged ONCE in LDS and the T_SB tiles are walked one after the other; wave w takes slice w of
    // each tile.  Everything a step needs was requested two steps earlier: in every step the values loaded before are
    // consumed FIRST, then the next loads are issued as straight-line, unconditional instructions (indices are clamped
    // instead of guarded).
    using tab_t = typename std::conditional<EXPECTED, double2, double>::type;  // (log-pmf, expected) sums of a cell
    constexpr uint32_t TAB_U = G::LROW * G::BL * sizeof(double) / 16;  // 16-byte units per chunk table
    constexpr int NP = (TAB_U + T_THREADS - 1) / T_THREADS;          // units per thread (the last one partial)
    static_assert(NP == 6, "table prefetch registers are written out by hand");
    __shared__ __attribute__((aligned(16))) double s_tab[G::LROW * G::BL];
    static_assert(G::LROW * G::BL % 2 == 0, "whole 16-byte units");
    __shared__ tab_t s_acc[T_SB * T_BC];  // per-cell sums of the workgroup's blocks
    __shared__ uint32_t s_col;
    const uint32_t tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    // group = linear block id mod groups (the workgroups of a group walk its chunks in step: each XCD's L2 fetches a table
    // chunk once, whatever the number of groups)
    const uint32_t g = blockIdx.x % groups;
    const uint32_t j0 = g * cpg, j1 = min(nj, j0 + cpg);
    if (j0 >= j1) return;
  for (;;) {
    if (tid == 0) s_col = atomicAdd(&work[g], 1u);
    __syncthreads();  // (also: the previous column's partial sums have been read out of s_acc)
    const uint32_t col = s_col;
    if (col >= n_cols) break;
    const uint32_t b0 = col * T_SB;
#pragma unroll
    for (int s = 0; s < T_SB; s++) {
        if constexpr (EXPECTED) s_acc[s * T_BC + tid] = make_double2(0.0, 0.0);
        else s_acc[s * T_BC + tid] = 0.0;
    }

    // explicit registers (an indexed local array ends up in scratch memory)
    double2 p_t0, p_t1, p_t2, p_t3, p_t4, p_t5;
#define TABLE_PREFETCH(J)                                                                                        \
    do {                                                                                                         \
        const double2 *src__ = reinterpret_cast<const double2 *>(tab) + (uint64_t)(J) * TAB_U + tid;             \
        p_t0 = src__[0];                                                                                         \
        p_t1 = src__[T_THREADS];                                                                                 \
        p_t2 = src__[2 * T_THREADS];                                                                             \
        p_t3 = src__[3 * T_THREADS];                                                                             \
        p_t4 = src__[4 * T_THREADS];                                                                             \
        p_t5 = src__[5 * T_THREADS]; /* partial: reads into the next chunk / the tail pad */                     \
    } while (0)

    // Software pipeline over the steps t = (chunk, block) of this workgroup: the rows of step t+2 are requested in step
    // t; the slice header they need (wave-uniform: scalar loads) is requested in step t-1.  Two buffers serve the even
    // and the odd steps; a buffer is consumed and then refilled in place.
    // lo, hi: the row's first 16 u16 (K odd: cell id + entries 0..14; K even: entries 0..15); cell: the cell id, from the row's
    // first u16 (odd) or the slice's block of cell ids (even); base = first u16 of the slice in `tiles` (wave-uniform, like k: both
    // stay in scalar registers — the row's own address is only needed again by the rare slice with rows beyond T_ROW_U16)
    struct row_t { tile_u4 lo, hi; uint32_t cell, k; uint64_t base; };
    // slice header of a step (beyond the last chunk: the last chunk's; a workgroup at the ragged end re-reads the last block)
    const uint32_t wv_s = (uint32_t)__builtin_amdgcn_readfirstlane((int)wv);
#define HDR_LOAD(H, J, S) /* S: a compile-time block number; J: the chunk (clamped by the caller) */           \
    do {                                                                                                         \
        /* The slices of a tile are sorted by length: wave w takes slice w, 15-w, w+8, 7-w (mod 16) of the      */ \
        /* chunk's tiles, so that all waves carry about the same load between two chunk barriers.  (Everything  */ \
        /* but the chunk is invariant in the chunk loop: a step forms the address with an add and a shift.)     */ \
        const uint32_t rot__ = (wv_s + 8u * ((uint32_t)(S) >> 1)) & 15u, sl__ = ((S) & 1u) ? 15u - rot__ : rot__; \
        if (TILE_ABL != 9 || first_rows) /* ablation 9: headers loaded in the prologue only; 10: always the column's first chunk's */ \
        (H) = reinterpret_cast<const uint4 *>(thdr + ((uint64_t)min(b0 + (uint32_t)(S), nb - 1) * nj + (TILE_ABL == 10 ? j0 : (J))) * T_HDR)[sl__]; \
    } while (0)
    // this lane's row of the slice with header H (the format follows from K's parity: tiled.h).  A row of at most 8 u16 is covered
    // by the first load: the second one then repeats it (never consumed) instead of reading far beyond the row.  The cell id: regular
    // kernels, a 2-byte load of its own in both formats (CELL_LOAD below); tier-2 kernels, the row's first u16 when K is odd and
    // a 2-byte load out of the slice's block of cell ids, requested here with the row, when K is even.
#define ROW_LOAD(E, H)                                                                                           \
    do {                                                                                                         \
        (E).k = (SKIP_EMPTY && (H).w) ? 0u : (H).z; /* 0: a slice without entries (tier-2 tiles): the step skips it */ \
        (E).base = ((uint64_t)(H).y << 32) | (H).x;                                                              \
        /* (a wave-uniform 64-bit base in scalar registers plus a 32-bit byte offset per lane: the loads take the  */ \
        /*  scalar-base form, and the address costs one multiply instead of 64-bit vector arithmetic)               */ \
        const char *sb__ = reinterpret_cast<const char *>(tiles + (E).base);                                     \
        const uint32_t odd__ = (H).z & 1u, n16__ = (H).z + odd__; /* u16 per row */                                \
        const uint32_t off__ = __umul24(lane, n16__ * 2u) + (odd__ ? 0u : 128u); /* (full-rate 24-bit multiply) */ \
        if ((!(TILE_ABL == 2 || TILE_ABL == 9) || first_rows) && !(SKIP_EMPTY && (H).w)) { /* ablations 2, 9: rows loaded in the prologue only */ \
            if constexpr (SKIP_EMPTY) { /* (short steps: an even K's cell id flies with the row, see CELL_LOAD) */ \
                if (!odd__) (E).cell = *reinterpret_cast<const uint16_t *>(sb__ + lane * 2u);                    \
            }                                                                                                    \
            (E).lo = *reinterpret_cast<const tile_u4 *>(sb__ + off__);                                           \
            (E).hi = *reinterpret_cast<const tile_u4 *>(sb__ + (n16__ > 8u ? 16u : 0u) + off__);                 \
        }                                                                                                        \
    } while (0)

    // this lane's cell id of the slice whose rows E was just asked for, regular geometry: the row's first u16 (K odd) or u16 `lane`
    // of the slice's block of cell ids (K even).  Requested at the END of a step, behind the last use of the buffer's previous cell
    // id, so that the register is refilled in place: requested with the rows it is a third live cell id per lane (the step's own and
    // one per row buffer), and the EM pass' kernel leaves its register granule (107 VGPRs for the parent's 102; 103 this way,
    // measured no slower).  It still has PFD - 1 whole steps to arrive, and vmcnt counts it in issue order behind the rows it belongs
    // to.  An odd K has the id in the row's first dword as well, and loading it again is work the sums do not need — but taking it from
    // there (the load for even K only, cell = K odd ? w[0] & 0xffff : loaded) keeps a copy alive beside the buffers: 105 / 91 VGPRs,
    // out of the granule again; the load is a hit in the line the row came from.
    // The tier-2 kernels (short steps, mostly K = 1, registers to spare: 107 of 112) do exactly that: ROW_LOAD, TILE_STEP.
#define CELL_LOAD(E)                                                                                             \
    do {                                                                                                         \
        const uint32_t k__ = (E).k, odd__ = k__ & 1u;                                                            \
        if constexpr (!SKIP_EMPTY)                                                                               \
        (E).cell = *reinterpret_cast<const uint16_t *>(reinterpret_cast<const char *>(tiles + (E).base) +        \
                                                       __umul24(lane, odd__ ? (k__ + 1u) * 2u : 2u));            \
    } while (0)
    // PFD = prefetch distance in steps = number of pipeline buffers.  With four blocks per column every block of the chunk has
    // a buffer of its own and the rows are requested a whole chunk ahead.
    // The tier-2 tiles of a deep matrix hold 0.4 entries per row: ten of a tile's sixteen slices (sorted by length) have none, and a
    // wave whose slice is marked so in its header skips the step — no row loads, no lookups, no accumulator update: that kernel alone
    // 1.90 -> 1.46 ms at 10^6 cells x 200k loci deep.  (It costs 6 VGPRs — 106: the per-entry kernels of the side stream, 88, then
    // find no room beside it and wait for it; the iteration still gains, 5.4 -> 5.0 ms.  Sharing ONE all-padding slice between the
    // empty slices instead, with the kernel unchanged, would update the same accumulators from several waves: not an option.)
    constexpr bool SKIP_EMPTY = G::NLO != 1;
    constexpr uint32_t PFD = T_SB == 4 ? (uint32_t)(G::NLO == 1 ? TILE_PFD : TILE_PFD_T2) : 2u;
    static_assert(PFD >= 2 && PFD <= 4, "row buffers");
    uint4 h0, h1, h2, h3;   // at the top of step t (t % PFD == 0): slice headers of steps t+PFD (h0), t+PFD+1 (h1), ...
    row_t e0, e1, e2, e3;   // at the top of step t (t % PFD == 0): rows of steps t (e0), t+1 (e1), ...
    // The table loads are the OLDEST requests when the chunk loop is entered, like on its back edge, so that the wait
    // for them is a counted vmcnt that leaves the younger row requests in flight (the scheduler must not move them
    // behind the loads below: vmcnt counts in issue order).
    bool first_rows = true;  // (ablations 2, 9)
    TABLE_PREFETCH(j0);
    __builtin_amdgcn_sched_barrier(0);
#define HDR_STEP(H, T) HDR_LOAD(H, min(j0 + (uint32_t)(T) / T_SB, j1 - 1), (uint32_t)(T) % T_SB)  /* header of step T of the column */
    HDR_STEP(h0, 0);
    HDR_STEP(h1, 1);
    if constexpr (PFD >= 3) HDR_STEP(h2, 2);
    if constexpr (PFD == 4) HDR_STEP(h3, 3);
    ROW_LOAD(e0, h0);
    ROW_LOAD(e1, h1);
    if constexpr (PFD >= 3) ROW_LOAD(e2, h2);
    if constexpr (PFD == 4) ROW_LOAD(e3, h3);
    CELL_LOAD(e0);
    CELL_LOAD(e1);
    if constexpr (PFD >= 3) CELL_LOAD(e2);
    if constexpr (PFD == 4) CELL_LOAD(e3);
    HDR_STEP(h0, PFD);
    HDR_STEP(h1, PFD + 1);
    if constexpr (PFD >= 3) HDR_STEP(h2, PFD + 2);
    if constexpr (PFD == 4) HDR_STEP(h3, PFD + 3);
#undef HDR_STEP
    first_rows = false;

    // one step: block S of the current chunk, pipeline buffers E / H
    // lookup number KK of the ladder = u16 number KK + 1 of the row = half (KK + 1) & 1 of dword (KK + 1) >> 1.  In both row
    // formats dword p >= 1 holds two consecutive entries and D = (K + 1) >> 1 dwords hold entries (K is wave-uniform), so the
    // lookups come in pairs behind one scalar branch on D; only dword 0 differs: its high half is an entry in both formats, its
    // low half is one when K is even (that lookup starts the row's sums).
#if TILE_ABL == 1 || TILE_ABL == 5  /* ablation: no table lookups */
#define TILE_LOOKUP(V, E16) do { if constexpr (EXPECTED) V = make_double2((double)(E16), 1.0); else V = (double)(E16); } while (0)
#elif TILE_ABL == 4  /* ablation: lookups free of bank conflicts (a lane keeps to its own bank pair; wrong values) */
#define TILE_LOOKUP(V, E16)                                                                                      \
    do {                                                                                                         \
        if constexpr (G::OFFSET_ENTRIES) { /* the entry's own two elements, moved inside their planes onto the lane's bank pair */ \
            static_assert(G::BL % 32u == 0, "a plane keeps the bank pair");                                      \
            const uint32_t own__ = (tile_entry_exp<G>(E16) & ~31u) | (lane & 31u);                               \
            if constexpr (EXPECTED) V = make_double2(s_tab[own__ + tile_entry_pmf<G>(E16) - tile_entry_exp<G>(E16)], s_tab[own__]); \
            else V = s_tab[own__ + tile_entry_pmf<G>(E16) - tile_entry_exp<G>(E16)];                             \
        } else {                                                                                                 \
        const uint32_t b__ = (((E16) >> 4) & 127u) * 32u + (lane & 31u), c__ = (((E16) >> 5) & 127u) * 32u + (lane & 31u); \
        if constexpr (EXPECTED) V = make_double2(s_tab[b__], s_tab[c__ + 4096u]);                                \
        else V = s_tab[b__];                                                                                     \
        }                                                                                                        \
    } while (0)
#else
// the entry's log-pmf and, in the EM pass, its expected term: where they sit is the entry's business (tiled.h).  Offset entries:
// the expected term's byte address is a shift and a mask of the row's dword, the log-pmf's one field extract and one multiply-add
// on top of it (plane difference x plane bytes); slot << 4 | code: two instructions for slot x 8, then two for each value.
#define TILE_LOOKUP(V, E16)                                                                                      \
    do {                                                                                                         \
        if constexpr (G::OFFSET_ENTRIES) {                                                                       \
            if constexpr (EXPECTED) V = make_double2(s_tab[tile_entry_pmf<G>(E16)], s_tab[tile_entry_exp<G>(E16)]); \
            else V = s_tab[tile_entry_pmf<G>(E16)];                                                              \
        } else { /* (the slot taken out once, as the tier-2 instances have always been compiled) */              \
            const uint32_t s__ = tile_entry_slot<G>(E16);                                                        \
            if constexpr (EXPECTED) V = make_double2(s_tab[tab_pmf<G>(s__, tile_entry_code<G>(E16))], s_tab[tab_exp<G>(s__, tile_entry_ne<G>(E16))]); \
            else V = s_tab[tab_pmf<G>(s__, tile_entry_code<G>(E16))];                                            \
        }                                                                                                        \
    } while (0)
#endif
#define TILE_RD(V, KK)                                                                                           \
    tab_t V;                                                                                                     \
    do {                                                                                                         \
        const uint32_t idx__ = (((KK) + 1) & 1) ? (w__[((KK) + 1) >> 1] >> 16) : (w__[((KK) + 1) >> 1] & 0xffffu); \
        TILE_LOOKUP(V, idx__);                                                                                   \
    } while (0)
#define TILE_ADD(V)                                                                                              \
    do {                                                                                                         \
        if constexpr (EXPECTED) { a_ll__ += (V).x; a_el__ += (V).y; }                                            \
        else a_ll__ += (V);                                                                                      \
    } while (0)
    // one level of the written-out lookup chain: request the next pair, THEN add the pair requested one level earlier (the
    // sums still run in entry order), so that four lookups of a wave are in flight instead of two
/* (TILE_PIN: without it the compiler hoists the two adds, common to both arms, above the branch — right behind the    */
/*  previous level's requests, which they then wait for: no lookup of the next level would be in flight meanwhile.  */
/*  The empty asm makes the value a different one in this arm and, with its memory clobber, keeps the requests above */
/*  it.)                                                                                                            */
#if TILE_PINNED
#define TILE_PIN(V)                                                                                              \
    do {                                                                                                         \
        if constexpr (EXPECTED) asm volatile("" : "+v"((V).x), "+v"((V).y) : : "memory");                        \
        else asm volatile("" : "+v"(V) : : "memory");                                                            \
    } while (0)
#else
#define TILE_PIN(V) do { } while (0)
#endif
#define TILE_LEVEL(KA, KB, PA, PB, BODY)                                                                         \
    if (D__ > (((KA) + 1u) >> 1)) {                                                                              \
        TILE_RD(v##KA, KA); TILE_RD(v##KB, KB);                                                                  \
        TILE_PIN(PA); TILE_PIN(PB);                                                                              \
        TILE_ADD(PA); TILE_ADD(PB);                                                                              \
        BODY                                                                                                     \
    } else { TILE_ADD(PA); TILE_ADD(PB); }
#define TILE_STEP(S, E, H)                                                                                       \
    do {                                                                                                         \
        /* 1. consume the row requested PFD steps ago: u16 number i of the row sits in half i & 1 of dword i >> 1 */ \
        const uint32_t w__[8] = {(E).lo.x, (E).lo.y, (E).lo.z, (E).lo.w, (E).hi.x, (E).hi.y, (E).hi.z, (E).hi.w}; \
        const uint32_t K__ = (uint32_t)__builtin_amdgcn_readfirstlane((int)(E).k); /* wave-uniform */            \
        const uint32_t D__ = (K__ + 1u) >> 1; /* dwords of the row that hold entries */                          \
        const uint64_t cur_base__ = (E).base;                                                                    \
        const uint32_t cell__ = (SKIP_EMPTY && (K__ & 1u)) ? (w__[0] & 0xffffu) : (E).cell;                      \
        /* 2. issue the next requests: rows of step t+PFD (their header is here; their cell ids: at the end of the step), */ \
        /*    header of step t+2 PFD */                                                                          \
        ROW_LOAD(E, H);                                                                                          \
        HDR_LOAD(H, min(j + ((S) + 2 * PFD) / T_SB, j1 - 1), ((S) + 2 * PFD) % T_SB);                            \
        /* 3. the cell's accumulator is requested first (LDS answers in order: it has landed when the sums are done), */ \
        /*    then this lane's cell of the slice: K lookups for every lane (padding entries hit the zero row) */  \
        if (!(SKIP_EMPTY && K__ == 0u)) {                                                                        \
        tab_t acc__;                                                                                             \
        if constexpr (TILE_ABL == 8) { if constexpr (EXPECTED) acc__ = make_double2(0.0, 0.0); else acc__ = 0.0; }        \
        else acc__ = s_acc[(S) * T_BC + (TILE_ABL == 6 ? tid : cell__)];                                         \
        double a_ll__ = 0.0, a_el__ = 0.0;                                                                       \
        if (!(K__ & 1u)) { /* even K: entry 0 sits where the odd format has the cell id; the sums start from it (0.0 + x = x but for x = -0.0, which no table value is: a log-pmf or an expected term is negative or +0.0) */ \
            tab_t vz__;                                                                                          \
            TILE_LOOKUP(vz__, w__[0] & 0xffffu);                                                                 \
            if constexpr (EXPECTED) { a_ll__ = vz__.x; a_el__ = vz__.y; }                                        \
            else a_ll__ = vz__;                                                                                  \
        }                                                                                                        \
        /* (written out: a loop with an early exit gets re-rolled and then selects its register at run time) */  \
        TILE_RD(v0, 0);                                                                                          \
        if (D__ > 1u) {                                                                                          \
            TILE_RD(v1, 1); TILE_RD(v2, 2);                                                                      \
            TILE_PIN(v0);                                                                                        \
            TILE_ADD(v0);                                                                                        \
            TILE_LEVEL(3, 4, v1, v2,                                                                             \
            TILE_LEVEL(5, 6, v3, v4,                                                                             \
            TILE_LEVEL(7, 8, v5, v6,                                                                             \
            TILE_LEVEL(9, 10, v7, v8,                                                                            \
            TILE_LEVEL(11, 12, v9, v10,                                                                          \
            TILE_LEVEL(13, 14, v11, v12,                                                                         \
                TILE_ADD(v13); TILE_ADD(v14);                                                                    \
                const uint32_t n16__ = K__ + (K__ & 1u); /* u16 per row */                                       \
                for (uint32_t i = T_ROW_U16; i < n16__; i++) { /* rare: a slice whose rows are longer than the registers */ \
                    tab_t v__;                                                                                   \
                    uint32_t x__ = (tiles + cur_base__ + ((K__ & 1u) ? 0u : 64u) + lane * n16__)[i];             \
                    /* (a value the compiler knows to be 16 bits wide gets SDWA forms, whose constant operands — 1, 15 — */ \
                    /*  then sit in two VGPRs for the whole kernel) */                                           \
                    asm volatile("" : "+v"(x__));                                                                \
                    TILE_LOOKUP(v__, x__);                                                                       \
                    TILE_ADD(v__);                                                                               \
                } ))))))                                                                                         \
        } else TILE_ADD(v0);                                                                                     \
        /* 4. add the tile's sums to the cell's accumulator (one lane per cell and tile; tiles of the same block */ \
        /*    are separated by the chunk barriers).  A read and a write: two ds_add_f64 measured 15 % slower.      */ \
        if constexpr (EXPECTED) { acc__.x += a_ll__; acc__.y += a_el__; }                                        \
        else acc__ += a_ll__;                                                                                    \
        if (TILE_ABL != 8 || a_ll__ == 12345.678) s_acc[(S) * T_BC + (TILE_ABL == 6 ? tid : cell__)] = acc__;   \
        }                                                                                                        \
        CELL_LOAD(E);                                                                                            \
    } while (0)

    static_assert(T_SB == 2 || T_SB == 4, "even and odd steps use different pipeline buffers");
    // the table of chunk j into LDS between two barriers, the next chunk's table requested
#if TILE_ABL == 3 || TILE_ABL == 5 || TILE_ABL == 7  /* ablation: table staged for the first chunk only */
#define TILE_STAGE_IF if (j == j0)
#define TILE_NEXT_TABLE() do { } while (0)
#else
#define TILE_STAGE_IF
#define TILE_NEXT_TABLE() TABLE_PREFETCH(min(j + 1, j1 - 1))
#endif
#define TILE_STAGE()                                                                                             \
    do {                                                                                                         \
        TILE_BARRIER(); /* every wave is done with the previous chunk's table (and, first time, s_acc is zeroed) */ \
        TILE_STAGE_IF {                                                                                          \
            double2 *dst = reinterpret_cast<double2 *>(s_tab) + tid;                                             \
            dst[0] = p_t0;                                                                                       \
            dst[T_THREADS] = p_t1;                                                                               \
            dst[2 * T_THREADS] = p_t2;                                                                           \
            dst[3 * T_THREADS] = p_t3;                                                                           \
            dst[4 * T_THREADS] = p_t4;                                                                           \
            if (tid + 5 * T_THREADS < TAB_U) dst[5 * T_THREADS] = p_t5;                                          \
        }                                                                                                        \
        TILE_NEXT_TABLE();                                                                                       \
        TILE_BARRIER(); /* table visible */                                                                      \
    } while (0)
    if constexpr (T_SB == 4 && PFD == 3) {
        // three row buffers over four steps per chunk: the assignment repeats every three chunks
        for (uint32_t j = j0;;) {
            TILE_STAGE();
            TILE_STEP(0, e0, h0); TILE_STEP(1, e1, h1); TILE_STEP(2, e2, h2); TILE_STEP(3, e0, h0);
            if (++j >= j1) break;
            TILE_STAGE();
            TILE_STEP(0, e1, h1); TILE_STEP(1, e2, h2); TILE_STEP(2, e0, h0); TILE_STEP(3, e1, h1);
            if (++j >= j1) break;
            TILE_STAGE();
            TILE_STEP(0, e2, h2); TILE_STEP(1, e0, h0); TILE_STEP(2, e1, h1); TILE_STEP(3, e2, h2);
            if (++j >= j1) break;
        }
    } else {
        for (uint32_t j = j0; j < j1; j++) {
            TILE_STAGE();
            TILE_STEP(0, e0, h0);
            TILE_STEP(1, e1, h1);
            if constexpr (T_SB == 4 && PFD == 4) {
                TILE_STEP(2, e2, h2);
                TILE_STEP(3, e3, h3);
            } else if constexpr (T_SB == 4) {
                TILE_STEP(2, e0, h0);
                TILE_STEP(3, e1, h1);
            }
        }
    }
#undef TILE_STAGE
#undef TILE_STAGE_IF
#undef TILE_NEXT_TABLE
    TILE_BARRIER();
#pragma unroll
    for (int s = 0; s < T_SB; s++) {
        if (b0 + s < nb) {
            const uint64_t c = (uint64_t)g * npad + (uint64_t)(b0 + s) * T_BC + tid;
            const tab_t a = s_acc[s * T_BC + tid];
            if constexpr (EXPECTED) { part_ll[c] = a.x; part_ell[c] = a.y; }
            else part_ll[c] = a;
        }
    }
    __builtin_amdgcn_s_waitcnt(0);  // the pipeline's last (clamped, unused) loads have landed before the registers are reused
  }
#undef TILE_STEP
#undef TILE_LEVEL
#undef TILE_PIN
#undef TILE_ADD
#undef TILE_RD
#undef TILE_LOOKUP
#undef CELL_LOAD
#undef ROW_LOAD
#undef HDR_LOAD
#undef TABLE_PREFETCH
}

// ---------------------------------------------------------------------------------------------------------
// overflow entries (alt+ref == 0 or > T_K; 0.8 % at cfg4).  Two consumers, two evaluations:
//   cell side   k_ovf_cell_direct: a thread per cell row evaluates the row's overflow entries itself from (alpha, beta) of
//               their loci (a gather out of an L x 16 B table that stays in L2) and takes the expected terms from a compact
//               E table (k_ovf_tables_e).  Runs on the side stream beside the tile kernel.
//   locus side  the locus pass needs every overflow entry's log-pmf in by-locus order: k_ovf_tables builds per-locus
//               cumulative log tables, k_locus_finalize evaluates lnC + LA[alt] + LB[ref] - LAB[n] per entry as it walks
//               the locus (the lanes of a locus share its table row).  Only the EM pass needs the tables, and only at the
//               locus finalize: the table kernel follows the cell side on the side stream.
// ---------------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ T group16_sum(T v)
{
#pragma unroll
    for (int m = LF_LANES / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, LF_LANES);
    return v;
}

// rare cases kept out of line so that the common path stays small
__device__ __noinline__ double ov_slow_log_pmf(const double *lf, double alpha, double beta, uint32_t a, uint32_t r)
{
    return dm_log_bb_pmf(lf, alpha, beta, a, r);
}

// ln sum_k pmf(k)^2 (stats.rs:8-22) for 4 <= n <= OV_NE by the pmf ratio recurrence of dm_expected_log_pmf, with pmf(0) built
// from per-factor ratios (each in (0, 1]: no overflow of long products at these n)
// 1 / y to about an ulp: v_rcp_f64 (good to ~27 bits) and one Newton step; no scaling / fix-up for subnormals or
// infinities, which the arguments here (sums and products of counts) never are
__device__ __forceinline__ double ov_rcp(double y)
{
    const double r = __builtin_amdgcn_rcp(y);
    return __builtin_fma(__builtin_fma(-y, r, 1.0), r, r);
}
__device__ __forceinline__ double ov_expected_rec(double alpha, double beta, uint32_t n)
{
    // x / y as x * ov_rcp(y) instead of the ~25-instruction IEEE division: the few lanes that carry an E(n) keep their
    // whole wave waiting, and 2 n ulp-sized errors are far inside the pass' tolerance
    const double ab = alpha + beta;
    double p = 1.0;
    for (uint32_t j = 0; j < n; ++j) p *= (beta + (double)j) * ov_rcp(ab + (double)j);
    double s = p * p;
    for (uint32_t k = 0; k < n; ++k) {
        p *= ((double)(n - k) * (alpha + (double)k)) * ov_rcp((double)(k + 1) * (beta + (double)(n - k - 1)));
        s += p * p;
    }
    return log(s);
}

// Per-locus overflow table (OV_ROW doubles): [0..17] LA[i] = sum_{m<i} ln(alpha+m), [18..35] LB, [36..53] LAB,
// [64..] E(n) for n = 4..OV_NE.  Two dense kernels (a fused one left most lanes of a wave idle while a few ran the long
// loops): k_ovf_tables = one thread per (locus, family A / B / AB) running the 17 logs and their prefix sums;
// k_ovf_tables_e = one thread per (locus, n) for the totals n that occur among the locus' overflow entries (nmask: static).
__global__ __launch_bounds__(256) void k_ovf_tables(uint64_t L, const double2 *__restrict__ ab, const uint32_t *__restrict__ nmask,
                                                    double *__restrict__ otab)
{
    const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t l = idx / 3;
    if (l >= L) return;
    const int fam = (int)(idx % 3);
    const double2 p = ab[l];
    double *row = otab + l * OV_ROW + fam * OV_NT;
    if (!(p.x >= 0.0)) {
        if (fam == 0) row[0] = -1.0;  // marks a masked locus
        return;
    }
    // only as far as the largest tabulated total among the locus' overflow entries (nmask, static): the logs are the
    // kernel's whole cost, and most loci stop at a total of 6 or 7 of the 17
    const uint32_t m = nmask[l];
    const int top = m ? 4 + (31 - __clz((int)m)) : 0;
    const double x0 = fam == 0 ? p.x : (fam == 1 ? p.y : p.x + p.y);
    double acc = 0.0;
    row[0] = 0.0;
    for (int i = 0; i < OV_NT - 1 && i < top; i++) {
        acc += log(x0 + (double)i);
        row[i + 1] = acc;
    }
}
__global__ __launch_bounds__(256) void k_ovf_tables_e(uint64_t L, const double2 *__restrict__ ab,
                                                      const uint32_t *__restrict__ nmask, double *__restrict__ otab,
                                                      double *__restrict__ etab /*[L][OV_REC]: the cell side's record*/)
{
    const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t l = idx >> 4;  // 16 slots per locus: 14 totals, the last one copies alpha / beta
    if (l >= L) return;
    const uint32_t i = (uint32_t)(idx & 15u);
    if (i == 15u) {  // (a masked locus carries its negative alpha along: the cell side tests that)
        if (etab) *reinterpret_cast<double2 *>(etab + l * OV_REC) = ab[l];
        return;
    }
    if (i > (uint32_t)OV_NE - 4u || !((nmask[l] >> i) & 1u)) return;
    const double2 p = ab[l];
    if (!(p.x >= 0.0)) return;
    const double e = ov_expected_rec(p.x, p.y, 4u + i);
    otab[l * OV_ROW + OV_EOFF + i] = e;
    if (etab && i >= 1 && i <= 4) etab[l * OV_REC + 2 + (i - 1)] = e;
}

// The overflow entries' log-pmfs in by-locus order for the locus finalize, shallow-coverage form: a thread per entry
// (neighbouring threads share a locus: the three table words an entry needs come out of L1), on the side stream beside the
// tile kernel; the finalize then reads 8 bytes per entry.  (A deep-coverage matrix, ovf_deep, evaluates them inside
// k_locus_finalize instead: storing and re-reading 2.6e8 values was 4 GB of traffic per iteration at 1M x 200k.)
__global__ __launch_bounds__(256) void k_ovf_values(uint64_t n_ovf, const uint32_t *__restrict__ ovc_locus,
                                                    const uint64_t *__restrict__ ovc_ent,
                                                    const double2 *__restrict__ ab, const double *__restrict__ lf,
                                                    const double *__restrict__ otab, double *__restrict__ lp_out)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_ovf) return;
    const uint32_t l = ovc_locus[i];
    const uint64_t en = ovc_ent[i];
    const double *row = otab + (uint64_t)l * OV_ROW;
    double lp = 0.0;
    if (row[0] >= 0.0) {  // else a masked locus: no PMFData (main.rs:556)
        const uint32_t a = ENT_ALT(en), r = ENT_REF(en), n = a + r;
        if (n == 0) lp = 0.0;  // quirk Q14: exactly zero
        else if (n < (uint32_t)OV_NT) lp = (lf[n] - lf[a] - lf[r]) + (row[a] + row[OV_NT + r] - row[2 * OV_NT + n]);
        else {
            const double2 p = ab[l];
            lp = ov_slow_log_pmf(lf, p.x, p.y, a, r);
        }
    }
    lp_out[i] = lp;
}

// cell side of the overflow entries: a thread per cell row evaluates them itself from (alpha, beta) of their loci (a 16-byte
// gather out of a table of L x 16 B that stays in L2) — one log of a ratio of short products per entry — in ascending-locus
// order (sequential: deterministic), and takes the expected terms from the compact E table.  The row's 8-byte entries are
// all the HBM traffic; gathering stored per-entry values instead fetched a 128-byte line per entry (2.3 GB at cfg4 for
// 0.26 GB of values) and slowed the tile kernel beside it more.  k_cell_finalize adds the result to the tile partials.
// (48 VGPRs and no calls: the persistent tile workgroups leave 96 VGPRs per SIMD, so two waves of this kernel fit beside
// them on every SIMD; the entry loop is not unrolled — a row has ~16 overflow entries and hundreds of thousands of rows
// are in flight.  Entries with a total above OV_FAST_N = 8 (1 % of them; longer products, and beyond the tables the generic
// paths: Lanczos ln_gamma, the log-space fold of the expected term) are left to k_ovf_cell_listed, which works off two
// short static lists of exactly those entries.)
// The rows' entries come from a 64-row ELLPACK copy (ovf_ell: entry k of the 64 rows of a group side by side, padded with
// all-ones to the group's longest row): a wave's loads are coalesced and every line is used once.  Reading the CSR row by
// row, a lane per row, re-fetched each row's 128-byte line for every one of its entries (measured 2.1 GB for 0.13 GB).
// PACKED (a big shard's EM pass): alpha, beta and the expected terms out of ONE 64-byte record per locus (k_ovf_tables_e).
// Gathered from two tables an entry fetches two sectors — 2.0 GB per pass at cfg4 on the fabric the tile kernel streams
// through, 1.0 GB this way.  The variant needs 64 VGPRs, i.e. one wave per SIMD beside the tile kernel: all a big shard's
// launch asks for (residency throttle, launch_overflow_cell); a small shard wants two and keeps the 48-VGPR form.
// FULL (a matrix whose overflow share is large — deep coverage — runs the kernel with the machine to itself): totals up to
// OV_NE (17) are taken here too — chunked products, up to three logs, E(n) from the per-locus table — instead of the tier-0
// list, whose one-thread-per-row walk is built for a handful of entries per row (at 13 % overflow entries that kernel alone
// took 12 ms of a 21 ms iteration at 1M x 200k).
template <bool EXPECTED, bool PACKED, bool FULL>
__global__ __launch_bounds__(256) void k_ovf_cell_direct(
    uint64_t n_rows, const uint64_t *__restrict__ ell_ptr, const uint64_t *__restrict__ ell,
    const double2 *__restrict__ ab, const double *__restrict__ lf, const double *__restrict__ etab,
    const double *__restrict__ otab, double *__restrict__ o_ll, double *__restrict__ o_ell)
{
    static_assert(EXPECTED || !PACKED, "the record is built for the EM pass");
    static_assert(!(FULL && PACKED), "the full form runs unthrottled: it takes the unpacked tables");
    const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n_rows) return;  // (rows beyond the end have no lane; their slots are padding)
    double s = 0.0, e = 0.0;
    const uint64_t grp = row >> 6, base = ell_ptr[grp] + (row & 63), end = ell_ptr[grp + 1];
#pragma unroll 1
    for (uint64_t i = base; i < end; i += 64) {
        const uint64_t en = ell[i];
        if (en == OVF_PAD) continue;
        const uint32_t l = ENT_IDX(en), a = ENT_ALT(en), r = ENT_REF(en), n = a + r;
        const double *rec = etab + (uint64_t)l * OV_REC;
        const double2 p = PACKED ? *reinterpret_cast<const double2 *>(rec) : ab[l];
        double ev = 0.0;  // (an overflow entry has a total of 0 or above T_K: the record covers T_K + 1 .. OV_FAST_N)
        if (PACKED) ev = n > (uint32_t)T_K && n <= (uint32_t)OV_FAST_N ? rec[n - 3] : 0.0;
        // masked locus: no PMFData (main.rs:556); 0/0 entry: exactly zero (Q14); a total above OV_FAST_N: k_ovf_cell_listed
        if (!(p.x >= 0.0) || n == 0 || n > (uint32_t)(FULL ? OV_NE : OV_FAST_N)) continue;
        if (FULL && n > (uint32_t)OV_FAST_N) {  // totals 9..17: the tier-0 arithmetic (k_ovf_cell_listed), in the row's order
            s += (lf[n] - lf[a] - lf[r]) + dm_log_beta_ratio(p.x, p.y, a, r);
            if (EXPECTED) e += otab[(uint64_t)l * OV_ROW + OV_EOFF + (n - 4)];
            continue;
        }
        // = dm_log_bb_pmf for these totals: ln C out of the factorial table, one log of a ratio of products of <= 8 factors
        const double abs_ = p.x + p.y;
        double num = 1.0, den = 1.0;
        for (uint32_t k = 0; k < n; ++k) {
            num *= (k < a) ? (p.x + (double)k) : (p.y + (double)(k - a));
            den *= abs_ + (double)k;
        }
        s += (lf[n] - lf[a] - lf[r]) + log(num / den);
        if (EXPECTED) {
            if (PACKED) e += ev;
            else e += n >= 5 ? rec[2 + (n - 5)] : otab[(uint64_t)l * OV_ROW + OV_EOFF + (n - 4)];
        }
    }
    o_ll[row] = s;
    if (EXPECTED) o_ell[row] = e;
}

// Deep coverage (ovf_deep): hundreds of overflow entries per row.  A thread per row walking them one after the other left the
// chip waiting (7.5 ms at 1M x 200k with 13 % overflow entries).  Here 16 lanes share a row: lane j takes the row's entries
// j, j + 16, ... straight out of the overflow CSR (a 128-byte line per 16 lanes), 16 gathers of a row in flight at once, and
// every total up to OV_NE = 17 takes the SAME instruction path — one product loop, one reciprocal, one log: a ratio of two
// products of at most 17 factors stays far inside the f64 range for alpha + beta below 1e17, so no chunking — because a wave
// whose lanes split between a short-total and a long-total path pays for both.  alpha, beta and E(5..8) come out of ONE
// 64-byte record per locus in the EM pass.  The per-lane sums are added by a fixed-shape butterfly (deterministic).
// (Measured and dropped: one launch per locus range whose records fit an L2 — 9.3 -> 11-14 ms: the kernel is bound by its
// arithmetic, not by the gathers.)
template <bool EXPECTED>
__global__ __launch_bounds__(256) void k_ovf_cell_wide(uint64_t n_rows, const uint64_t *__restrict__ ovf_ptr,
                                                       const uint64_t *__restrict__ ovf_ent, const double2 *__restrict__ ab,
                                                       const double *__restrict__ lf, const double *__restrict__ etab,
                                                       const double *__restrict__ otab, double *__restrict__ o_ll,
                                                       double *__restrict__ o_ell)
{
    const uint32_t j = threadIdx.x % LF_LANES;
    const uint64_t row_raw = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / LF_LANES;
    const bool in = row_raw < n_rows;
    const uint64_t row = in ? row_raw : n_rows - 1;  // whole waves stay in the butterflies
    const uint64_t beg = ovf_ptr[row], end = in ? ovf_ptr[row + 1] : beg;
    double s = 0.0, e = 0.0;
#pragma unroll 2
    for (uint64_t i = beg + j; i < end; i += LF_LANES) {
        const uint64_t en = ovf_ent[i];
        const uint32_t l = ENT_IDX(en), a = ENT_ALT(en), r = ENT_REF(en), n = a + r;
        const double *rec = etab + (uint64_t)l * OV_REC;
        const double2 p = EXPECTED ? *reinterpret_cast<const double2 *>(rec) : ab[l];
        double ev = 0.0;
        if (EXPECTED) {
            if (n > (uint32_t)T_K && n <= (uint32_t)OV_FAST_N) ev = rec[n - 3];
            else if (n > (uint32_t)OV_FAST_N && n <= (uint32_t)OV_NE) ev = otab[(uint64_t)l * OV_ROW + OV_EOFF + (n - 4)];
        }
        // masked locus: no PMFData (main.rs:556); 0/0 entry: exactly zero (Q14); totals above OV_NE: the generic list
        if (!(p.x >= 0.0) || n == 0 || n > (uint32_t)OV_NE) continue;
        double lp;
        if (p.x + p.y < 1e17) {
            double num = 1.0, den = 1.0, fa = p.x, fb = p.y, fab = p.x + p.y;
            for (uint32_t k = 0; k < n; ++k) {
                const bool isa = k < a;
                num *= isa ? fa : fb;
                den *= fab;
                fa += isa ? 1.0 : 0.0;
                fb += isa ? 0.0 : 1.0;
                fab += 1.0;
            }
            lp = (lf[n] - lf[a] - lf[r]) + log(num * ov_rcp(den));
        } else {
            lp = ov_slow_log_pmf(lf, p.x, p.y, a, r);
        }
        s += lp;
        if (EXPECTED) e += ev;
    }
    s = group16_sum(s);
    if (EXPECTED) e = group16_sum(e);
    if (in && j == 0) {
        o_ll[row] = s;
        if (EXPECTED) o_ell[row] = e;
    }
}

// ---------------------------------------------------------------------------------------------------------
// tier 2: the overflow entries with 5 <= alt+ref <= 8 (99 % of them at vartrix-like coverage) are table-driven as well.
// Under one (alpha_l, beta_l) their log-pmf depends on (alt, ref) only and a locus carries few distinct pairs, so a pass
// evaluates every (locus, pair) that occurs in the shard ONCE (k_t2_tables: 30 pairs + 4 expected terms per locus at most, a
// static histogram says which occur) into a table in global memory, and both consumers read it:
//   cell side   k_t2_cell: a thread per cell row, four entries' lookups in flight — no arithmetic, a 64-byte sector per entry
//               (it used to evaluate a log of a product ratio per entry with one wave per SIMD beside the tile kernel: 1.2 ms
//               at 10^6 cells x 200k loci for 1.6e7 entries, f64-latency bound);
//   locus side  the minority cells' tier-2 entries are COUNTED per (locus, pair) (k_t2_minority walks the excluded cells'
//               overflow rows: integer atomics, exact and order independent) and k_locus_finalize turns counts x table values
//               into the locus' contributions, like it does for the regular entries.  No per-entry values are stored or read.
// The table row of a locus is six 64-byte sectors [E(n), up to seven log-pmfs of total n]: n = 5, 6, 7 (ref 0..6), 7 (ref 7),
// 8 (ref 0..6), 8 (ref 7, 8) — an entry's log-pmf and expected term share a sector.
// What is left for the per-entry paths: totals 0 (quirk Q14) and above 8 (the tier lists on the cell side, `ovx` on the locus side).
// ---------------------------------------------------------------------------------------------------------
// The pairs that occur in the shard and the sectors that hold at least one of them are STATIC: two lists made at ingest
// (k_t2_lists, in locus order).  One thread per listed pair (blocks [0, gp)) or sector (blocks [gp, ...)): dense waves
// whose lanes all run the same loops.  (A thread per table slot — 48 per locus, most of them idle while a few lanes ran
// the long expected-term loop — took 0.41 ms beside the tile kernel at 200k loci, 0.30 ms on a 125k-cell shard.)
// Slots of pairs that do not occur are never written and never read.  A masked locus (alpha < 0) gets zeros: its
// entries add nothing.
//
// A caching pass (option t2_cache, k_t2_cell<.., CACHE>) has this kernel say which loci it must gather again: blocks [g0, ...)
// take 1024 loci each, a thread per locus and turn, and compare the pass' (alpha, beta) BITS with those the locus' kept values were written under (ab_t2;
// the masked encoding alpha = -1 like any other value) and with the last caching pass' (ab_last, brought up to date here: one
// thread per locus).  A wave writes its 64 loci's dirty bits as two whole words — every word of the mask, every pass, nothing
// to clear — and adds its counts to the pass' pair of counters; the other pair, the previous pass', is cleared for the next.
// Validity is this comparison and nothing else: whatever moved alpha / beta (the exclusion set, the loci mask, a reset, an
// engine switch, a posterior phase in between) shows here, and no call site has anything to invalidate.
struct t2_dirty_t {
    uint32_t *bits;         // null: not a caching pass.  [ceil(L / 64)][2] bit l % 64 of word pair l / 64: locus l is dirty
    uint32_t g0, L;         // first block of the per-locus part; loci
    const double2 *ab_t2;   // [L]
    double2 *ab_last;       // [L]
    uint32_t *cnt, *other;  // [2] dirty loci, loci that moved since the last caching pass: this pass' / the one to clear
};
__device__ __forceinline__ bool ab_differ(double2 a, double2 b)
{
    return __double_as_longlong(a.x) != __double_as_longlong(b.x) || __double_as_longlong(a.y) != __double_as_longlong(b.y);
}
template <bool EXPECTED>
__global__ __launch_bounds__(256) void k_t2_tables(uint32_t n_pairs, const uint32_t *__restrict__ plist /*locus << 5 | pair*/,
                                                   uint32_t n_sec, const uint32_t *__restrict__ slist /*locus << 3 | sector*/,
                                                   uint32_t gp, const double2 *__restrict__ ab, const double *__restrict__ lf,
                                                   double *__restrict__ tab2, uint32_t *__restrict__ grp_ctr /*null: none*/,
                                                   t2_dirty_t dz)
{
    // (the lookups that follow on this stream deal their row groups from this counter: reset here, no memset of its own)
    if (grp_ctr && blockIdx.x == 0 && threadIdx.x == 0) *grp_ctr = 0u;
    if (dz.bits && blockIdx.x == 0 && threadIdx.x == 0) dz.other[0] = dz.other[1] = 0u;
    if (dz.bits && blockIdx.x >= dz.g0) {
        // (a wave takes 256 loci, 64 at a time, and adds its counts once: the lookups wait for this kernel, and thousands of
        //  atomics on one address in front of them are time the side chain does not have beside an all-dirty pass)
        const uint32_t lane = threadIdx.x & 63u, l0 = ((blockIdx.x - dz.g0) * 4u + (threadIdx.x >> 6)) * 256u;
        uint32_t nd = 0, nm = 0;
        for (uint32_t k = 0; k < 4u; k++) {
            const uint32_t l = l0 + k * 64u + lane;
            bool dirty = false, moved = false;
            if (l < dz.L) {
                const double2 p = ab[l];
                dirty = ab_differ(p, dz.ab_t2[l]);
                moved = ab_differ(p, dz.ab_last[l]);
                if (moved) dz.ab_last[l] = p;
            }
            const uint64_t bd = __ballot(dirty), bm = __ballot(moved);
            if (lane == 0u && l < dz.L) {  // (l: the first of the 64 loci, a multiple of 64)
                dz.bits[(l >> 6) * 2] = (uint32_t)bd;
                dz.bits[(l >> 6) * 2 + 1] = (uint32_t)(bd >> 32);
            }
            nd += (uint32_t)__popcll(bd);
            nm += (uint32_t)__popcll(bm);
        }
        if (lane == 0u && nd) atomicAdd(&dz.cnt[0], nd);
        if (lane == 0u && nm) atomicAdd(&dz.cnt[1], nm);
        return;
    }
    if (blockIdx.x < gp) {
        const uint32_t i = blockIdx.x * 256 + threadIdx.x;
        if (i >= n_pairs) return;
        const uint32_t key = plist[i], l = key >> 5, c2 = key & 31u;
        const uint32_t n = 5u + (c2 >= 6u) + (c2 >= 13u) + (c2 >= 21u), r = c2 - t2_code(n, 0u), a = n - r;
        const double2 p = ab[l];
        double v = 0.0;
        if (p.x >= 0.0) {  // = dm_log_bb_pmf for a total of at most DM_CHUNK: one log of a ratio of two short products
            double num = 1.0, den = 1.0, fa = p.x, fb = p.y, fab = p.x + p.y;
#pragma unroll
            for (uint32_t k = 0; k < T2_NMAX; ++k) {  // (one instruction path for every total and split)
                const bool on = k < n, isa = k < a;
                num *= on ? (isa ? fa : fb) : 1.0;
                den *= on ? fab : 1.0;
                fa += isa ? 1.0 : 0.0;
                fb += (on && !isa) ? 1.0 : 0.0;
                fab += 1.0;
            }
            v = (lf[n] - lf[a] - lf[r]) + log(num / den);
        }
        tab2[(uint64_t)l * T2_ROW + t2_pos(n, r)] = v;
    } else if (EXPECTED) {
        const uint32_t i = (blockIdx.x - gp) * 256 + threadIdx.x;
        if (i >= n_sec) return;
        const uint32_t key = slist[i], l = key >> 3, sec = key & 7u;
        const uint32_t n = 5u + (sec >= 1u) + (sec >= 2u) + (sec >= 4u);
        const double2 p = ab[l];
        tab2[(uint64_t)l * T2_ROW + sec * 8u] = p.x >= 0.0 ? ov_expected_rec(p.x, p.y, n) : 0.0;
    }
}

// The same values in the CHUNKED layout of the tier-2 tiles (deep coverage: k_tile_ll<.., geo_t2> reads them out of LDS like the
// regular tables): [chunk][slot][G::LROW] = the pairs' log-pmfs of totals 5..G::NHI, then E(5..G::NHI).  A deep matrix carries
// every pair at nearly every locus, so no lists here: blocks [0, gp) take a (locus, pair) per thread, the others a (locus, total)
// — dense waves that run the same loops (the expected term's recurrence is much longer than a pair's product).  The last slot
// of a chunk and the slots beyond L are never written (zeroed once at build); a masked locus gets zeros.
template <bool EXPECTED, class G>
__global__ __launch_bounds__(256) void k_t2c_tables(uint64_t L, uint32_t gp, const double2 *__restrict__ ab, const double *__restrict__ lf,
                                                    double *__restrict__ tabc)
{
    constexpr uint64_t ELEMS = (uint64_t)G::LROW * G::BL;
    if (blockIdx.x < gp) {
        const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
        const uint64_t l = i / G::NCODE;
        if (l >= L) return;
        const uint32_t c2 = (uint32_t)(i % G::NCODE);
        const uint32_t n = 5u + (c2 >= 6u) + (c2 >= 13u) + (c2 >= 21u), r = c2 - t2_code(n, 0u), a = n - r;
        const double2 p = ab[l];
        double v = 0.0;
        if (p.x >= 0.0) {  // (the arithmetic of k_t2_tables: both sides of a pass add the same bits)
            double num = 1.0, den = 1.0, fa = p.x, fb = p.y, fab = p.x + p.y;
#pragma unroll
            for (uint32_t k = 0; k < T2_NMAX; ++k) {
                const bool on = k < n, isa = k < a;
                num *= on ? (isa ? fa : fb) : 1.0;
                den *= on ? fab : 1.0;
                fa += isa ? 1.0 : 0.0;
                fb += (on && !isa) ? 1.0 : 0.0;
                fab += 1.0;
            }
            v = (lf[n] - lf[a] - lf[r]) + log(num / den);
        }
        tabc[(l / G::BLU) * ELEMS + tab_pmf<G>((uint32_t)(l % G::BLU), c2)] = v;
    } else if (EXPECTED) {
        constexpr uint32_t NE = G::NHI - G::NLO + 1;
        const uint64_t i = (uint64_t)(blockIdx.x - gp) * 256 + threadIdx.x;
        const uint64_t l = i / NE;
        if (l >= L) return;
        const uint32_t n = G::NLO + (uint32_t)(i % NE);
        const double2 p = ab[l];
        tabc[(l / G::BLU) * ELEMS + tab_exp<G>((uint32_t)(l % G::BLU), n - G::NLO)] = p.x >= 0.0 ? ov_expected_rec(p.x, p.y, n) : 0.0;
    }
}

// o[row] += the tier-2 tile pass' partial sums of the row, in group order (the overflow kernels of the side stream wrote o before)
template <bool EXPECTED>
__global__ __launch_bounds__(256) void k_t2_tile_add(uint64_t n_rows, uint32_t groups, uint64_t npad, const double *__restrict__ part_ll,
                                                     const double *__restrict__ part_ell, double *__restrict__ o_ll,
                                                     double *__restrict__ o_ell)
{
    const uint64_t row = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    double s = 0.0, e = 0.0;
    for (uint32_t g = 0; g < groups; g++) {
        s += part_ll[(uint64_t)g * npad + row];
        if (EXPECTED) e += part_ell[(uint64_t)g * npad + row];
    }
    o_ll[row] += s;
    if (EXPECTED) o_ell[row] += e;
}

// cell side: a thread per cell row of the 64-row ELLPACK copy (coalesced entry loads), four entries' lookups in flight;
// sums in the row's order (ascending locus): deterministic.  Entries of other totals (0, above 8) are skipped.
// Waves that take one 64-row group after the other: the launch's grid size sets how many gathers are in flight chip-wide.
// Beside the tile kernel a SMALL grid is the point — every lookup fetches a line out of a table far bigger than an L2, and
// 1.6e7 of them in a burst (2 GB at 5 TB/s) starve the tile kernel's stream for the burst's duration (+0.2 ms at 10^6 cells x 200k
// loci); spread over the tile kernel's run time the same lines cost it far less (launch_overflow_cell).
// A launch on its own strides over the groups by its grid size.  DEAL: the groups are dealt from a device counter (reset by the
// k_t2_tables launch in front), a group per wave and turn, so that launches of different shapes can share one pass' groups: the
// small co-resident grid and the helper grid on the CUs the tile grid leaves free (launch_overflow_cell).  Whichever wave takes
// a group, the row's lane adds the same values in the same order: the output does not depend on the deal.  (U: lookups in
// flight per lane; padding entries add 0.0, so U changes no bit.  Measured and dropped: the entry stream and the gathers as
// non-temporal loads, +0.2 ms per iteration at 10^6 cells)
constexpr unsigned T2_HELP_LDS = 8192;  // dynamic LDS a helper block asks for and does not use: no room beside a tile workgroup
constexpr unsigned T2_HELP_BLOCKS = 4;  // helper blocks (four waves each) per free CU
constexpr int T2_HELP_U = 8;            // lookups in flight per lane of a helper block (registers are not scarce on a free CU)
constexpr unsigned T2_FILL_WAVES = 512;  // co-resident waves of a caching pass that fills (the others: t2_waves' automatic value)
constexpr unsigned T2_FILL_PCT = 25;    // a caching pass fills while at most this share of the loci moved since the last
//
// CACHE (option t2_cache; the EM pass' table set only): an entry's two values are a pure function of its locus' (alpha, beta)
// bits, and those move only at loci touched by a cell that changed sides or whose mask changed — every locus early in a run, a
// few per cent late, none once the exclusion set stands still.  The instance keeps them in `val`, a double2 per slot of the
// ELLPACK copy in the copy's layout (coalesced), and the pass' k_t2_tables says which loci are dirty (t2_dirty_t).  Per pass,
// the same for every wave (the counters are final when the tables kernel ends):
//   clean   no locus is dirty: the row's sums are a sequential stream over `val`, 16 bytes per slot; the entries are not read
//           (slots of padding and of entries outside tier 2 hold the 0.0 the other forms add);
//   fill    every slot's kept values are loaded beside the entries (the two do not depend on each other); entries of dirty loci
//           then gather as ever and STORE what they found in their place; the wave that takes group g
//           also copies the g-th share of the loci's (alpha, beta) to ab_t2 — every group is taken in a pass, so when the pass
//           ends all entries of every locus are written under the bits ab_t2 then holds;
//   bypass  the form without CACHE, bit for bit: nothing stored, ab_t2 untouched, so what was dirty stays dirty.
// fill or bypass (cz.fill; -1: by rule): a pass in which nearly every locus moved would store 16 bytes per slot that the next
// pass, as volatile, never reads.  The rule fills while at most cz.fill_max loci MOVED since the last caching pass — not "are
// dirty": a store that was never filled is all dirty and would never get filled.  The sums add the same values in the same
// order in all three: the output does not depend on the state of the store.
struct t2_cache_t {
    double2 *val;           // [slots of ell]
    const uint32_t *bits;   // the pass' dirty mask (t2_dirty_t)
    const uint32_t *cnt;    // [2] dirty loci, loci that moved
    int fill;               // 1 = fill, 0 = bypass, -1 = fill while cnt[1] <= fill_max
    uint32_t fill_max, L;
    uint32_t calm;          // blocks of the launch that take part in a pass that does not fill (the others end at once)
    const double2 *ab;      // [L] the pass'
    double2 *ab_t2;         // [L]
};
template <bool EXPECTED, int WAVES, int U, bool DEAL, bool CACHE = false>
__global__ __launch_bounds__(64 * WAVES) void k_t2_cell(uint64_t n_rows, const uint64_t *__restrict__ ell_ptr,
                                                        const uint64_t *__restrict__ ell, const double *__restrict__ tab2,
                                                        double *__restrict__ o_ll, double *__restrict__ o_ell,
                                                        uint32_t *__restrict__ grp_ctr, t2_cache_t cz)
{
  const uint64_t n_grp = (n_rows + 63) >> 6;
  const uint32_t lane = threadIdx.x & 63u;
  bool clean = false, fill = false;  // (wave-uniform, and the same in every wave of the pass)
  uint32_t n_blk = gridDim.x;        // blocks that take part
  if constexpr (CACHE) {
      clean = cz.cnt[0] == 0u;
      fill = !clean && (cz.fill >= 0 ? cz.fill != 0 : cz.cnt[1] <= cz.fill_max);
      // How many waves suit a pass depends on what it does, which only the device knows: a filling pass waits on three loads
      // in a row (entry, dirty bit, gather) and moves few bytes, so it takes the whole grid; a bypassing pass is the burst of
      // gathers the small grid was sized for, and the clean stream disturbs the tile kernel least from few waves too.
      if (!fill) n_blk = min(n_blk, cz.calm);
      if (blockIdx.x >= n_blk) return;
  }
  for (uint64_t turn = 0;; turn++) {  // (bounded: every turn takes a group; nothing waits for another wave)
    uint64_t grp;
    if constexpr (DEAL) {
        uint32_t take = 0;
        if (lane == 0) take = atomicAdd(grp_ctr, 1u);
        grp = (uint32_t)__builtin_amdgcn_readfirstlane((int)take);
    } else {
        grp = blockIdx.x + turn * n_blk;  // (one-wave blocks)
    }
    if (grp >= n_grp) break;
    if (CACHE && fill) {  // this group's share of the loci
        const uint64_t per = (cz.L + n_grp - 1) / n_grp, l1 = min((grp + 1) * per, (uint64_t)cz.L);
        for (uint64_t l = grp * per + lane; l < l1; l += 64) cz.ab_t2[l] = cz.ab[l];
    }
    const uint64_t row = grp * 64 + lane;
    if (row < n_rows) {
    double s = 0.0, e = 0.0;
    const uint64_t base = ell_ptr[grp] + lane, end = ell_ptr[grp + 1];
    if (CACHE && clean) {
        for (uint64_t i = base; i < end; i += (uint64_t)U * 64) {
            double2 v[U];
#pragma unroll
            for (int u = 0; u < U; u++)  // (wave-uniform bound)
                v[u] = i + (uint64_t)u * 64 < end ? cz.val[i + (uint64_t)u * 64] : make_double2(0.0, 0.0);
#pragma unroll
            for (int u = 0; u < U; u++) {
                s += v[u].x;
                if (EXPECTED) e += v[u].y;
            }
        }
    } else if (CACHE && fill) {
        for (uint64_t i = base; i < end; i += (uint64_t)U * 64) {
            uint64_t en[U];
            uint32_t dw[U];
            double2 v[U];
#pragma unroll
            for (int u = 0; u < U; u++) {  // the entries and, beside them, not behind them, what is kept for their slots
                const bool in = i + (uint64_t)u * 64 < end;
                en[u] = in ? ell[i + (uint64_t)u * 64] : OVF_PAD;
                v[u] = in ? cz.val[i + (uint64_t)u * 64] : make_double2(0.0, 0.0);
            }
#pragma unroll
            for (int u = 0; u < U; u++) {  // the entry's locus' dirty bit (a 25 KB mask at 200k loci: cache hits)
                const bool ok = en[u] != OVF_PAD && t2_total(ENT_ALT(en[u]) + ENT_REF(en[u]));
                dw[u] = ok ? (cz.bits[ENT_IDX(en[u]) >> 5] >> (ENT_IDX(en[u]) & 31u)) & 1u : 0u;
            }
#pragma unroll
            for (int u = 0; u < U; u++)
                if (dw[u]) {
                    const uint32_t r = ENT_REF(en[u]), n = ENT_ALT(en[u]) + r;
                    const uint64_t at = (uint64_t)ENT_IDX(en[u]) * T2_ROW + t2_pos(n, r);
                    v[u].x = tab2[at];
                    v[u].y = EXPECTED ? tab2[at & ~7ull] : 0.0;
                }
#pragma unroll
            for (int u = 0; u < U; u++) {  // (the stores behind all the loads: U lookups stay in flight)
                if (dw[u]) cz.val[i + (uint64_t)u * 64] = v[u];
                s += v[u].x;
                if (EXPECTED) e += v[u].y;
            }
        }
    } else
    for (uint64_t i = base; i < end; i += (uint64_t)U * 64) {
        uint64_t en[U];
        double lp[U], ev[U];
#pragma unroll
        for (int u = 0; u < U; u++)  // (wave-uniform bound)
            en[u] = i + (uint64_t)u * 64 < end ? ell[i + (uint64_t)u * 64] : OVF_PAD;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t r = ENT_REF(en[u]), n = ENT_ALT(en[u]) + r;
            const bool ok = en[u] != OVF_PAD && t2_total(n);
#ifdef T2_ABL  /* ablation: every lookup falls into the first 1024 loci's rows (384 KB: L2 hits; wrong values) */
            const uint64_t at = (uint64_t)(ENT_IDX(en[u]) & 1023u) * T2_ROW + t2_pos(ok ? n : T2_NMIN, ok ? r : 0u);
#else
            const uint64_t at = (uint64_t)ENT_IDX(en[u]) * T2_ROW + t2_pos(ok ? n : T2_NMIN, ok ? r : 0u);
#endif
            lp[u] = ok ? tab2[at] : 0.0;
            if (EXPECTED) ev[u] = ok ? tab2[at & ~7ull] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            s += lp[u];
            if (EXPECTED) e += ev[u];
        }
    }
    o_ll[row] = s;
    if (EXPECTED) o_ell[row] = e;
    }
    // The lanes of a ragged last group must not go round on their own: the deal at the loop's head is the WAVE's (lane 0 takes,
    // all read).  With `continue` for those lanes the compiler made an inner loop of them that never saw lane 0's take.
    __builtin_amdgcn_wave_barrier();
  }
}

// locus side: the tier-2 entries of the cells of the exclusion set, counted per (locus, pair).  16 lanes per cell walk its
// overflow row (~16 entries: one 128-byte line); scattered integer atomics.  The counters are kept across iterations like
// the regular codes' (tally_plan): with valid counts only the CHANGED cells are walked, +1 for a newly excluded cell and -1
// (u32 wrap-around: exact) for a rescued one — nothing at all once the set stops moving; else the counters were cleared
// (tiled_locus_pass) and the whole new set is counted.  (A change larger than the new set is walked as a change too: its
// atomics are bounded by the two sets, and clearing first would take a launch of its own every iteration.)
__global__ __launch_bounds__(256) void k_t2_minority(const uint32_t *__restrict__ tc, int valid, uint64_t nloc,
                                                     const uint32_t *__restrict__ minlist, const uint32_t *__restrict__ chg,
                                                     const uint64_t *__restrict__ ovf_ptr, const uint64_t *__restrict__ ovf_ent,
                                                     uint32_t *__restrict__ cnt2)
{
    const uint32_t n_a = valid ? tc[1] : tc[0], n = valid ? n_a + tc[2] : n_a;
    const uint32_t j = threadIdx.x % LF_LANES;
    const uint32_t ng = gridDim.x * (256 / LF_LANES);
    for (uint32_t k = (blockIdx.x * 256 + threadIdx.x) / LF_LANES; k < n; k += ng) {
        const uint32_t cell = !valid ? minlist[k] : k < n_a ? chg[k] : chg[nloc - 1 - (k - n_a)];
        const uint32_t inc = k < n_a ? 1u : ~0u;
        for (uint64_t i = ovf_ptr[cell] + j, end = ovf_ptr[cell + 1]; i < end; i += LF_LANES) {
            const uint64_t en = ovf_ent[i];
            const uint32_t r = ENT_REF(en), t = ENT_ALT(en) + r;
            if (t2_total(t)) atomicAdd(&cnt2[(uint64_t)ENT_IDX(en) * T2_CSTRIDE + t2_code(t, r)], inc);
        }
    }
}

// the log-pmfs of the overflow entries OUTSIDE tier 2 (totals 0 and above 8: 1 % of the overflow entries) in by-locus order for
// the locus finalize: a thread per entry, the tier lists' arithmetic (the cell side adds the same bits)
__global__ __launch_bounds__(256) void k_ovx_values(uint64_t n_ovx, const uint32_t *__restrict__ ovx_locus, const uint64_t *__restrict__ ovx_ent,
                                                    const double2 *__restrict__ ab, const double *__restrict__ lf, double *__restrict__ lp_out)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_ovx) return;
    const uint64_t en = ovx_ent[i];
    const double2 p = ab[ovx_locus[i]];
    const uint32_t a = ENT_ALT(en), r = ENT_REF(en), n = a + r;
    double lp = 0.0;  // a masked locus has no PMFData (main.rs:556); a 0/0 entry is exactly zero (quirk Q14)
    if (p.x >= 0.0 && n != 0u)
        lp = n <= (uint32_t)OV_NE ? (lf[n] - lf[a] - lf[r]) + dm_log_beta_ratio(p.x, p.y, a, r) : ov_slow_log_pmf(lf, p.x, p.y, a, r);
    lp_out[i] = lp;
}

// The tier lists (k_ovf_tier_lists: the overflow entries the fast kernel leaves out, in row order; tier 0 = totals 9..OV_NE, tier 1 =
// above).  Their log-pmfs and expected terms, added to the rows' sums: a thread per listed entry; the thread of a row's FIRST listed
// entry walks the row's run (entries of a row are adjacent, in ascending-locus order: deterministic) and updates the row.
// GENERIC = false (tier 0): call-free and light enough to run beside the tile kernel; true (tier 1): dm_* generic paths.
template <bool EXPECTED, bool GENERIC>
__global__ __launch_bounds__(256) void k_ovf_cell_listed(uint64_t n_list, const uint32_t *__restrict__ rows,
                                                         const uint64_t *__restrict__ ents, const double2 *__restrict__ ab,
                                                         const double *__restrict__ lf, const double *__restrict__ otab,
                                                         double *__restrict__ o_ll, double *__restrict__ o_ell)
{
    const uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i0 >= n_list) return;
    const uint32_t row = rows[i0];
    if (i0 > 0 && rows[i0 - 1] == row) return;
    double s = 0.0, e = 0.0;
    for (uint64_t i = i0; i < n_list && rows[i] == row; i++) {
        const uint64_t en = ents[i];
        const uint32_t l = ENT_IDX(en), a = ENT_ALT(en), r = ENT_REF(en), n = a + r;
        const double2 p = ab[l];
        if (!(p.x >= 0.0)) continue;  // masked locus: no PMFData (main.rs:556)
        if (GENERIC) {
            s += dm_log_bb_pmf(lf, p.x, p.y, a, r);
            if (EXPECTED) e += dm_expected_log_pmf(lf, p.x, p.y, n);
        } else {
            s += (lf[n] - lf[a] - lf[r]) + dm_log_beta_ratio(p.x, p.y, a, r);
            if (EXPECTED) e += otab[(uint64_t)l * OV_ROW + OV_EOFF + (n - 4)];
        }
    }
    o_ll[row] += s;
    if (EXPECTED) o_ell[row] += e;
}

// ln sum_k pmf(k)^2 (stats.rs:8-22) for any n, in O(n): the pmfs relative to the one next to the mode, k* = round(n alpha / (alpha +
// beta)), by the ratio recurrence upwards and downwards from there (terms far from the mode underflow to zero harmlessly, none
// overflows: pmf(k) / pmf(k*) stays near or below one), then ln(sum) + 2 ln pmf(k*).  The reference folds all n + 1 log-pmfs in
// log space (O(n^2) the way a thread has to evaluate them); this differs from it by rounding only — engine 1 keeps the fold, and
// every parity test runs both engines.
__device__ __noinline__ double ov_expected_mode(const double *lf, double alpha, double beta, uint32_t n)
{
    const double fn = (double)n;
    uint32_t ks = (uint32_t)(fn * alpha * ov_rcp(alpha + beta) + 0.5);
    if (ks > n) ks = n;
    double s = 1.0, t = 1.0;
    for (uint32_t k = ks; k < n; ++k) {  // pmf(k+1) / pmf(k) = (n-k)(alpha+k) / ((k+1)(beta+n-k-1))
        t *= ((double)(n - k) * (alpha + (double)k)) * ov_rcp((double)(k + 1) * (beta + (double)(n - k - 1)));
        s += t * t;
    }
    t = 1.0;
    for (uint32_t k = ks; k > 0; --k) {  // pmf(k-1) / pmf(k) = k (beta+n-k) / ((n-k+1)(alpha+k-1))
        t *= ((double)k * (beta + (double)(n - k))) * ov_rcp((double)(n - k + 1) * (alpha + (double)(k - 1)));
        s += t * t;
    }
    return log(s) + 2.0 * dm_log_bb_pmf(lf, alpha, beta, ks, n - ks);
}

// Totals above OV_NE (tier 1: a few entries in 10^4 even with deep coverage): chunked products for the log-pmf, the mode-anchored
// recurrence above for the expected term — a thread per listed entry, at most 64 VGPRs so that a wave fits beside the tile kernel's
// four per SIMD.  (Until round 3 the expected term was the reference's log-space fold, 16 lanes per entry.)  The values go to two
// small arrays; k_ovf_listed_add walks each row's run and adds them in list order.
template <bool EXPECTED>
__global__ __launch_bounds__(256, 8) void k_ovf_listed_values(uint64_t n_list, const uint64_t *__restrict__ ents,
                                                              const double2 *__restrict__ ab, const double *__restrict__ lf,
                                                              double *__restrict__ v_lp, double *__restrict__ v_e)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_list) return;
    const uint64_t en = ents[i];
    const uint32_t l = ENT_IDX(en), a = ENT_ALT(en), r = ENT_REF(en), n = a + r;
    const double2 p = ab[l];
    const bool live = p.x >= 0.0;  // else a masked locus: no PMFData (main.rs:556)
    v_lp[i] = live ? dm_log_bb_pmf(lf, p.x, p.y, a, r) : 0.0;
    if (EXPECTED) v_e[i] = live ? ov_expected_mode(lf, p.x, p.y, n) : 0.0;
}
template <bool EXPECTED>
__global__ __launch_bounds__(256) void k_ovf_listed_add(uint64_t n_list, const uint32_t *__restrict__ rows, const double *__restrict__ v_lp,
                                                        const double *__restrict__ v_e, double *__restrict__ o_ll, double *__restrict__ o_ell)
{
    const uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i0 >= n_list) return;
    const uint32_t row = rows[i0];
    if (i0 > 0 && rows[i0 - 1] == row) return;
    double s = 0.0, e = 0.0;
    for (uint64_t i = i0; i < n_list && rows[i] == row; i++) {
        s += v_lp[i];
        if (EXPECTED) e += v_e[i];
    }
    o_ll[row] += s;
    if (EXPECTED) o_ell[row] += e;
}

// chunk-group partials in group order, then the row's overflow sum, then the normalisation (main.rs:314-323).
// Two rows per thread: 16-byte loads and stores (8-byte ones left this 190 MB stream at 1.8 TB/s).
template <bool EXPECTED>
__global__ __launch_bounds__(256) void k_cell_finalize(uint64_t n_rows, uint32_t groups, uint64_t npad,
                                                       const double *__restrict__ part_ll,
                                                       const double *__restrict__ part_ell,
                                                       const double *__restrict__ o_ll /*null: no overflow entries*/,
                                                       const double *__restrict__ o_ell,
                                                       const uint64_t *__restrict__ csr_ptr,
                                                       const uint32_t *__restrict__ masked_cnt, double *__restrict__ ll,
                                                       double *__restrict__ ell, double *__restrict__ nloci,
                                                       double *__restrict__ norm_out)
{
    const uint64_t row = 2 * ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x);
    if (row >= n_rows) return;
    const bool two = row + 1 < n_rows;  // (npad is even and the arrays are 16-byte aligned: a pair never straddles)
    double2 s = make_double2(0.0, 0.0), e = make_double2(0.0, 0.0);
    for (uint32_t g0 = 0; g0 < groups; g0 += 8) {  // eight groups' partials in flight, added in group order
        double2 pl[8], pe[8];
#pragma unroll
        for (uint32_t u = 0; u < 8; u++) {
            const bool ok = g0 + u < groups;
            pl[u] = ok ? *reinterpret_cast<const double2 *>(part_ll + (uint64_t)(g0 + u) * npad + row) : make_double2(0.0, 0.0);
            if (EXPECTED)
                pe[u] = ok ? *reinterpret_cast<const double2 *>(part_ell + (uint64_t)(g0 + u) * npad + row) : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (uint32_t u = 0; u < 8; u++) {
            if (g0 + u < groups) {
                s.x += pl[u].x; s.y += pl[u].y;
                if (EXPECTED) { e.x += pe[u].x; e.y += pe[u].y; }
            }
        }
    }
    if (o_ll) {
        s.x += o_ll[row];
        if (two) s.y += o_ll[row + 1];
        if (EXPECTED) {
            e.x += o_ell[row];
            if (two) e.y += o_ell[row + 1];
        }
    }
    const uint64_t p0 = csr_ptr[row], p1 = csr_ptr[row + 1], p2 = two ? csr_ptr[row + 2] : p1;
    const double c0 = (double)((p1 - p0) - (uint64_t)masked_cnt[row]);
    const double c1 = two ? (double)((p2 - p1) - (uint64_t)masked_cnt[row + 1]) : 0.0;
    const double n0 = c0 > 0.0 ? s.x / c0 : 0.0, n1 = c1 > 0.0 ? s.y / c1 : 0.0;  // main.rs:315-322
    if (two) {
        *reinterpret_cast<double2 *>(ll + row) = s;
        if (EXPECTED) *reinterpret_cast<double2 *>(ell + row) = e;
        *reinterpret_cast<double2 *>(nloci + row) = make_double2(c0, c1);
    } else {
        ll[row] = s.x; nloci[row] = c0;
        if (EXPECTED) ell[row] = e.x;
        if (two) { ll[row + 1] = s.y; nloci[row + 1] = c1; if (EXPECTED) ell[row + 1] = e.y; }
    }
    if (norm_out) {  // a slice of the exchange buffer: starts at the shard's first cell, any parity
        norm_out[row] = n0;
        if (two) norm_out[row + 1] = n1;
    }
}

// ---------------------------------------------------------------------------------------------------------
// locus pass over the compact CSC.  Two entry widths: 24 bits (cell 20 | code 4; four entries = three dwords) when
// the shard has at most 2^20 cells, else 32 bits (cell 28 | code 4).  The pass is a pure HBM stream, so bytes matter.
// ---------------------------------------------------------------------------------------------------------
// Form of the locus pass, decided on the device from this shard's exclusion-set size (LM_NUM / LM_DEN)
// (n_sub = partial planes of the minority-driven form; sub_cap = cells of a subset, i.e. what its 16-bit LDS counters hold: a
// cell adds to one counter as many times as it has entries at one locus — a file may list a (locus, cell) pair any number of
// times, every line being an entry — so a subset takes at most 65535 / (the most entries a cell of this matrix has at one
// locus) cells, and never more than 32767 (tiled_build: lr_cap).  A set too large for that is counted by the streamed form.)
__device__ __forceinline__ bool locus_by_minority(int mode, uint32_t n_min, uint64_t nloc, uint32_t n_sub, uint32_t sub_cap)
{
    if ((uint64_t)n_min > (uint64_t)n_sub * sub_cap) return false;
    return mode == 2 || (mode == 0 && (uint64_t)n_min * LM_DEN <= nloc * LM_NUM);
}

// The regular-code counts of the exclusion set per (locus, code) are KEPT across iterations (ctx tally, u32 [L][16]) and
// updated from the set's change: new = old + the entries of the newly excluded cells - those of the rescued ones (integers:
// exact and order independent; u32 wrap-around is exact too, every final count being non-negative).  The set hardly moves
// once the loop settles (every timed bench step: no change), so the count kernels then return at once.  Per iteration, on the
// device (tc = d_counters + DC_N_MIN: new set, newly excluded, rescued):
//   valid, no change            nothing is counted, k_locus_finalize reads the kept plane
//   valid, change <= new set    the minority-driven form walks the CHANGED cells' rows: a subset of the partial planes per
//                               sign (u16 counters: a subset never mixes the two signs), k_locus_finalize adds them with
//                               their signs to the kept plane and stores it back
//   otherwise                   a recount of the new set: the minority-driven form (its planes replace the kept plane) or the
//                               streamed one (k_locus_stats2 overwrites it), chosen as before (locus_mode)
// A subset takes at least TALLY_SUB_CELLS cells (one batch of k_minority_ranges): a small change is few planes to add — or
// sub_cap cells where that is less (a matrix that lists a pair 64 times or more), so that k_minority_ranges' share of
// ceil(n / subsets) cells never exceeds sub_cap: with n <= n_sub * sub_cap (tally_plan) both arms of the min keep it.
#define TALLY_SUB_CELLS 1024
struct TallyPlan {
    uint32_t n_a, n_r;  // cells counted with sign + (list positions 0 .. n_a-1) and - (n_a .. n_a+n_r-1)
    uint32_t s_a, s_r;  // subsets (u16 partial planes) of either sign
    bool delta;         // the list is the change (k_flag's chg), else the new set (minlist)
    bool fresh;         // minority-driven recount: the planes replace the kept counts
    bool stream;        // streamed recount (k_locus_stats2)
};
__device__ __forceinline__ uint32_t tally_subsets(uint32_t n, uint32_t n_sub, uint32_t sub_cap)
{
    const uint32_t per = max(1u, min((uint32_t)TALLY_SUB_CELLS, sub_cap));  // (sub_cap 0: only an empty list gets here)
    return min(n_sub, (n + per - 1) / per);
}
__device__ __forceinline__ TallyPlan tally_plan(int mode, int valid, const uint32_t *tc, uint64_t nloc, uint32_t n_sub, uint32_t sub_cap)
{
    const uint32_t n_min = tc[0], n_add = tc[1], n_res = tc[2];
    TallyPlan p = {0u, 0u, 0u, 0u, false, false, false};
    if (valid) {
        const uint64_t n_chg = (uint64_t)n_add + n_res, cap = (uint64_t)n_sub * sub_cap;
        if (n_chg == 0) return p;
        // (the transposed offsets hold nloc * LM_NUM / LM_DEN cells whatever the locus_mode: tiled_locus_pass)
        if (n_chg <= n_min && n_chg * LM_DEN <= nloc * LM_NUM && n_add <= cap && n_res <= cap) {
            p.delta = true;
            p.n_a = n_add; p.n_r = n_res;
            p.s_a = tally_subsets(n_add, n_sub, sub_cap); p.s_r = tally_subsets(n_res, n_sub, sub_cap);
            return p;
        }
    }
    if (locus_by_minority(mode, n_min, nloc, n_sub, sub_cap)) {
        p.fresh = true;
        p.n_a = n_min;
        p.s_a = tally_subsets(n_min, n_sub, sub_cap);
    } else {
        p.stream = true;
    }
    return p;
}
// the k-th cell of the plan's list
__device__ __forceinline__ uint32_t tally_cell(const TallyPlan &p, const uint32_t *__restrict__ minlist,
                                               const uint32_t *__restrict__ chg, uint64_t nloc, uint32_t k)
{
    if (!p.delta) return minlist[k];
    return k < p.n_a ? chg[k] : chg[nloc - 1 - (k - p.n_a)];
}

struct __attribute__((packed, aligned(4))) ls_u3 { uint32_t x, y, z; };  // 12-byte load at a 4-byte aligned address
#define LS_THREADS 1024
template <bool BITS_IN_LDS, int EB>
__global__ __launch_bounds__(LS_THREADS) void k_locus_stats2(uint64_t L, uint32_t nbits_words,
                                                             const uint64_t *__restrict__ c4_ptr,
                                                             const uint32_t *__restrict__ c4_ent,
                                                             const uint32_t *__restrict__ flag_bits,
                                                             uint32_t *__restrict__ tally, int locus_mode, int valid,
                                                             uint64_t nloc, const uint32_t *__restrict__ tc, uint32_t n_sub, uint32_t sub_cap)
{
    if (!tally_plan(locus_mode, valid, tc, nloc, n_sub, sub_cap).stream) return;  // kept counts, or k_minority_ranges counts
    extern __shared__ uint32_t s_bits[];
    __shared__ uint32_t s_whist[LS_THREADS / 64][16];
    if (threadIdx.x < (LS_THREADS / 64) * 16) (&s_whist[0][0])[threadIdx.x] = 0;
    if (BITS_IN_LDS)
        for (uint32_t i = threadIdx.x; i < nbits_words; i += LS_THREADS) s_bits[i] = flag_bits[i];
    __syncthreads();
    uint32_t *whist = s_whist[threadIdx.x >> 6];
    const uint32_t *bits = BITS_IN_LDS ? s_bits : flag_bits;
    const int lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t)blockIdx.x * (LS_THREADS / 64) + (threadIdx.x >> 6);
    const uint64_t nwaves = (uint64_t)gridDim.x * (LS_THREADS / 64);
    // the column pointers of a locus are requested one locus ahead, its per-code constants at the top of its turn: a
    // short column (a small shard) then costs one memory latency, not three in a row
    uint64_t n_c4b = 0, n_c4e = 0;
    if (wave0 < L) { n_c4b = c4_ptr[wave0]; n_c4e = c4_ptr[wave0 + 1]; }
    for (uint64_t l = wave0; l < L; l += nwaves) {
        // columns are padded to groups of four entries (code 15 = no entry): 16 bytes at 32 bits, 12 bytes at 24 bits
        const uint64_t vbeg = n_c4b >> 2, nvec = (n_c4e >> 2) - vbeg;
        const uint32_t *wp = c4_ent + vbeg * (EB == 32 ? 4 : 3);
        {
            const uint64_t ln = min(l + nwaves, L - 1);  // clamped: the last round re-reads a valid locus
            n_c4b = c4_ptr[ln]; n_c4e = c4_ptr[ln + 1];
        }
        // minority entries are few: they vote into this wave's 16-bin LDS histogram (integer atomics: exact).  Two
        // register buffers of four vectors (16 entries) per lane: one is processed while the other one loads.
        struct raw_t { uint32_t w[4][EB == 32 ? 4 : 3]; uint32_t in; };  // in: bit u = vector u lies inside the column
        // (the macros keep the buffers in named registers: no indexed local arrays).  The loads are unconditional (index
        // clamped) and nothing touches the loaded registers before LS_PROCESS: they stay in flight meanwhile.
#define LS_LOAD(R, I0)                                                                                           \
        (R).in = 0;                                                                                              \
        _Pragma("unroll") for (int u = 0; u < 4; u++) {                                                          \
            const uint64_t i__ = (I0) + (uint64_t)u * 64 + lane;                                                 \
            const bool in__ = i__ < nvec;                                                                        \
            (R).in |= in__ ? (1u << u) : 0u;                                                                     \
            const uint32_t *q__ = wp + (in__ ? i__ : 0) * (EB == 32 ? 4 : 3);                                    \
            if (EB == 32) {                                                                                      \
                const uint4 v__ = *reinterpret_cast<const uint4 *>(q__);                                         \
                (R).w[u][0] = v__.x; (R).w[u][1] = v__.y; (R).w[u][2] = v__.z; (R).w[u][EB == 32 ? 3 : 0] = v__.w; \
            } else {                                                                                             \
                const ls_u3 v__ = *reinterpret_cast<const ls_u3 *>(q__);                                         \
                (R).w[u][0] = v__.x; (R).w[u][1] = v__.y; (R).w[u][2] = v__.z;                                   \
            }                                                                                                    \
        }
        // unpack 16 (cell, code) pairs, fetch their 16 bitmask words back to back, then vote.  Padding (and a vector
        // beyond the column: all ones) is cell = all ones, code 15: with the bitmask in LDS its word is inside the
        // allocation (sized for the largest cell index of the entry width) and bin 15 of the histogram is never read.
#define LS_PROCESS(R)                                                                                            \
        do {                                                                                                     \
            uint32_t cell__[16], code__[16], word__[16];                                                         \
            _Pragma("unroll") for (int u = 0; u < 4; u++) {                                                      \
                const bool in__ = (((R).in >> u) & 1u) != 0;                                                     \
                if (EB == 32) {                                                                                  \
                    _Pragma("unroll") for (int q = 0; q < 4; q++) {                                              \
                        const uint32_t x__ = in__ ? (R).w[u][EB == 32 ? q : 0] : ~0u;                            \
                        cell__[4 * u + q] = x__ & 0x0fffffffu; code__[4 * u + q] = x__ >> 28;                    \
                    }                                                                                            \
                } else {                                                                                         \
                    const uint32_t w0 = in__ ? (R).w[u][0] : ~0u, w1 = in__ ? (R).w[u][1] : ~0u,                 \
                                   w2 = in__ ? (R).w[u][2] : ~0u;                                                \
                    const uint32_t es__[4] = {w0 & 0xffffffu, (w0 >> 24) | ((w1 & 0xffffu) << 8),               \
                                              (w1 >> 16) | ((w2 & 0xffu) << 16), w2 >> 8};                       \
                    _Pragma("unroll") for (int q = 0; q < 4; q++) {                                              \
                        cell__[4 * u + q] = es__[q] & 0xfffffu; code__[4 * u + q] = es__[q] >> 20;               \
                    }                                                                                            \
                }                                                                                                \
            }                                                                                                    \
            _Pragma("unroll") for (int e = 0; e < 16; e++) {                                                     \
                if (!(BITS_IN_LDS && EB == 24) && code__[e] >= (uint32_t)T_NCODE) cell__[e] = 0u; /* stay in range */ \
                word__[e] = bits[cell__[e] >> 5];                                                                \
            }                                                                                                    \
            _Pragma("unroll") for (int e = 0; e < 16; e++)                                                       \
                if ((word__[e] >> (cell__[e] & 31)) & 1u) atomicAdd(&whist[code__[e]], 1u);                      \
        } while (0)

        if (nvec) {
            raw_t ra, rb;
            LS_LOAD(ra, 0);
            for (uint64_t i0 = 0; i0 < nvec; i0 += 2 * 4 * 64) {
                LS_LOAD(rb, i0 + 4 * 64);
                LS_PROCESS(ra);
                LS_LOAD(ra, i0 + 2 * 4 * 64);
                LS_PROCESS(rb);
            }
        }
#undef LS_PROCESS
#undef LS_LOAD
        // the wave's bins are this locus' minority counts per code: the kept plane (same wave wrote the bins: LDS
        // operations of one wave complete in order); k_locus_finalize turns them into the pass' outputs
        if (lane < 16) {
            tally[l * 16 + lane] = whist[lane];
            whist[lane] = 0;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// locus pass, minority-driven form.  Everything the pass reports follows from the per-(locus, code) counts of the
// MINORITY cells' regular entries (the majority side is the static histogram minus that), and the exclusion set is a
// small part of the cells (below the lower quartile by construction, a few percent in practice).  So instead of
// streaming the whole compact CSC past the exclusion bitmask, walk only the by-cell CSR rows of the excluded cells.
// Global atomics are out (measured: 2.7e10 scattered u32 atomics/s on this chip, 3.7 ms for cfg4's 1e8 entries), so
// the counting happens in LDS: the loci are cut into ranges of LR_LOCI, a workgroup owns one range and one of n_sub
// subsets of the excluded cells, finds every such cell's entries of its range through a per-(cell, range) offset
// table built at ingest (roff), counts them into a u32 histogram in LDS (integer atomics: exact, order independent)
// and writes the histogram out as one of n_sub partial planes; k_locus_finalize adds the planes.  The result is
// bit-identical to the streamed form.  Cost: the excluded cells' entries instead of all of them.  The form is chosen
// on the device from this shard's exclusion-set size (no host round trip); the kernels of the other form return at once.
// ---------------------------------------------------------------------------------------------------------
// The excluded cells' offset rows, gathered and transposed: mroff[r][k] for the k-th cell of minlist, mbeg[k] = start of its
// row.  k_minority_ranges then reads its range's offsets as contiguous runs instead of one 64-byte line per (cell, range)
// out of the big per-cell table (measured: those line fetches were a third of that kernel's traffic).
__global__ __launch_bounds__(256) void k_minority_offsets(int locus_mode, int valid, uint64_t nloc, uint32_t n_sub, uint32_t sub_cap, uint32_t R,
                                                          uint64_t mstride, const uint32_t *__restrict__ tc,
                                                          const uint32_t *__restrict__ minlist, const uint32_t *__restrict__ chg,
                                                          const uint64_t *__restrict__ csr_ptr,
                                                          const uint32_t *__restrict__ roff, uint32_t *__restrict__ mroff,
                                                          uint64_t *__restrict__ mbeg)
{
    const TallyPlan tp = tally_plan(locus_mode, valid, tc, nloc, n_sub, sub_cap);
    const uint32_t n_list = tp.n_a + tp.n_r;  // the plan's list (none: the streamed form, or no change)
    const uint32_t k0 = blockIdx.x * LT_CELLS;
    if (k0 >= n_list) return;
    extern __shared__ uint32_t s_t[];  // [LT_CELLS][row], row odd: the column read below strides by it
    __shared__ uint32_t s_cell[LT_CELLS];
    const uint32_t row = (R + 1) | 1u, nk = min((uint32_t)LT_CELLS, n_list - k0);
    if (threadIdx.x < nk) {
        const uint32_t cell = tally_cell(tp, minlist, chg, nloc, k0 + threadIdx.x);
        s_cell[threadIdx.x] = cell;
        mbeg[k0 + threadIdx.x] = csr_ptr[cell];
    }
    __syncthreads();
    // every cell's offsets are one contiguous run of R + 1 words: all threads stride over the (cell, range) pairs, so
    // that many independent loads are in flight
    const uint32_t tot = nk * (R + 1);
#pragma unroll 8
    for (uint32_t i = threadIdx.x; i < tot; i += 256) {
        const uint32_t c = i / (R + 1), r = i - c * (R + 1);
        s_t[c * row + r] = roff[(uint64_t)s_cell[c] * (R + 1) + r];
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < (R + 1) * LT_CELLS; i += 256) {
        const uint32_t r = i / LT_CELLS, c = i % LT_CELLS;
        if (c < nk) mroff[(uint64_t)r * mstride + k0 + c] = s_t[c * row + r];
    }
}

__global__ __launch_bounds__(LR_THREADS) void k_minority_ranges(int locus_mode, int valid, uint64_t nloc, uint64_t L, uint32_t R,
                                                               uint32_t n_sub, uint32_t sub_cap, uint64_t mstride,
                                                               const uint32_t *__restrict__ tc,
                                                               const uint32_t *__restrict__ mroff,
                                                               const uint64_t *__restrict__ mbeg,
                                                               const uint16_t *__restrict__ c4r,
                                                               uint32_t *__restrict__ hist_min /*[2 n_sub][L][16] u16*/)
{
    // (grid: R x 2 n_sub workgroups; those beyond the plan's subsets return)
    const TallyPlan tp = tally_plan(locus_mode, valid, tc, nloc, n_sub, sub_cap);
    const uint32_t sub = blockIdx.x / R;
    if (sub >= tp.s_a + tp.s_r) return;
    // u16 counters, two per word, code-major: the bank of a counter follows the locus (spread out), not the code (most
    // entries are single reads: codes 0 and 1).  A subset has at most sub_cap cells (tally_plan), each with at most 65535 / sub_cap
    // entries at one locus: no carry.  Its cells
    // are all of one sign (k_locus_finalize adds or subtracts the whole plane).
    __shared__ uint32_t s_hist[T_NCODE * LR_ROW / 2];
    __shared__ uint64_t s_beg[LR_THREADS];
    __shared__ uint32_t s_len[LR_THREADS];
    const uint32_t tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const uint32_t r = blockIdx.x % R;
    const bool neg = sub >= tp.s_a;
    const uint32_t lo = neg ? tp.n_a : 0u, n_sign = neg ? tp.n_r : tp.n_a, s_sign = neg ? tp.s_r : tp.s_a;
    const uint32_t q = neg ? sub - tp.s_a : sub;
    const uint32_t per = (n_sign + s_sign - 1) / s_sign;
    const uint32_t k0 = lo + min(n_sign, q * per), k1 = lo + min(n_sign, q * per + per);
    const uint32_t l0 = r * LR_LOCI;
    for (uint32_t i = tid; i < T_NCODE * LR_ROW / 2; i += LR_THREADS) s_hist[i] = 0;
    const uint32_t grp = lane / LR_GROUP, gl = lane % LR_GROUP;
#define LR_COUNT(E)                                                                                              \
    do {                                                                                                         \
        if (((E) >> 12) < (uint32_t)T_NCODE) {                                                                   \
            const uint32_t idx__ = ((E) >> 12) * LR_ROW + ((E) & 0x0fffu);                                       \
            atomicAdd(&s_hist[idx__ >> 1], 1u << ((idx__ & 1u) * 16u));                                          \
        }                                                                                                        \
    } while (0)
    // one excluded cell per thread: where its entries of this range start, and how many there are (requested one batch
    // ahead, so the loads fly during the batch before)
    uint64_t p_b = 0;
    uint32_t p_n = 0;
#define LR_PREFETCH(KB)                                                                                          \
    do {                                                                                                         \
        const uint32_t k__ = (KB) + tid;                                                                         \
        p_b = 0; p_n = 0;                                                                                        \
        if (k__ < k1) {                                                                                          \
            const uint32_t o0__ = mroff[(uint64_t)r * mstride + k__], o1__ = mroff[(uint64_t)(r + 1) * mstride + k__]; \
            p_b = mbeg[k__] + o0__;                                                                              \
            p_n = o1__ - o0__;                                                                                   \
        }                                                                                                        \
    } while (0)
    LR_PREFETCH(k0);
    for (uint32_t kb = k0; kb < k1; kb += LR_THREADS) {
        s_beg[tid] = p_b;
        s_len[tid] = p_n;
        __syncthreads();  // (also: the histogram is zeroed)
        LR_PREFETCH(kb + LR_THREADS);
        // a wave takes 64 of the segments, LR_GROUP lanes per segment; per trip the first LR_GROUP entries of 32 of them
        // are requested back to back (16 loads per lane in flight), then counted; longer segments finish in a loop
        constexpr int SPW = 64 / LR_GROUP;  // segments per wave load
        constexpr int NQ = 16;
        for (uint32_t q0 = 0; q0 < 64 / SPW; q0 += NQ) {
            uint32_t e[NQ];
#pragma unroll
            for (int u = 0; u < NQ; u++) {
                const uint32_t seg = wv * 64 + (q0 + u) * SPW + grp;
                e[u] = gl < s_len[seg] ? (uint32_t)c4r[s_beg[seg] + gl] : 0xffffu;  // all ones: code 15, not counted
            }
#pragma unroll
            for (int u = 0; u < NQ; u++) LR_COUNT(e[u]);
            for (int u = 0; u < NQ; u++) {
                const uint32_t seg = wv * 64 + (q0 + u) * SPW + grp;
                const uint32_t sn = s_len[seg];
                const uint64_t sb = s_beg[seg];
                for (uint32_t j = gl + LR_GROUP; j < sn; j += LR_GROUP) {
                    const uint32_t x = (uint32_t)c4r[sb + j];
                    LR_COUNT(x);
                }
            }
        }
        __syncthreads();  // segments consumed before the next batch overwrites them
    }
#undef LR_PREFETCH
#undef LR_COUNT
    __syncthreads();
    // this subset's plane of the range, as [locus][16] u16 like the counters (codes 14, 15: zero): 32 bytes per locus
    // and plane for this kernel to write and k_locus_finalize to read
    const uint64_t nl = min((uint64_t)LR_LOCI, L - l0);
    uint32_t *dst = reinterpret_cast<uint32_t *>(reinterpret_cast<uint16_t *>(hist_min) + ((uint64_t)sub * L + l0) * 16);
    for (uint32_t i = tid; i < nl * 8; i += LR_THREADS) {
        const uint32_t lo = i >> 3, c0 = (i & 7u) * 2u;
        uint32_t v = 0;
#pragma unroll
        for (uint32_t h = 0; h < 2; h++) {
            const uint32_t code = c0 + h, idx = code * LR_ROW + lo;
            if (code < (uint32_t)T_NCODE) v |= ((s_hist[idx >> 1] >> ((idx & 1u) * 16u)) & 0xffffu) << (16u * h);
        }
        dst[i] = v;
    }
}

// Outputs of the locus pass from the minority counts (both forms end here, so they agree to the bit).  16 lanes per
// locus: lane j < 14 takes code j's count (sum of the planes), static histogram and log-pmf; the locus' overflow entries
// (alt+ref == 0 or > T_K; ~1 %, their log-pmfs evaluated from the locus' cumulative-log row) are walked 16 at a time; per-lane partial results
// are added by a 4-step butterfly over the 16 lanes (fixed shape: deterministic).
template <bool INLINE_OVF>  // the overflow entries' log-pmfs: evaluated here (deep coverage) or read from ovf_lp (k_ovf_values)
__global__ __launch_bounds__(256) void k_locus_finalize(uint64_t L, int locus_mode, int valid, uint64_t nloc, uint32_t n_sub, uint32_t sub_cap,
                                                        const uint32_t *__restrict__ tc,
                                                        const uint32_t *__restrict__ hist_min, uint32_t *__restrict__ tally,
                                                        const uint32_t *__restrict__ flag_bits,
                                                        const uint32_t *__restrict__ hist_all,
                                                        const double *__restrict__ tab, uint32_t tab_stride,
                                                        const uint8_t *__restrict__ mask,
                                                        const uint64_t *__restrict__ ovc_ptr /*null: no overflow*/,
                                                        const uint64_t *__restrict__ ovc_ent,
                                                        const double *__restrict__ ovf_lp /*null: evaluate here*/,
                                                        const double *__restrict__ otab, const double *__restrict__ lf,
                                                        const double2 *__restrict__ ab, double *__restrict__ out,
                                                        const uint32_t *__restrict__ cnt2 /*null: no tier 2*/,
                                                        const uint32_t *__restrict__ hist_all2, const uint32_t *__restrict__ pmask2,
                                                        const double *__restrict__ tab2,
                                                        uint8_t *__restrict__ mask_next /*null: the locus filter is a kernel of its own*/,
                                                        uint32_t *__restrict__ n_filtered)
{
    // the kept u32 counts (filled by k_locus_stats2 if it recounted), plus / minus this iteration's u16 partial planes
    const TallyPlan tp = tally_plan(locus_mode, valid, tc, nloc, n_sub, sub_cap);
    const uint32_t n_planes = tp.s_a + tp.s_r;
    const uint32_t j = threadIdx.x % LF_LANES;
    const uint64_t l_raw = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / LF_LANES;
    const bool in = l_raw < L;
    const uint64_t l = in ? l_raw : L - 1;  // whole waves stay in the butterflies
    const bool live = mask[l] != 0;
    uint64_t obeg = 0, oend = 0;
    if (ovc_ptr) { obeg = ovc_ptr[l]; oend = ovc_ptr[l + 1]; }
    double cmin = 0.0, cmaj = 0.0;
    uint32_t nmin = 0;
    uint64_t amin = 0, rmin = 0;
    if (j < T_NCODE) {
        uint32_t cnt = tp.fresh ? 0u : tally[l * 16 + j];
        if (n_planes) {
            const uint16_t *h16 = reinterpret_cast<const uint16_t *>(hist_min);
            for (uint32_t p = 0; p < tp.s_a; p++) cnt += h16[((uint64_t)p * L + l) * 16 + j];
            for (uint32_t p = tp.s_a; p < n_planes; p++) cnt -= h16[((uint64_t)p * L + l) * 16 + j];
        }
        if (in && (n_planes || tp.fresh)) tally[l * 16 + j] = cnt;  // the counts of the new set, kept for the next iteration
        const uint32_t h_all = hist_all[l * T_NCODE + j];
        // (element stride 2 when the table holds (log-pmf, expected) pairs)
        const double t_code = tab[(l / T_BLU) * TAB_ELEMS + tab_pmf<geo_reg>((uint32_t)(l % T_BLU), j)];
        amin = (uint64_t)cnt * T_A_OF[j];
        rmin = (uint64_t)cnt * T_R_OF[j];
        if (live) {
            nmin = cnt;
            cmin = (double)cnt * t_code;
            cmaj = (double)(h_all - cnt) * t_code;
        }
    }
    // tier 2 (the overflow entries with totals 5..8, counted per (locus, pair) by k_t2_minority): lane j takes the pairs j and
    // j + 16; count x table value, like the regular codes.  The counters are kept for the next iteration.
    if (cnt2) {
        const uint32_t pm = pmask2[l];  // (the pairs that occur at this locus, static: 8 of the 30 on a 125k-cell shard)
#pragma unroll
        for (uint32_t h = 0; h < 2; h++) {
            const uint32_t c2 = j + h * LF_LANES;
            if (!((pm >> c2) & 1u)) continue;  // the pair does not occur at this locus: no counts, no table slot
            const uint32_t h_all = hist_all2[l * T2_CSTRIDE + c2];
            const uint32_t cnt = cnt2[l * T2_CSTRIDE + c2];
            const uint32_t n2 = 5u + (c2 >= 6u) + (c2 >= 13u) + (c2 >= 21u), r2 = c2 - t2_code(n2, 0u);
            const double t_code = tab2[l * T2_ROW + t2_pos(n2, r2)];
            amin += (uint64_t)cnt * (n2 - r2);
            rmin += (uint64_t)cnt * r2;
            if (live) {
                nmin += cnt;
                cmin += (double)cnt * t_code;
                cmaj += (double)(h_all - cnt) * t_code;
            }
        }
    }
    // overflow entries: four independent entry loads per lane in flight, then their exclusion-bitmask words and their
    // log-pmfs = lnC + LA[alt] + LB[ref] - LAB[n] out of the locus' cumulative-log row (k_ovf_tables; the 16 lanes share the
    // row: L1) — evaluated here instead of being stored by a kernel of their own and read back (12 + 8 + 8 bytes per entry)
    const double *orow = otab + l * OV_ROW;
    for (uint64_t i0 = obeg + j; i0 < oend; i0 += 4 * LF_LANES) {
        uint64_t en[4];
        double lp[4];
        uint32_t w[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint64_t i = i0 + (uint64_t)u * LF_LANES;
            en[u] = i < oend ? ovc_ent[i] : ~0ull;
            lp[u] = (!INLINE_OVF && i < oend) ? ovf_lp[i] : 0.0;  // (stored by k_ovf_values: zero at masked loci)
        }
#pragma unroll
        for (int u = 0; u < 4; u++) w[u] = en[u] != ~0ull ? flag_bits[ENT_IDX(en[u]) >> 5] : 0u;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (!INLINE_OVF) break;
            lp[u] = 0.0;
            if (en[u] == ~0ull || !live) continue;  // (a masked locus has no PMFData, main.rs:556: only its tallies count)
            const uint32_t a = ENT_ALT(en[u]), r = ENT_REF(en[u]), n = a + r;
            if (n == 0) lp[u] = 0.0;  // quirk Q14: exactly zero
            else if (n < (uint32_t)OV_NT)  // (totals below 18: ln C straight out of the factorial table — no ln_gamma branch inlined here)
                lp[u] = (lf[n] - lf[a] - lf[r]) + (orow[a] + orow[OV_NT + r] - orow[2 * OV_NT + n]);
            else {
                const double2 p = ab[l];
                lp[u] = ov_slow_log_pmf(lf, p.x, p.y, a, r);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (en[u] == ~0ull) continue;
            const bool minority = ((w[u] >> (ENT_IDX(en[u]) & 31)) & 1u) != 0;
            if (minority) { amin += ENT_ALT(en[u]); rmin += ENT_REF(en[u]); }
            if (live) {
                if (minority) { cmin += lp[u]; nmin++; } else cmaj += lp[u];
            }
        }
    }
    cmin = group16_sum(cmin);
    cmaj = group16_sum(cmaj);
    nmin = group16_sum(nmin);
    amin = group16_sum(amin);
    rmin = group16_sum(rmin);
    if (in && j == 0) {
        out[LB_CONTRIB_MIN * L + l] = cmin;
        out[LB_CONTRIB_MAJ * L + l] = cmaj;
        out[LB_CELLS_MIN * L + l] = (double)nmin;
        out[LB_ALT_MIN * L + l] = (double)amin;
        out[LB_REF_MIN * L + l] = (double)rmin;
        // An unsharded ctx has the locus' final sums right here: the -80 filter of locus_filter_and_output_locus_data
        // (main.rs:428-451; k_locus_filter's arithmetic on the values just written) without a launch of its own.
        if (mask_next) {
            const double fn = (double)nmin;
            const double per_cell = fn != 0.0 ? cmin / fn : 0.0;
            uint8_t m = mask[l];
            if (per_cell < -80.0) {
                m = 0;
                atomicAdd(n_filtered, 1u);
            }
            mask_next[l] = m;
        }
    }
}

// entries of newly masked loci no longer count as used loci of their cells (main.rs:556,575)
template <int EB>
__global__ __launch_bounds__(256) void k_masked_update(uint64_t L, const uint8_t *__restrict__ mask_old,
                                                       const uint8_t *__restrict__ mask_new,
                                                       const uint64_t *__restrict__ c4_ptr,
                                                       const uint32_t *__restrict__ c4_ent,
                                                       const uint64_t *__restrict__ ovc_ptr,
                                                       const uint64_t *__restrict__ ovc_ent,
                                                       uint32_t *__restrict__ masked_cnt)
{
    const int lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * 4;
    for (uint64_t l = wave0; l < L; l += nwaves) {
        if (!(mask_old[l] && !mask_new[l])) continue;
        for (uint64_t i = c4_ptr[l] + lane; i < c4_ptr[l + 1]; i += 64) {
            uint32_t cell, code;
            c4_read1<EB>(c4_ent, i, &cell, &code);
            if (code < (uint32_t)T_NCODE) atomicAdd(&masked_cnt[cell], 1u);
        }
        for (uint64_t i = ovc_ptr[l] + lane; i < ovc_ptr[l + 1]; i += 64) atomicAdd(&masked_cnt[ENT_IDX(ovc_ent[i])], 1u);
    }
}

// ---------------------------------------------------------------------------------------------------------
// posterior phase (calculate_posteriors, main.rs:228-280)
// ---------------------------------------------------------------------------------------------------------
__global__ void k_ab_posterior3(uint64_t L, const double *__restrict__ s_alt, const double *__restrict__ s_ref,
                                const double *__restrict__ alt_min, const double *__restrict__ ref_min, double mf0,
                                double2 *__restrict__ ab3, double *__restrict__ ab6)
{
    const uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= L) return;
    double a_maj = (s_alt[l] + 1.0) - alt_min[l], b_maj = (s_ref[l] + 1.0) - ref_min[l];          // main.rs:239
    const double a_min = (s_alt[l] + 1.0) - (s_alt[l] - alt_min[l]);                                // main.rs:241
    const double b_min = (s_ref[l] + 1.0) - (s_ref[l] - ref_min[l]);
    const double a_dbl = (a_maj - 1.0) * mf0 + (a_min - 1.0) + 1.0;                                 // main.rs:245
    const double b_dbl = (b_maj - 1.0) * mf0 + (b_min - 1.0) + 1.0;
    const double mf = fmax(mf0, 0.01);                                                              // main.rs:250
    a_maj = (a_maj - 1.0) * mf + 1.0;                                                               // main.rs:252
    b_maj = (b_maj - 1.0) * mf + 1.0;
    ab3[l] = make_double2(a_min, b_min);
    ab3[L + l] = make_double2(a_maj, b_maj);
    ab3[2 * L + l] = make_double2(a_dbl, b_dbl);
    double *o = ab6 + 8 * l;
    o[0] = a_min; o[1] = b_min; o[2] = a_maj; o[3] = b_maj; o[4] = a_dbl; o[5] = b_dbl; o[6] = 0.0; o[7] = 0.0;
}

__global__ __launch_bounds__(256) void k_posterior_finalize(uint64_t n_rows, const double *__restrict__ osum /*[3][2][n_rows] or null*/,
                                                            uint32_t groups, uint64_t npad,
                                                            const double *__restrict__ part /*[3][2][G][npad]*/,
                                                            double lp_min, double lp_maj, double lp_dbl,
                                                            double *__restrict__ post,
                                                            double *__restrict__ sdbl /*[n_rows] or null: option resolve_posteriors*/)
{
    const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n_rows) return;
    const uint64_t set_stride = 2ull * groups * npad;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (uint32_t g = 0; g < groups; g++) {
        s0 += part[(uint64_t)g * npad + row];
        s1 += part[set_stride + (uint64_t)g * npad + row];
        s2 += part[2 * set_stride + (uint64_t)g * npad + row];
    }
    if (osum) {
        s0 += osum[row];
        s1 += osum[2 * n_rows + row];
        s2 += osum[4 * n_rows + row];
    }
    const double s_min = s0, s_maj = s1, s_dbl = s2;
    const double log_num = lp_min + s_min;                       // main.rs:267
    double log_den = dm_logsumexp(log_num, lp_maj + s_maj);      // main.rs:268
    const double log_dbl = lp_dbl + s_dbl;                       // main.rs:270
    log_den = dm_logsumexp(log_den, log_dbl);                    // main.rs:271
    post[row] = exp(log_num - log_den);
    post[n_rows + row] = exp(log_dbl - log_den);
    post[2 * n_rows + row] = s_maj;
    post[3 * n_rows + row] = s_min;
    if (sdbl) sdbl[row] = s_dbl;
}

// ===========================================================================================================
// Launch geometry of a tile pass over nb cell blocks and `groups` chunk groups: sb cell blocks per column (several blocks
// amortise the table staging; with few blocks, i.e. a small shard, more columns are worth more: sb is halved while the columns
// x groups keep less than 90 % of the CUs busy; option tile_sb forces it), the columns, and a grid of persistent workgroups:
// one per CU, an equal number for every chunk group, never more than there are columns.
struct TileGeo {
    int sb;
    uint32_t n_cols;
    unsigned grid;
};
static TileGeo tile_geometry(const cellector_ctx *c, uint32_t nb, uint32_t groups)
{
    int sb = T_SB_MAX;
    while (sb > 2 && (uint64_t)((nb + sb - 1) / sb) * groups * 10 < (uint64_t)c->n_cu * 9) sb >>= 1;
    if (c->tile_sb_opt) sb = c->tile_sb_opt;
    const uint32_t n_cols = (nb + sb - 1) / sb;
    const uint32_t per_group = std::min(std::max((uint32_t)c->n_cu / groups, 1u), n_cols);
    return {sb, n_cols, per_group * groups};
}
// the tile kernel of geometry class G over one tile set.  t_a, t_b: a timer's events, which ride on the dispatch (no barrier
// packets around the kernel; regular tiles only)
template <class G>
static void launch_tile_ll(cellector_ctx *c, bool expected, const TileGeo &tg, uint32_t nj, uint32_t cpg, uint32_t groups, uint32_t *work,
                           const uint16_t *thdr, const uint16_t *tiles, const double *tab, double *part_ll, double *part_ell,
                           hipEvent_t t_a = nullptr, hipEvent_t t_b = nullptr)
{
    with_bool(expected, [&](auto E) {
        with_bool(tg.sb == 4, [&](auto WIDE) {
            constexpr int SB = WIDE.value ? 4 : 2;
            if constexpr (std::is_same<G, geo_reg>::value)
                if (t_a) {
                    hipExtLaunchKernelGGL((k_tile_ll<E.value, SB, G>), dim3(tg.grid), dim3(T_THREADS), 0, c->stream, t_a, t_b, 0, c->t_nb, nj, cpg,
                                          groups, tg.n_cols, work, thdr, tiles, tab, c->t_npad, part_ll, part_ell);
                    return;
                }
            hipLaunchKernelGGL((k_tile_ll<E.value, SB, G>), dim3(tg.grid), dim3(T_THREADS), 0, c->stream, c->t_nb, nj, cpg, groups, tg.n_cols,
                               work, thdr, tiles, tab, c->t_npad, part_ll, part_ell);
        });
    });
}

// one tier-2 tile pass on the main stream: this pass' chunked tables, then the tile kernel over the second tile set
template <class G>
static cellector_status t2_tiles_pass_g(cellector_ctx *c, const double2 *ab, int set, bool expected)
{
    constexpr uint32_t NE = G::NHI - G::NLO + 1;
    const unsigned gp = gcap(c->L * G::NCODE, 256, 0x7fffffffu), ge = expected ? gcap(c->L * NE, 256, 0x7fffffffu) : 0u;
    with_bool(expected, [&](auto E) {
        hipLaunchKernelGGL((k_t2c_tables<E.value, G>), dim3(gp + ge), dim3(256), 0, c->stream, c->L, gp, ab, (const double *)c->lf, c->tab2c);
    });
    double *part_ll = c->part2 + (uint64_t)set * 2 * c->t2_groups * c->t_npad;
    double *part_ell = part_ll + (uint64_t)c->t2_groups * c->t_npad;
    const TileGeo tg = tile_geometry(c, c->t_nb, c->t2_groups);
    HIPCHK(c, hipMemsetAsync(c->tile_work2, 0, T_GROUPS_MAX * sizeof(uint32_t), c->stream));
    launch_tile_ll<G>(c, expected, tg, c->t2_nj, c->t2_cpg, c->t2_groups, c->tile_work2, c->thdr2, c->tiles2, c->tab2c, part_ll, part_ell);
    HIPCHK(c, hipGetLastError());
    return CELLECTOR_OK;
}
static cellector_status t2_tiles_pass(cellector_ctx *c, const double2 *ab, int set, bool expected)
{
    if (!c->t2_tiles) return CELLECTOR_OK;
    return c->t2_tiles == 8 ? t2_tiles_pass_g<geo_t2<8>>(c, ab, set, expected) : t2_tiles_pass_g<geo_t2<6>>(c, ab, set, expected);
}
// ... and its partial sums added to the overflow sums of the set (behind the side stream's kernels, which write those)
static cellector_status t2_tiles_add(cellector_ctx *c, int set, bool expected)
{
    if (!c->t2_tiles) return CELLECTOR_OK;
    double *part_ll = c->part2 + (uint64_t)set * 2 * c->t2_groups * c->t_npad, *part_ell = part_ll + (uint64_t)c->t2_groups * c->t_npad;
    double *o_ll = c->ovf_sum + (uint64_t)set * 2 * c->nloc, *o_ell = o_ll + c->nloc;
    with_bool(expected, [&](auto E) {
        hipLaunchKernelGGL(k_t2_tile_add<E.value>, dim3(gcap(c->nloc, 256, 0x7fffffffu)), dim3(256), 0, c->stream, c->nloc, c->t2_groups, c->t_npad,
                           part_ll, part_ell, o_ll, o_ell);
    });
    HIPCHK(c, hipGetLastError());
    return CELLECTOR_OK;
}

// Overflow side of one pass: tables -> per-entry values (locus-major) -> per-cell sums.  Launched on the side stream so
// that these small, latency-bound kernels run next to the tile kernel instead of in front of it.
// cell side of the overflow entries of one pass, on stream `st`
static void launch_overflow_cell(cellector_ctx *c, hipStream_t st, const double2 *ab, int set, bool expected, bool em_pass = false,
                                 bool cache = false /*the EM pass of a ctx with the store of option t2_cache*/)
{
    double *o_ll = c->ovf_sum + (uint64_t)set * 2 * c->nloc, *o_ell = o_ll + c->nloc;
    const unsigned g = gcap(c->nloc, 256, 0x7fffffffu), eg = gcap(c->L * 16, 256, 0x7fffffffu);
    const bool deep = c->ovf_deep;  // the overflow share is large: full form, never throttled, no tier-0 list
    const uint64_t n0 = deep ? 0 : c->ovf_n_tier[0], n1 = c->ovf_n_tier[1];  // the listed entries this pass evaluates
    auto tables_e = [&] { hipLaunchKernelGGL(k_ovf_tables_e, dim3(eg), dim3(256), 0, st, c->L, ab, c->ovf_nmask, c->ovf_tab, c->ovf_etab); };
    with_bool(expected, [&](auto E) {
        constexpr bool EXP = E.value;
        if (c->t2 && !deep) {
            // tier 2: the pairs' table of this pass, then the rows' lookups (writes the sums); the other totals ADD to them
            const unsigned gp = gcap(c->t2_np, 256, 0x7fffffffu), gs = EXP ? gcap(c->t2_ns, 256, 0x7fffffffu) : 0u;
            // (side_lds > 0: a request for dynamic LDS the lookup kernel does not use, to limit its blocks per CU in A/B runs)
            const size_t lds_req = c->side_lds > 0 ? (size_t)c->side_lds : 0;
            const uint64_t n_grp = (c->nloc + 63) / 64;
            // Helper grid: the tile grid is a whole number of workgroups per chunk group and can leave CUs without one (245 of
            // 256 at 10^6 cells).  A tile workgroup holds nearly all of its CU's LDS, so blocks that ask for T2_HELP_LDS bytes
            // (unused) are placed on the free CUs only while the tile kernel runs, anywhere once it has ended.  They take groups
            // off the same counter as the co-resident grid above: work-conserving, and the same sums whoever looks a row up.
            // Automatic (t2_helper -1): T2_HELP_BLOCKS blocks per free CU beside the EM pass' tile kernel of a big shard (iteration
            // 1.838 -> 1.812 ms at 10^6 cells).  Not in the posterior phase, whose three lookup passes run ahead of their tile
            // kernels (4.8 -> 5.0 ms with it), and not on a small shard, whose tile kernel is too short to hide the two more
            // cross-stream waits (200k cells: 0.310 -> 0.328 ms).  t2_helper n > 0 forces n blocks per free CU, on one CU's worth
            // where none is free (tests).
            const unsigned tile_grid = tile_geometry(c, c->t_nb, c->t_groups).grid;
            const unsigned free_cu = (unsigned)c->n_cu > tile_grid ? (unsigned)c->n_cu - tile_grid : 0u;
            const unsigned hg = st != c->side || !c->t2_helper ? 0u
                                : c->t2_helper < 0             ? (em_pass && c->nloc >= (1ull << 19) ? free_cu * T2_HELP_BLOCKS : 0u)
                                                               : std::max(free_cu, 1u) * (unsigned)c->t2_helper;
            // waves of the co-resident grid: all groups at once when it has the machine to itself; beside the tile kernel option
            // t2_waves, 0 = 512, or 256 where a helper grid takes part of the groups
            const unsigned side_waves = c->t2_waves > 0 ? (unsigned)c->t2_waves : hg ? 256u : 512u;
            // (a caching pass launches the waves a filling pass wants; in the other passes the device sends the surplus home)
            const unsigned launch_waves = cache && c->t2_waves <= 0 ? std::max(side_waves, T2_FILL_WAVES) : side_waves;
            const unsigned cg = (unsigned)std::min<uint64_t>(n_grp ? n_grp : 1, st == c->side ? (uint64_t)launch_waves : 0x7fffffffull);
            uint32_t *ctr = c->t2_ctr + set;  // a counter per table set (the EM pass uses set 0, the posterior passes 0..2)
            // A caching pass (option t2_cache, see k_t2_cell): the tables kernel also forms the dirty mask and the two counts, into
            // the pair of counters of the pass' parity; the lookup grids read them.  Kept values of a pass without the expected
            // column have none: the next pass with it starts from an empty store (ab_t2 back to all-ones).
            t2_dirty_t dz = {};
            t2_cache_t cz = {};
            unsigned gd = 0;
            if (cache) {
                uint32_t *cnt = c->t2_ctr + 4 + 2 * (c->t2_pass & 1u), *other = c->t2_ctr + 4 + 2 * (~c->t2_pass & 1u);
                c->t2_pass++;
                if (EXP && !c->t2_val_exp) (void)hipMemsetAsync(c->ab_t2, 0xff, c->L * sizeof(double2), st);
                c->t2_val_exp = EXP;
                gd = gcap(c->L, 1024, 0x7fffffffu);  // (a wave per 256 loci)
                dz = t2_dirty_t{c->t2_dirty, gp + gs, (uint32_t)c->L, c->ab_t2, c->ab_last, cnt, other};
                cz = t2_cache_t{c->t2_val, c->t2_dirty, cnt, c->t2_fill, (uint32_t)(c->L * T2_FILL_PCT / 100), (uint32_t)c->L,
                                st == c->side ? side_waves : 0x7fffffffu, ab, c->ab_t2};
            }
            if (hg)  // the helper starts behind the tables: an event that rides on their dispatch (no barrier packet)
                hipExtLaunchKernelGGL(k_t2_tables<EXP>, dim3(gp + gs + gd), dim3(256), 0, st, nullptr, c->ev_t2tab, 0, (uint32_t)c->t2_np,
                                      (const uint32_t *)c->t2_plist, (uint32_t)c->t2_ns, (const uint32_t *)c->t2_slist, (uint32_t)gp, ab,
                                      (const double *)c->lf, (double *)c->tab2, ctr, dz);
            else
                hipLaunchKernelGGL(k_t2_tables<EXP>, dim3(gp + gs + gd), dim3(256), 0, st, c->t2_np, c->t2_plist, c->t2_ns, c->t2_slist, gp,
                                   ab, c->lf, c->tab2, ctr, dz);
            // (without a helper the grid strides over the groups as it always did: 15 000 one-wave blocks alone on the machine
            //  cost 0.18 ms of an overlap-0 iteration in atomics on the one counter)
            with_bool(cache, [&](auto CA) {
                if (hg)
                    hipLaunchKernelGGL((k_t2_cell<EXP, 1, 4, true, CA.value>), dim3(cg), dim3(64), lds_req, st, c->nloc, c->ovf_ell_ptr,
                                       c->ovf_ell, c->tab2, o_ll, o_ell, ctr, cz);
                else
                    hipLaunchKernelGGL((k_t2_cell<EXP, 1, 4, false, CA.value>), dim3(cg), dim3(64), lds_req, st, c->nloc, c->ovf_ell_ptr,
                                       c->ovf_ell, c->tab2, o_ll, o_ell, ctr, cz);
                if (hg) {
                    cz.calm = hg;  // (the helper grid is the same in every pass)
                    (void)hipStreamWaitEvent(c->side2, c->ev_t2tab, 0);
                    hipLaunchKernelGGL((k_t2_cell<EXP, 4, T2_HELP_U, true, CA.value>), dim3(hg), dim3(256), T2_HELP_LDS, c->side2, c->nloc,
                                       c->ovf_ell_ptr, c->ovf_ell, c->tab2, o_ll, o_ell, ctr, cz);
                    (void)hipEventRecord(c->ev_help, c->side2);
                }
            });
            if (EXP && n0) tables_e();  // E(9..17) of the tier-0 entries
            // the kernels below add to the sums the lookups store, and the next pass' tables overwrite what they read
            if (hg) (void)hipStreamWaitEvent(st, c->ev_help, 0);
        } else {
            if (EXP) tables_e();
            // Residency throttle (EM pass): a request for dynamic LDS it does not use leaves room for only ONE block of this kernel beside
            // a tile workgroup (one wave per SIMD instead of two).  On a big shard the kernel still ends well inside the tile
            // kernel and disturbs it less (cfg4: 2.83 -> 2.78 ms per iteration); a small shard's tile kernel is too short for that.
            const size_t lds_req =
                !EXP || deep ? 0 : c->side_lds >= 0 ? (size_t)c->side_lds : (st == c->side && c->nloc >= (1ull << 19) ? 5000 : 0);
            auto direct = [&](auto PACKED, auto FULL) {
                hipLaunchKernelGGL((k_ovf_cell_direct<EXP, PACKED.value, FULL.value>), dim3(g), dim3(256), lds_req, st, c->nloc, c->ovf_ell_ptr,
                                   c->ovf_ell, ab, c->lf, c->ovf_etab, c->ovf_tab, o_ll, o_ell);
            };
            if (deep && c->ovf_deep_wide)
                hipLaunchKernelGGL(k_ovf_cell_wide<EXP>, dim3(gcap(c->nloc * LF_LANES, 256, 0x7fffffffu)), dim3(256), 0, st, c->nloc,
                                   c->t2_tiles ? c->ovr_ptr : c->ovf_ptr, c->t2_tiles ? c->ovr_ent : c->ovf_ent, ab, c->lf, c->ovf_etab,
                                   c->ovf_tab, o_ll, o_ell);
            else if (deep) direct(std::false_type(), std::true_type());
            else if (!lds_req) direct(std::false_type(), std::false_type());
            else if constexpr (EXP) direct(std::true_type(), std::false_type());  // one block per CU: the 64-VGPR form, packed record
        }
        // the totals the kernels above leave out, as two short static lists: tier 0 (9..17) and tier 1 (above)
        if (n0)
            hipLaunchKernelGGL((k_ovf_cell_listed<EXP, false>), dim3(gcap(n0, 256, 0x7fffffffu)), dim3(256), 0, st, n0, c->ovf_tier_row[0],
                               c->ovf_tier_ent[0], ab, c->lf, c->ovf_tab, o_ll, o_ell);
        if (n1) {
            hipLaunchKernelGGL(k_ovf_listed_values<EXP>, dim3(gcap(n1, 256, 0x7fffffffu)), dim3(256), 0, st, n1, c->ovf_tier_ent[1], ab, c->lf,
                               c->ovf_tier_val, c->ovf_tier_val + n1);
            hipLaunchKernelGGL(k_ovf_listed_add<EXP>, dim3(gcap(n1, 256, 0x7fffffffu)), dim3(256), 0, st, n1, c->ovf_tier_row[1], c->ovf_tier_val,
                               c->ovf_tier_val + n1, o_ll, o_ell);
        }
    });
}
// locus side: the per-locus cumulative-log tables that k_locus_finalize evaluates the overflow entries' log-pmfs from, on stream `st`
static void launch_overflow_locus_values(cellector_ctx *c, hipStream_t st, const double2 *ab)
{
    if (c->t2 && !c->ovf_deep) {  // tier 2 needs nothing here (k_t2_tables is the cell side's first kernel); the few other entries:
        if (c->ovx_n)
            hipLaunchKernelGGL(k_ovx_values, dim3(gcap(c->ovx_n, 256, 0x7fffffffu)), dim3(256), 0, st, c->ovx_n, c->ovx_locus, c->ovx_ent, ab,
                               c->lf, c->ovx_lp);
        return;
    }
    if (c->t2)  // deep: the pairs' log-pmfs for the locus finalize's counts (the cell side does not use the table)
        hipLaunchKernelGGL(k_t2_tables<false>, dim3(gcap(c->t2_np, 256, 0x7fffffffu)), dim3(256), 0, st, c->t2_np, c->t2_plist, c->t2_ns,
                           c->t2_slist, gcap(c->t2_np, 256, 0x7fffffffu), ab, c->lf, c->tab2, (uint32_t *)nullptr, t2_dirty_t{});
    hipLaunchKernelGGL(k_ovf_tables, dim3(gcap(c->L * 3, 256, 0x7fffffffu)), dim3(256), 0, st, c->L, ab, c->ovf_nmask, c->ovf_tab);
    if (!c->ovf_deep)  // shallow coverage: the values are stored here, beside the tile kernel, and the finalize reads them
        hipLaunchKernelGGL(k_ovf_values, dim3(gcap(c->ovf_n, 256, 0x7fffffffu)), dim3(256), 0, st, c->ovf_n, c->ovc_locus, c->ovc_ent, ab,
                           c->lf, c->ovf_tab, c->ovf_lp);
}

static bool have_overflow(const cellector_ctx *c) { return c->ovf_n != 0 && c->L != 0 && c->nloc != 0; }

// fork: the side stream starts after everything already queued on the main stream (alpha/beta are ready there)
static cellector_status side_fork(cellector_ctx *c)
{
    if (c->tab_event_valid) {  // the table kernel is the last thing queued on the main stream and its completion has an event
        c->tab_event_valid = false;
        HIPCHK(c, hipStreamWaitEvent(c->side, c->ev_tab, 0));
        return CELLECTOR_OK;
    }
    HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->side, c->ev_fork, 0));
    return CELLECTOR_OK;
}
// join: the main stream continues after everything queued on the side stream
static cellector_status side_join(cellector_ctx *c)
{
    HIPCHK(c, hipEventRecord(c->ev_join, c->side));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
    return CELLECTOR_OK;
}

// the chunk tables of one pass
static cellector_status build_tile_tables(cellector_ctx *c, const double2 *ab, int set, bool expected, bool form_ab = false,
                                          const uint8_t *mask = nullptr, hipEvent_t done = nullptr /*rides on the dispatch*/)
{
    const uint64_t tab_elems = (uint64_t)c->t_nj * TAB_ELEMS;
    double *tab = expected ? c->tab + 3 * tab_elems : c->tab + (uint64_t)set * tab_elems;
    const unsigned tgrid = gcap((uint64_t)c->t_nj * T_BL, 64);
    ab_src_t src = {};
    if (form_ab) {  // first kernel of an EM iteration: alpha/beta from the exchanged tallies, counters reset
        const uint64_t L = c->L;
        src.s_alt = c->s_alt; src.s_ref = c->s_ref;
        src.alt_min = c->x_locus + LB_ALT_MIN * L; src.ref_min = c->x_locus + LB_REF_MIN * L;
        src.mask = mask ? mask : c->mask; src.ab_out = c->ab;
        src.xl_counters = c->x_locus + (uint64_t)LB_PLANES * L; src.d_counters = c->d_counters;
        src.tile_work = c->tile_work; src.n_work = 3u * T_GROUPS_MAX;
        c->work_zeroed = true;
    }
    with_bool(expected, [&](auto E) {
        if (done)  // (an event RECORDED behind the kernel is a barrier packet of its own: ~6 us of idle queue in front of the next kernel)
            hipExtLaunchKernelGGL(k_build_tables<E.value>, dim3(tgrid), dim3(64 * TB_PARTS), 0, c->stream, nullptr, done, 0, c->L, c->t_nj, ab,
                                  (const double *)c->lf, tab, src);
        else
            hipLaunchKernelGGL(k_build_tables<E.value>, dim3(tgrid), dim3(64 * TB_PARTS), 0, c->stream, c->L, c->t_nj, ab, c->lf, tab, src);
    });
    c->tab_event_valid = done != nullptr;
    if (set == 0) {  // the locus pass of this iteration reads the log-pmfs of the EM pass' table
        c->tab_em = tab;
        c->tab_em_stride = expected ? 2 : 1;
    }
    HIPCHK(c, hipGetLastError());
    return CELLECTOR_OK;
}

// tile kernel of one pass on the main stream (its tables are built)
static cellector_status run_tile_pass(cellector_ctx *c, int set, bool expected)
{
    const uint64_t tab_elems = (uint64_t)c->t_nj * TAB_ELEMS;
    double *tab = expected ? c->tab + 3 * tab_elems : c->tab + (uint64_t)set * tab_elems;
    double *part_ll = c->part + (uint64_t)set * 2 * c->t_groups * c->t_npad;
    double *part_ell = part_ll + (uint64_t)c->t_groups * c->t_npad;
    const TileGeo tg = tile_geometry(c, c->t_nb, c->t_groups);
    uint32_t *work = c->tile_work + (size_t)set * T_GROUPS_MAX;
    if (!(set == 0 && c->work_zeroed))  // else: reset by this iteration's k_alpha_beta
        HIPCHK(c, hipMemsetAsync(work, 0, T_GROUPS_MAX * sizeof(uint32_t), c->stream));
    hipEvent_t t_a = nullptr, t_b = nullptr;
    timer_take(c, CELLECTOR_K_TILE_LL, &t_a, &t_b);  // (both stay null when the launch is not timed)
    launch_tile_ll<geo_reg>(c, expected, tg, c->t_nj, c->t_cpg, c->t_groups, work, c->thdr, c->tiles, tab, part_ll, part_ell, t_a, t_b);
    HIPCHK(c, hipGetLastError());
    return CELLECTOR_OK;
}

// first half of the cell pass: tables, the tile kernel and the overflow kernels beside it (results in scratch arrays)
static cellector_status cell_pass_launch(cellector_ctx *c, const double2 *ab, bool for_em)
{
    timer_begin(c, CELLECTOR_K_CELL_LL);
    const bool ovf = have_overflow(c);
    // The overflow entries' cell side runs on the side stream BESIDE the tile kernel: in the few wave slots the persistent
    // tile workgroups leave it is several times slower than alone, but it ends well inside the tile kernel's time.  In an
    // EM iteration the locus side's values follow on the side stream once the tile kernel is done; the locus finalize
    // waits for them (tiled_locus_pass).  (overlap 0: everything in the main stream.)
    if (for_em && c->tables_prebuilt) c->tables_prebuilt = false;  // built ahead by the previous iteration's em_finish
    else CHK(build_tile_tables(c, ab, 0, c->compute_expected, for_em));
    // (deep coverage, ovf_deep: the same arrangement with the unthrottled 16-lanes-per-row kernel — it fills the tile kernel's
    //  idle issue slots while that runs and has the machine to itself afterwards: 7.8 ms per iteration at 1M x 200k deep
    //  against 8.3 with the two one after the other)
    // the EM pass' tier-2 lookups keep their values (option t2_cache); a ctx built with the option off gets its store here
    const bool cache = for_em && ovf && c->t2 && !c->ovf_deep && t2_cache_on(c);
    if (cache && !c->t2_val) CHK(t2_cache_alloc(c));
    if (ovf && c->overlap) {
        // the tile kernel is launched FIRST: with the tables built ahead the queue is empty when the host gets here, and
        // every launch ahead of it (five on the side stream) would be ~10 us of idle GPU
        CHK(side_fork(c));
        CHK(run_tile_pass(c, 0, c->compute_expected));
        CHK(t2_tiles_pass(c, ab, 0, c->compute_expected));
        launch_overflow_cell(c, c->side, ab, 0, c->compute_expected, for_em, cache);
        HIPCHK(c, hipEventRecord(c->ev_join, c->side));
        if (for_em && c->overlap == 1) {  // the locus side's values right behind the cell side, beside the tile kernel
            launch_overflow_locus_values(c, c->side, ab);  // (they may end after it: only the locus finalize waits for them)
            HIPCHK(c, hipEventRecord(c->ev_join2, c->side));
            c->ovf_locus_pending = true;
        }
        if (for_em && c->overlap == 2) {  // ... or once the tile kernel is done, beside the order statistics
            HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
            HIPCHK(c, hipStreamWaitEvent(c->side, c->ev_fork, 0));
            launch_overflow_locus_values(c, c->side, ab);
            HIPCHK(c, hipEventRecord(c->ev_join2, c->side));
            c->ovf_locus_pending = true;
        }
        c->cell_join_pending = true;
    } else {
        if (ovf) {
            launch_overflow_cell(c, c->stream, ab, 0, c->compute_expected, for_em, cache);
            if (for_em) launch_overflow_locus_values(c, c->stream, ab);
        }
        CHK(run_tile_pass(c, 0, c->compute_expected));
        CHK(t2_tiles_pass(c, ab, 0, c->compute_expected));
    }
    return CELLECTOR_OK;
}

cellector_status tiled_cell_pass(cellector_ctx *c, const double2 *ab, double *norm_out, bool for_em, const uint32_t *masked_cnt)
{
    if (c->nloc == 0) return CELLECTOR_OK;
    const bool ovf = have_overflow(c);
    // (Measured and dropped: em_finish queueing this first half for the NEXT iteration right behind its table kernel, so that the
    //  tile kernel starts without waiting for the host to read the summary and launch — no gain at 10^6 cells, none on a 125k-cell
    //  shard: 0.50 vs 0.49 ms.  The ~15 us between the table kernel and the tile kernel are not the host's.)
    CHK(cell_pass_launch(c, ab, for_em));
    if (c->cell_join_pending) {  // the overflow entries' cell-side sums (side stream)
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
        c->cell_join_pending = false;
    }
    CHK(t2_tiles_add(c, 0, c->compute_expected));
    double *part_ll = c->part, *part_ell = c->part + (uint64_t)c->t_groups * c->t_npad;
    const double *o_ll = ovf ? c->ovf_sum : nullptr, *o_ell = ovf ? c->ovf_sum + c->nloc : nullptr;
    const unsigned grid = gcap((c->nloc + 1) / 2, 256, 0x7fffffffu);
    with_bool(c->compute_expected, [&](auto E) {
        hipLaunchKernelGGL(k_cell_finalize<E.value>, dim3(grid), dim3(256), 0, c->stream, c->nloc, c->t_groups, c->t_npad, part_ll,
                           part_ell, o_ll, o_ell, c->csr_ptr, masked_cnt ? masked_cnt : c->masked_cnt.get(), c->ll, c->ell, c->nloci, norm_out);
    });
    timer_end(c, CELLECTOR_K_CELL_LL);
    HIPCHK(c, hipGetLastError());
    return CELLECTOR_OK;
}

cellector_status tiled_locus_pass(cellector_ctx *c)
{
    if (c->L == 0) return CELLECTOR_OK;
    timer_begin(c, CELLECTOR_K_LOCUS_STATS);
    // (k_locus_finalize's loop over the overflow entries, a third of its time at 10^6 cells, was tried as a kernel of its
    //  own on the side stream beside k_minority_ranges: both stream scattered lines, the pair took as long as one after
    //  the other)
    const uint32_t words = (uint32_t)((c->nloc + 31) / 32);
    // kept counts (tally, cnt2) of the old exclusion set: this iteration updates them from the change (k_flag's chg) on the device
    // (tally_plan); else the next kernels recount.  Until em_finish swaps the flags they belong to neither set.
    const int valid = c->tally_delta && c->tally_valid ? 1 : 0;
    c->tally_valid = false;
    if (!valid && c->t2) HIPCHK(c, hipMemsetAsync(c->cnt2, 0, c->L * T2_CSTRIDE * sizeof(uint32_t), c->stream));
    // (k_flag wrote the exclusion bitmask flag_bits along with the flags)
    const size_t lds = (size_t)words * 4;
    unsigned grid = (unsigned)c->n_cu;
    const uint64_t need = (c->L + LS_THREADS / 64 - 1) / (LS_THREADS / 64);
    if (grid > need) grid = (unsigned)(need ? need : 1);
#define LAUNCH_LS(INLDS, EBV, GRID, LDSB)                                                                              \
    hipLaunchKernelGGL((k_locus_stats2<INLDS, EBV>), dim3(GRID), dim3(LS_THREADS), LDSB, c->stream, c->L, words, c->c4_ptr, \
                       c->c4_ent, c->flag_bits, c->tally, c->locus_mode, valid, c->nloc, c->d_counters + DC_N_MIN, c->lr_sub, c->lr_cap)
    // (a forced minority-driven form, locus_mode 2, still launches the streamed kernel: it returns at once unless the
    //  exclusion set is too large for that form's 16-bit counters, the one case the device predicate overrides the option;
    //  likewise locus_mode 1 launches the minority-driven kernels while counts are kept: they walk the change)
    if (lds <= 128 * 1024) {
        if (c->c4_bits == 24) {
            // the whole 2^20-cell bitmask: a padding entry (cell = all ones) then reads inside the allocation
            const int lb = 128 * 1024;
            HIPCHK(c, hipFuncSetAttribute((const void *)k_locus_stats2<true, 24>, hipFuncAttributeMaxDynamicSharedMemorySize, lb));
            LAUNCH_LS(true, 24, grid, lb);
        } else {
            const int lb = (int)(lds ? lds : 4);
            HIPCHK(c, hipFuncSetAttribute((const void *)k_locus_stats2<true, 32>, hipFuncAttributeMaxDynamicSharedMemorySize, lb));
            LAUNCH_LS(true, 32, grid, lb);
        }
    } else {
        LAUNCH_LS(false, 32, grid * 2, 4);  // more than 2^20 cells per shard: 32-bit entries, bitmask read from L2
    }
#undef LAUNCH_LS
    // capacity of the transposed offsets: the largest exclusion set the automatic choice hands to this form, also the largest
    // change tally_plan walks; the forced form (tests, ablations) may need all cells
    const uint64_t want = c->locus_mode == 2 ? c->nloc : (c->locus_mode == 0 || c->tally_delta) ? c->nloc * LM_NUM / LM_DEN + LT_CELLS : 0;
    if (want && c->nloc) {
        const uint32_t R = (uint32_t)((c->L + LR_LOCI - 1) / LR_LOCI);
        if (c->mroff_cap < want) {
            HIPCHK(c, hipStreamSynchronize(c->stream));
            c->mroff.reset(); c->mbeg.reset();
            c->mroff_cap = (want + 63) & ~63ull;
            CHK(dev_alloc(c, &c->mroff, (uint64_t)(R + 1) * c->mroff_cap));
            CHK(dev_alloc(c, &c->mbeg, c->mroff_cap));
        }
        const size_t lds_t = (size_t)LT_CELLS * (R + 2) * sizeof(uint32_t);
        if (lds_t > 64 * 1024)
            HIPCHK(c, hipFuncSetAttribute((const void *)k_minority_offsets, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_t));
        hipLaunchKernelGGL(k_minority_offsets, dim3(gcap(want, LT_CELLS, 0x7fffffffu)), dim3(256), lds_t, c->stream, c->locus_mode,
                           valid, c->nloc, c->lr_sub, c->lr_cap, R, c->mroff_cap, c->d_counters + DC_N_MIN, c->minlist, c->chg, c->csr_ptr, c->roff,
                           c->mroff, c->mbeg);
        // (R x lr_sub workgroups per sign: a change that both adds and rescues cells fills twice the planes of a recount)
        hipLaunchKernelGGL(k_minority_ranges, dim3(R * c->lr_sub * 2), dim3(LR_THREADS), 0, c->stream, c->locus_mode, valid, c->nloc,
                           c->L, R, c->lr_sub, c->lr_cap, c->mroff_cap, c->d_counters + DC_N_MIN, c->mroff, c->mbeg, c->c4r, c->hist_min);
    }
    // the tier-2 entries per (locus, pair) of the changed cells, or of the whole new set.  (On the side stream it does NOT run
    // beside k_minority_ranges, whose sixteen 128-register waves per CU leave no room: it started when that kernel ended, two
    // event gaps later.)
    if (c->t2 && c->nloc)
        hipLaunchKernelGGL(k_t2_minority, dim3(gcap(c->nloc / LM_DEN + 1, 256 / LF_LANES, 8192)), dim3(256), 0, c->stream, c->d_counters + DC_N_MIN,
                           valid, c->nloc, c->minlist, c->chg, c->ovf_ptr, c->ovf_ent, c->cnt2);
    if (c->ovf_locus_pending) {  // the overflow entries' log-pmfs of this iteration (side stream)
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_join2, 0));
        c->ovf_locus_pending = false;
    }
    // the entries the finalize walks one by one: all overflow entries, or (tier 2) those outside tier 2
    const uint64_t *w_ptr = c->t2 ? (c->ovx_n ? c->ovx_ptr : nullptr) : (c->ovf_n ? c->ovc_ptr : nullptr);
    const uint64_t *w_ent = c->t2 ? c->ovx_ent : c->ovc_ent;
    const double *w_lp = c->t2 ? c->ovx_lp : c->ovf_lp;
    // (a ctx that holds all cells and has no communicator: nothing is exchanged between the finalize and the filter)
    c->filter_fused = !comm_active(c->comm) && c->nloc == c->total_cells && c->fuse_filter;
    with_bool(c->ovf_deep, [&](auto INL) {
        hipLaunchKernelGGL(k_locus_finalize<INL.value>, dim3(gcap(c->L * LF_LANES, 256, 0x7fffffffu)), dim3(256), 0, c->stream, c->L,
                           c->locus_mode, valid, c->nloc, c->lr_sub, c->lr_cap, c->d_counters + DC_N_MIN, c->hist_min, c->tally, c->flag_bits,
                           c->hist_all, c->tab_em, (uint32_t)c->tab_em_stride, c->mask, w_ptr, w_ent, w_lp, c->ovf_tab, c->lf, c->ab,
                           c->x_locus, c->t2 ? c->cnt2 : (uint32_t *)nullptr, c->hist_all2, c->t2_pmask, c->tab2,
                           c->filter_fused ? c->mask_next : (uint8_t *)nullptr, c->d_counters);
    });
    timer_end(c, CELLECTOR_K_LOCUS_STATS);
    HIPCHK(c, hipGetLastError());
    return CELLECTOR_OK;
}

// The NEXT iteration's first kernel (alpha/beta + tables + counter reset), queued by em_finish behind the locus filter and
// the summary kernel, i.e. before the host waits for the summary: it then runs while the host wakes up and decides.  It
// reads what the next em_begin would read: the exchanged tallies and the filtered mask (mask_next, about to become mask).
cellector_status tiled_prebuild_tables(cellector_ctx *c)
{
    if (c->nloc == 0 || c->L == 0) return CELLECTOR_OK;
    CHK(build_tile_tables(c, c->ab, 0, c->compute_expected, true, c->mask_next, c->ev_tab));
    c->tables_prebuilt = true;
    c->prebuilt_expected = c->compute_expected;
    return CELLECTOR_OK;
}

// target += the entries of the loci that mask_old has and mask_new has not
static cellector_status launch_masked_update(cellector_ctx *c, const uint8_t *mask_old, const uint8_t *mask_new, uint32_t *target)
{
    with_bool(c->c4_bits == 24, [&](auto NARROW) {
        hipLaunchKernelGGL(k_masked_update<NARROW.value ? 24 : 32>, dim3(gcap(c->L, 4)), dim3(256), 0, c->stream, c->L, mask_old, mask_new,
                           c->c4_ptr, c->c4_ent, c->ovc_ptr, c->ovc_ent, target);
    });
    HIPCHK(c, hipGetLastError());
    return CELLECTOR_OK;
}

// called after the locus filter with mask = this iteration's mask, mask_next = filtered mask
cellector_status tiled_masked_update(cellector_ctx *c)
{
    if (c->L == 0) return CELLECTOR_OK;
    return launch_masked_update(c, c->mask, c->mask_next, c->masked_cnt);
}

// a caller's mask (cellector_set_loci_mask): the counts from scratch — zeroed, then one update from an all-ones "old" mask to c->mask
cellector_status tiled_masked_recount(cellector_ctx *c, uint8_t *ones)
{
    HIPCHK(c, hipMemsetAsync(c->masked_cnt, 0, (c->nloc ? c->nloc : 1) * 4, c->stream));
    if (c->L == 0 || c->nloc == 0) return CELLECTOR_OK;
    HIPCHK(c, hipMemsetAsync(ones, 1, c->L, c->stream));
    return launch_masked_update(c, ones, c->mask, c->masked_cnt);
}

// the counts under the mask of ONE call (cellector_cell_log_likelihoods): cnt [nloc] is the caller's scratch, host_mask [L] or
// null = all used.  The ctx's own masked_cnt, mask and n_masked_loci are not touched.  Complete on return.
cellector_status tiled_call_masked_count(cellector_ctx *c, const uint8_t *host_mask, uint32_t *cnt)
{
    HIPCHK(c, hipMemsetAsync(cnt, 0, (c->nloc ? c->nloc : 1) * 4, c->stream));
    if (!host_mask || c->L == 0 || c->nloc == 0) return CELLECTOR_OK;
    DevBuf<uint8_t> ones, m;
    CHK(dev_alloc(c, &ones, c->L));
    CHK(dev_alloc(c, &m, c->L));
    HIPCHK(c, hipMemsetAsync(ones, 1, c->L, c->stream));
    HIPCHK(c, hipMemcpyAsync(m, host_mask, c->L, hipMemcpyHostToDevice, c->stream));
    CHK(launch_masked_update(c, ones, m, cnt));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (the two scratch masks go)
    return CELLECTOR_OK;
}

cellector_status tiled_posteriors(cellector_ctx *c, double mf0, double lp_min, double lp_maj, double lp_dbl, double *sdbl)
{
    c->tables_prebuilt = false;  // the posterior passes rebuild table set 0 and use its column counters
    if (c->cell_join_pending) {
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
        c->cell_join_pending = false;
    }
    c->work_zeroed = false;
    const uint64_t L = c->L;
    if (L)
        hipLaunchKernelGGL(k_ab_posterior3, dim3(gcap(L, 256)), dim3(256), 0, c->stream, L, c->s_alt, c->s_ref,
                           c->x_locus + LB_ALT_MIN * L, c->x_locus + LB_REF_MIN * L, mf0, c->ab3, c->ab6);
    HIPCHK(c, hipGetLastError());
    if (c->nloc == 0) return CELLECTOR_OK;
    timer_begin(c, CELLECTOR_K_POSTERIOR);
    const bool ovf = have_overflow(c);
    for (int set = 0; set < 3; set++) CHK(build_tile_tables(c, c->ab3 + (uint64_t)set * L, set, false));
    if (ovf && c->overlap) {
        CHK(side_fork(c));
        for (int set = 0; set < 3; set++) launch_overflow_cell(c, c->side, c->ab3 + (uint64_t)set * L, set, false);
        for (int set = 0; set < 3; set++) CHK(run_tile_pass(c, set, false));
        for (int set = 0; set < 3; set++) CHK(t2_tiles_pass(c, c->ab3 + (uint64_t)set * L, set, false));
        CHK(side_join(c));
    } else {
        if (ovf)
            for (int set = 0; set < 3; set++) launch_overflow_cell(c, c->stream, c->ab3 + (uint64_t)set * L, set, false);
        for (int set = 0; set < 3; set++) CHK(run_tile_pass(c, set, false));
        for (int set = 0; set < 3; set++) CHK(t2_tiles_pass(c, c->ab3 + (uint64_t)set * L, set, false));
    }
    for (int set = 0; set < 3; set++) CHK(t2_tiles_add(c, set, false));
    hipLaunchKernelGGL(k_posterior_finalize, dim3(gcap(c->nloc, 256, 0x7fffffffu)), dim3(256), 0, c->stream, c->nloc,
                       ovf ? c->ovf_sum : (const double *)nullptr, c->t_groups, c->t_npad, c->part, lp_min, lp_maj, lp_dbl, c->post, sdbl);
    timer_end(c, CELLECTOR_K_POSTERIOR);
    HIPCHK(c, hipGetLastError());
    return CELLECTOR_OK;
}
