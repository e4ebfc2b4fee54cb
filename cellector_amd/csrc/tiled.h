// Engine v2, shared by its two halves: kernels_tiled.hip (the passes an iteration runs) and kernels_tiled_build.hip (what
// tiled_build makes once per ingest).  Constants, entry encodings and the host-side launch helpers.  Internal.
#pragma once
#include <algorithm>
#include <initializer_list>
#include <type_traits>

#include "ctx.h"
#include "device_math.h"

#define T_K 4           // entries with 1 <= alt+ref <= T_K are "regular": log-pmf and expected term come from tables
#define T_NCODE 14      // (alt, ref) combinations with 1 <= n <= T_K: K(K+3)/2
#ifndef T_LROW
#define T_LROW 18       // table doubles per locus: the T_NCODE log-pmfs, then the T_K expected terms
#endif
#ifndef T_BL
#define T_BL 640        // locus slots per chunk (the table is T_BL * T_LROW * 8 B = 90 KB of LDS); the last slot is all zeros
#endif
#define T_BLU (T_BL - 1)  // loci per chunk
#define T_BC 1024       // cells per block == threads per workgroup
#define T_THREADS 1024
static_assert(T_BC == T_ROWS_PER_TILE, "cellector_engine_info derives the lookup count from this");
#define T_SB_MAX 4      // cell blocks per workgroup sharing one staged table (2 or 4: chosen per launch)
#define T_GROUPS_MAX 64 // upper bound of the chunk groups of a launch
static_assert(T_GROUPS_MAX == CELLECTOR_TILE_WORK_STRIDE, "k_alpha_beta resets the counters with this stride");
#define T_GROUPS 8      // chunk groups beyond this many are charged for their partial sums (tiled_build's cost model)
#define T_ROW_U16 16    // u16 of a row held in registers (two 16-byte loads): 15 entries behind the cell id (K odd) or 16 (K even);
                        // longer rows: slow path
// A u16 entry names a locus slot of the chunk and a code; its bits, and where its log-pmf and its expected term sit in the chunk's
// table, are the geometry's business (tile_entry / tile_entry_pmf / tile_entry_exp and tab_pmf / tab_exp below).  T_NULL, the
// padding entry (code 0 of the chunk's all-zero slot: both lookups read 0.0), is defined behind them.
// A slice in `tiles` is 64 x (K + 1) u16, K = the entries of its longest row, at least 1 (every geometry: a slice without any
// entry keeps one padding entry per row, 256 bytes, and the kernels need no form for an empty row; the tier-2 kernels skip it by
// the header's flag).  Rows must start on a dword for the 16-byte loads, so the format follows from K's parity:
//   K odd   64 rows of K + 1 u16: row i = [cell (0..1023) that lane i works for, K entries of that cell];
//   K even  the 64 cell ids first (u16 i = lane i's cell), then 64 rows of K u16: the entries alone.
// Rows are padded with T_NULL to K entries.  Either way a slice is 128 (K + 1) bytes, starts on a 128-byte boundary, and dword
// p >= 1 of a row holds two consecutive entries; dword 0 holds the cell id and entry 0 (odd) or entries 0 and 1 (even).
// Tile header (fixed stride, in u16 units): 16 slices x {u64 first u16 of the slice in `tiles`, u32 K, u32 1 = the slice has no
// entry at all}.
#define T_HDR 128
// u16 inside a slice: of row r's cell id, of its first entry; u16 of a row
__host__ __device__ __forceinline__ constexpr uint32_t slice_cell_at(uint32_t K, uint32_t r) { return (K & 1u) ? r * (K + 1u) : r; }
__host__ __device__ __forceinline__ constexpr uint32_t slice_row_at(uint32_t K, uint32_t r) { return (K & 1u) ? r * (K + 1u) + 1u : 64u + r * K; }
__host__ __device__ __forceinline__ constexpr uint32_t slice_k(uint32_t longest) { return longest ? longest : 1u; }
#define TAB_ELEMS ((uint64_t)T_LROW * T_BL)  // table doubles per chunk

__device__ __forceinline__ bool ent_regular(uint64_t e)
{
    const uint32_t n = ENT_ALT(e) + ENT_REF(e);
    return n >= 1u && n <= (uint32_t)T_K;
}
__device__ __forceinline__ uint32_t ent_code(uint64_t e)
{
    const uint32_t r = ENT_REF(e), n = ENT_ALT(e) + r;
    return n * (n + 1u) / 2u - 1u + r;
}

#define TB_PARTS 6  // waves of a k_build_tables workgroup: each takes its share of a locus' 18 values

// Table / entry geometry of a tile set.  geo_reg: the regular entries (totals 1..T_K): 18 doubles per locus, u16 entry =
// E << 4 | c (offset entries, below; TILE_OE 0: n-1 << 14 | slot << 4 | code).  geo_t2<NMAX>: the tier-2 tiles of a deep-coverage
// matrix (totals 5..NMAX, tiled_build):
// NMAX = 8: 30 log-pmfs + 4 expected terms per locus, 338 loci per chunk, entry = n-5 << 14 | slot << 5 | pair;
// NMAX = 6: 13 + 2 doubles per locus, 767 loci per chunk, entry = n-5 << 14 | slot << 4 | pair.
// The image of a chunk's table (in global memory and, copied as it is, in LDS) is a property of the geometry:
//   locus-major  [slot][LROW]: a locus' log-pmfs, then its expected terms;
//   code-major   [LROW planes][BL]: the expected-term planes first, the log-pmf planes after them, plane p at p * BL + slot.  A
//                lookup's bank pair is then slot mod 32 whatever the code (locus-major at an even LROW: the expected term of an
//                n = 1 entry, 70 % of them, only ever reaches the even bank pairs), and the plane's byte offset is code x (BL x 8)
//                added onto slot x 8 by one multiply-add — the constant part of both lookups (0 and NE planes) fits the 16-bit
//                offset field of a DS instruction.
#ifndef TILE_CM
#define TILE_CM 1  // regular geometry: 1 = code-major table image, 0 = locus-major (the measurement's other arm)
#endif
// Offset entries (a code-major image whose expected-term planes fit 12 bits of element index): the entry carries where its two
// values sit instead of naming slot, code and total, so that the tile kernel does not work that out again for every entry of every
// pass —
//   entry = E << 4 | c,   E = tab_exp(slot, n - NLO): the expected term's element (its plane is among the first LROW - NCODE),
//                         c = the log-pmf's plane - the expected term's plane = LROW - NCODE + code - (n - NLO): 4..14,
//   log-pmf element = E + c * BL (= tab_pmf(slot, code)); the total is E / BL + NLO, the slot E % BL, the code follows from c.
// Two address instructions per value (shift + mask; field extract + multiply-add) where slot << 4 | code takes two for the slot and
// two for each value.  The total's own field of the plain encoding is redundant with the code, which is where the bits come from.
#ifndef TILE_OE
#define TILE_OE 1  // regular geometry, code-major image: 1 = offset entries, 0 = n-1 << 14 | slot << 4 | code (the measurement's other arm)
#endif
struct geo_reg {
    static constexpr uint32_t LROW = T_LROW, BL = T_BL, NCODE = T_NCODE, SHIFT = 4, SMASK = 1023u, CMASK = 15u;
    static constexpr uint32_t BLU = BL - 1, NLO = 1, NHI = T_K;  // loci per chunk (the last slot is all zeros); totals covered
    static constexpr bool CODE_MAJOR = TILE_CM != 0;
    static constexpr bool OFFSET_ENTRIES = CODE_MAJOR && TILE_OE != 0;
};
template <int NMAX>
struct geo_t2 {
    static_assert(NMAX == 6 || NMAX == 8, "tier-2 tile geometries");
    static constexpr uint32_t NCODE = NMAX == 8 ? 30 : 13, NE = NMAX - 4, LROW = NCODE + NE;
    static constexpr uint32_t BL = NMAX == 8 ? 339 : 768, SHIFT = NMAX == 8 ? 5 : 4, SMASK = NMAX == 8 ? 511u : 1023u,
                              CMASK = NMAX == 8 ? 31u : 15u;
    static constexpr uint32_t BLU = BL - 1, NLO = 5, NHI = NMAX;
    static constexpr bool CODE_MAJOR = false, OFFSET_ENTRIES = false;  // (their fields do not fit 16 bits as offsets)
};
// THE index function of a chunk's table: element of the log-pmf of `code` resp. of the expected term number `ne` (= n - G::NLO)
// of locus slot `slot`.  Everything that writes or reads a chunk table goes through these two.
template <class G>
__host__ __device__ __forceinline__ constexpr uint32_t tab_pmf(uint32_t slot, uint32_t code)
{
    return G::CODE_MAJOR ? (G::LROW - G::NCODE + code) * G::BL + slot : slot * G::LROW + code;
}
template <class G>
__host__ __device__ __forceinline__ constexpr uint32_t tab_exp(uint32_t slot, uint32_t ne)
{
    return G::CODE_MAJOR ? ne * G::BL + slot : slot * G::LROW + G::NCODE + ne;
}
// THE bit layout of a u16 tile entry: made from (slot, code), taken apart again, and turned into the elements of its two table
// values.  The builders, the bank model and the tile kernel go through these and know no bits themselves.
// total - NLO of a code (codes are numbered total by total, n + 1 of them for the total n: ent_code / t2_code)
template <class G>
__host__ __device__ __forceinline__ constexpr uint32_t tile_code_ne(uint32_t code)
{
    uint32_t ne = 0;
    for (uint32_t n = G::NLO, first = n + 1u; n < G::NHI && code >= first; n++, first += n + 1u) ne++;
    return ne;
}
template <class G>
__host__ __device__ __forceinline__ constexpr uint16_t tile_entry(uint32_t slot, uint32_t code)
{
    const uint32_t ne = tile_code_ne<G>(code);
    if constexpr (G::OFFSET_ENTRIES) return (uint16_t)((tab_exp<G>(slot, ne) << 4) | (G::LROW - G::NCODE + code - ne));
    else return (uint16_t)((ne << 14) | (slot << G::SHIFT) | code);
}
template <class G>
__host__ __device__ __forceinline__ constexpr uint32_t tile_entry_ne(uint32_t e)  // total - NLO
{
    if constexpr (G::OFFSET_ENTRIES) return (e >> 4) / G::BL;
    else return e >> 14;
}
template <class G>
__host__ __device__ __forceinline__ constexpr uint32_t tile_entry_slot(uint32_t e)
{
    if constexpr (G::OFFSET_ENTRIES) return (e >> 4) % G::BL;
    else return (e >> G::SHIFT) & G::SMASK;
}
template <class G>
__host__ __device__ __forceinline__ constexpr uint32_t tile_entry_code(uint32_t e)
{
    if constexpr (G::OFFSET_ENTRIES) return (e & 15u) + tile_entry_ne<G>(e) - (G::LROW - G::NCODE);
    else return e & G::CMASK;
}
// elements of the entry's log-pmf and of its expected term in the chunk's table (e: the 16 bits, zero-extended)
template <class G>
__host__ __device__ __forceinline__ constexpr uint32_t tile_entry_pmf(uint32_t e)
{
    if constexpr (G::OFFSET_ENTRIES) return (e >> 4) + (e & 15u) * G::BL;
    else return tab_pmf<G>(tile_entry_slot<G>(e), tile_entry_code<G>(e));
}
template <class G>
__host__ __device__ __forceinline__ constexpr uint32_t tile_entry_exp(uint32_t e)
{
    if constexpr (G::OFFSET_ENTRIES) return e >> 4;
    else return tab_exp<G>(tile_entry_slot<G>(e), tile_entry_ne<G>(e));
}
// padding entry of a geometry: code 0 of the chunk's all-zero slot
template <class G>
__host__ __device__ __forceinline__ constexpr uint16_t tile_entry_null() { return tile_entry<G>(G::BLU, 0u); }
#define T_NULL (tile_entry_null<geo_reg>())
// Every (slot, code) of a geometry makes an entry that gives slot, code and total back and whose two elements are tab_pmf / tab_exp
// of them, inside the chunk's image: a build that passes this cannot address outside the table.
template <class G>
constexpr bool tile_entries_round_trip()
{
    for (uint32_t slot = 0; slot < G::BL; slot++)
        for (uint32_t code = 0; code < G::NCODE; code++) {
            const uint32_t ne = tile_code_ne<G>(code), e = tile_entry<G>(slot, code);
            const uint32_t pmf = tile_entry_pmf<G>(e), exp = tile_entry_exp<G>(e);
            if (ne > G::NHI - G::NLO) return false;
            if (tile_entry_slot<G>(e) != slot || tile_entry_code<G>(e) != code || tile_entry_ne<G>(e) != ne) return false;
            if (pmf != tab_pmf<G>(slot, code) || exp != tab_exp<G>(slot, ne)) return false;
            if (pmf >= G::LROW * G::BL || exp >= G::LROW * G::BL) return false;
            if (G::OFFSET_ENTRIES && (G::LROW - G::NCODE + code - ne > 15u || exp >= 4096u)) return false;  // c: 4 bits, E: 12
        }
    return true;
}
static_assert(!geo_reg::OFFSET_ENTRIES || (geo_reg::LROW - geo_reg::NCODE) * geo_reg::BL <= 4096u,
              "offset entries: the expected-term planes' elements take 12 bits");
static_assert(tile_entries_round_trip<geo_reg>(), "regular tile entries");
static_assert(tile_entries_round_trip<geo_t2<6>>(), "tier-2 tile entries, totals 5..6");
static_assert(tile_entries_round_trip<geo_t2<8>>(), "tier-2 tile entries, totals 5..8");
static_assert(tile_code_ne<geo_reg>(0) == 0 && tile_code_ne<geo_reg>(1) == 0 && tile_code_ne<geo_reg>(2) == 1 &&
              tile_code_ne<geo_reg>(4) == 1 && tile_code_ne<geo_reg>(5) == 2 && tile_code_ne<geo_reg>(8) == 2 &&
              tile_code_ne<geo_reg>(9) == 3 && tile_code_ne<geo_reg>(T_NCODE - 1) == 3, "codes of the totals 1..T_K (ent_code)");
static_assert(tile_code_ne<geo_t2<8>>(5) == 0 && tile_code_ne<geo_t2<8>>(6) == 1 && tile_code_ne<geo_t2<8>>(13) == 2 &&
              tile_code_ne<geo_t2<8>>(20) == 2 && tile_code_ne<geo_t2<8>>(21) == 3 && tile_code_ne<geo_t2<6>>(12) == 1,
              "codes of the totals 5..8 (t2_code)");

// overflow entries (alt+ref == 0 or > T_K)
#define LF_LANES 16  // lanes that share a locus (k_locus_finalize) or a row (k_ovf_cell_wide)
#define OV_NT 18  // cumulative tables cover counts 0..17; larger counts take the generic device_math path
#define OV_NE 17  // expected terms E(n) tabulated for n = 4..17
#define OV_FAST_N DM_CHUNK  // the cell side's fast kernel takes totals up to this (99 % of the overflow entries)
#define OV_ROW 128  // doubles of a locus' overflow table row (k_ovf_tables); its E(n) start at OV_EOFF
#define OV_EOFF 64
#define OV_REC 8  // the cell side's per-locus record: alpha, beta, E(5..8), pad = ONE 64-byte sector per overflow entry
#define OVF_PAD (~0ull)  // padding slot of the 64-row ELLPACK copy (k_ovf_ell_build)

// tier 2: the overflow entries with totals 5..8 (k_t2_tables)
#define T2_NMIN 5u
#define T2_NMAX 8u
#define T2_NCODE 30    // (alt, ref) pairs with 5 <= alt+ref <= 8; code = n(n+1)/2 - 15 + ref
#define T2_CSTRIDE 32  // u32 counters per locus (hist_all2, cnt2)
#define T2_ROW 48      // table doubles per locus
static_assert(T2_NMAX == (unsigned)OV_FAST_N, "the tier lists take the totals above tier 2");
__device__ __forceinline__ bool t2_total(uint32_t n) { return n - T2_NMIN <= T2_NMAX - T2_NMIN; }
__device__ __forceinline__ uint32_t t2_code(uint32_t n, uint32_t r) { return n * (n + 1u) / 2u - 15u + r; }
// position of the pair's log-pmf in the locus' table row; its sector's first double is E(n)
__device__ __forceinline__ uint32_t t2_pos(uint32_t n, uint32_t r)
{
    const uint32_t hi = r >= 7u ? 1u : 0u;
    return ((n - T2_NMIN) + (n == 8u ? 1u : 0u) + hi) * 8u + 1u + (hi ? r - 7u : r);
}
// the tier list an overflow entry goes to (k_ovf_tier_lists): none, 0 = totals 9..OV_NE, 1 = above
__device__ __forceinline__ int ovf_tier(uint64_t en)
{
    const uint32_t n = ENT_ALT(en) + ENT_REF(en);
    return n <= (uint32_t)OV_FAST_N ? -1 : (n <= (uint32_t)OV_NE ? 0 : 1);
}

// compact CSC entry of the locus pass: 24 bits (cell 20 | code 4) or 32 bits (cell 28 | code 4)
template <int EB>
__device__ __forceinline__ void c4_read1(const uint32_t *__restrict__ base, uint64_t i, uint32_t *cell, uint32_t *code)
{
    if (EB == 32) {
        const uint32_t x = base[i];
        *cell = x & 0x0fffffffu;
        *code = x >> 28;
    } else {
        const uint8_t *b = reinterpret_cast<const uint8_t *>(base) + 3 * i;
        const uint32_t v = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16);
        *cell = v & 0xfffffu;
        *code = v >> 20;
    }
}
template <int EB>
__device__ __forceinline__ void c4_write1(uint32_t *__restrict__ base, uint64_t i, uint32_t cell, uint32_t code)
{
    if (EB == 32) {
        base[i] = cell | (code << 28);
    } else {
        uint8_t *b = reinterpret_cast<uint8_t *>(base) + 3 * i;
        const uint32_t v = cell | (code << 20);
        b[0] = (uint8_t)v; b[1] = (uint8_t)(v >> 8); b[2] = (uint8_t)(v >> 16);
    }
}
// Form of the locus pass, decided on the device from this shard's exclusion-set size (locus_by_minority)
#define LM_NUM 1  // minority-driven when n_min / nloc <= LM_NUM / LM_DEN
#define LM_DEN 8

// Locus ranges of the minority-driven locus pass.  A (cell, range) segment is a short run inside a long row and memory comes in 128-byte lines, so short segments waste
// most of what they fetch (measured at 1024 loci per range: 80-byte segments, 2 GB fetched for 0.8 GB of entries, the
// kernel at the HBM rate).  Hence wide ranges, with 16-bit counters so that the histogram still fits in LDS.
#define LR_LOCI 4096     // loci per range: the LDS histogram is 14 codes x LR_LOCI x u16 = 112 KB
#define LR_SUB_MAX 16    // at most this many subsets of the exclusion set (partial planes); chosen per matrix
#define LR_THREADS 1024  // one workgroup per CU, 128 VGPRs: 16 entry loads per lane stay in flight
#define LR_GROUP 64      // lanes per (cell, range) segment: ~41 entries at 1 % density (a tail loop would serialise)
#define LR_ROW (LR_LOCI + 2)  // u16 counters per code row (even: a row starts on a word)
#define LT_CELLS 64  // cells per workgroup of k_minority_offsets
#define TB_BINS 64  // entry counts >= TB_BINS-1 share the last bin (they sort to the end, in cell order)
// u16 of a tile staged in LDS (48 KB: two workgroups per CU); a bigger tile is written directly (rows of hundreds of entries)
#define TB_STAGE (24 * 1024)

// ---- host side ----
static inline unsigned gcap(uint64_t n, unsigned per_block, unsigned cap = 1u << 20)
{
    uint64_t g = (n + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (unsigned)g;
}

// A run-time bool as a template argument: f is a generic lambda, called with std::true_type or std::false_type, so that a launch
// and its argument list are written once.  Only what f names for each of the two gets instantiated.
template <class F>
static inline void with_bool(bool b, F &&f)
{
    if (b) f(std::true_type());
    else f(std::false_type());
}

// The build's recurring step for an output in CSR form.  Every array of `a` is [n + 1] with its last slot zeroed by the caller:
// pass(false) launches the kernels that COUNT into [0, n) (it gets the payload pointers as they are then: not dereferenced), an
// exclusive scan per array, in the order listed, turns the counts into offsets and slot n into the total, payload() allocates from
// the totals and pass(true) launches the same kernels to FILL.
struct CountedPtr { uint64_t *ptr, *total; };
template <class Pass, class Payload>
static inline cellector_status count_scan_fill(cellector_ctx *c, uint64_t n, std::initializer_list<CountedPtr> a, Pass pass,
                                               Payload payload)
{
    pass(std::false_type());
    HIPCHK(c, hipGetLastError());
    for (const CountedPtr &p : a) CHK(dev_exclusive_scan_u64(c, p.ptr, n + 1, p.total));
    CHK(payload());
    pass(std::true_type());
    HIPCHK(c, hipGetLastError());
    return CELLECTOR_OK;
}
