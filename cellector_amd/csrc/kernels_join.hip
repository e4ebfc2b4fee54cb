// The keyed join of two count streams into a staged COO (cellector_ingest_mtx_joined / _coo_joined; contract in
// include/cellector_ffi.h, numpy twin cellector_amd/join.py).  FIRST and SECOND are token arrays (locus, cell, count) in any
// order; the result has one entry per distinct (locus, cell) of either, ascending strictly by the 64-bit key locus << 32 | cell.
//
//   check      per side: index 0 / range / count above 65535 as k_pair_check reports them (smallest entry << 3 | its kind), the
//              0-based key of every entry written beside its count, and is the side strictly ascending?
//   sort       a side that is not: rocprim radix sort of (key, count); an ascending side is taken as it stands
//   duplicates adjacent equal keys of a sorted side; the smallest per side
//   join       merge path over tiles of JOIN_TILE steps through the two key arrays.  k_join_partition binary-searches every tile's
//              cross-diagonal; a cut that falls between A[i] and an equal B[j] (FIRST goes first among equals) moves one step
//              down SECOND, so a matched pair is never split and a tile holds at most JOIN_TILE + 1 entries.  k_join_count stages
//              a tile's two key ranges in LDS and counts the matches (a binary search per FIRST key); a scan of the tile counts
//              gives every tile its place; k_join_emit stages the keys again, ranks every entry among the tile's outputs
//              (own index + the other side's keys below - the matched pairs below, from a block scan of the match flags) and
//              writes locus, cell, alt, ref in output order.  Each pass reads every key once, the second every count once; no
//              merged intermediate exists.
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "ctx.h"
#include "lane_rows.h"

#define JOIN_TILE 2048
#define JB 256
#define JT_CAP (JOIN_TILE + 1)                // entries of a tile: a cut moved for a matched pair adds one
#define JT_ITEMS ((JT_CAP + JB - 1) / JB)     // rounds of the block over a tile
#define JT_NONE 0xffffu

static_assert(JT_CAP < 0x8000, "an entry's place inside its tile and a match bit share 16 bits");

enum { JE_NONE = 0, JE_INDEX0 = 1, JE_LOCUS = 2, JE_CELL = 3, JE_COUNT = 4 };  // (the kinds of k_pair_check, in its order)
#define JE_KIND_BITS 3
static const char *const je_what[] = {"", "index 0 (indices are 1-based)", "locus index out of range", "cell index out of range",
                                      "count above 65535 not supported"};
static const char *const je_side[] = {"FIRST", "SECOND"};

static inline unsigned jgrid(uint64_t n) { return (unsigned)((n + JB - 1) / JB ? (n + JB - 1) / JB : 1); }

// ---- check ----------------------------------------------------------------------------------------------------------------------
// base: 1 for the tokens of a text file, 0 for a caller's COO
__global__ __launch_bounds__(JB) void k_join_check(uint64_t n, const uint32_t *__restrict__ locus, const uint32_t *__restrict__ cell,
                                                   const uint32_t *__restrict__ count, uint32_t base, uint64_t total_loci,
                                                   uint64_t total_cells, uint64_t *__restrict__ key, unsigned long long *__restrict__ first_bad,
                                                   uint32_t *__restrict__ not_ascending)
{
    const uint64_t i = (uint64_t)blockIdx.x * JB + threadIdx.x;
    if (i >= n) return;
    const uint32_t l = locus[i], c = cell[i];
    uint32_t kind = JE_NONE;
    if (base && (l == 0 || c == 0)) kind = JE_INDEX0;
    else if ((uint64_t)(l - base) >= total_loci) kind = JE_LOCUS;
    else if ((uint64_t)(c - base) >= total_cells) kind = JE_CELL;
    else if (count[i] > CELLECTOR_MAX_COUNT) kind = JE_COUNT;
    if (kind != JE_NONE) atomicMin(first_bad, ((unsigned long long)i << JE_KIND_BITS) | kind);
    const uint64_t k = (uint64_t)(l - base) << 32 | (uint64_t)(c - base);
    key[i] = k;
    // (a refused entry's key means nothing: the call fails before anyone reads the flag)
    if (i > 0 && ((uint64_t)(locus[i - 1] - base) << 32 | (uint64_t)(cell[i - 1] - base)) >= k) *not_ascending = 1u;
}

// ---- duplicates -----------------------------------------------------------------------------------------------------------------
// both sides in one launch (n = 0: a side that arrived strictly ascending has none); dup[s] = the smallest key side s lists twice
__global__ __launch_bounds__(JB) void k_join_dups(uint64_t na, const uint64_t *__restrict__ ka, uint64_t nb, const uint64_t *__restrict__ kb,
                                                  unsigned long long *__restrict__ dup)
{
    const uint64_t i = (uint64_t)blockIdx.x * JB + threadIdx.x + 1;
    if (i < na && ka[i - 1] == ka[i]) atomicMin(&dup[0], (unsigned long long)ka[i]);
    if (i < nb && kb[i - 1] == kb[i]) atomicMin(&dup[1], (unsigned long long)kb[i]);
}

// ---- partition ------------------------------------------------------------------------------------------------------------------
// Cut t lies on the cross-diagonal d = min(t * JOIN_TILE, na + nb): a_start[t] = the lowest a with A[a] > B[d - 1 - a] (FIRST first
// among equals), b_start[t] = d - a, one more when A[a - 1] == B[b]: the pair goes to the tile in front of the cut.  (B[b] is the
// next step of the path then, A[a] being above A[a - 1]: every later cut lies behind it, and the cuts stay monotone on both sides.)
__global__ __launch_bounds__(JB) void k_join_partition(uint64_t na, const uint64_t *__restrict__ ka, uint64_t nb, const uint64_t *__restrict__ kb,
                                                       uint64_t ntiles, uint64_t *__restrict__ a_start /*[ntiles + 1]*/,
                                                       uint64_t *__restrict__ b_start /*[ntiles + 1]*/)
{
    const uint64_t t = (uint64_t)blockIdx.x * JB + threadIdx.x;
    if (t > ntiles) return;
    const uint64_t n = na + nb;
    const uint64_t d = t * JOIN_TILE < n ? t * JOIN_TILE : n;
    uint64_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);  // (mid < na; 0 <= d - 1 - mid < nb)
        if (ka[mid] <= kb[d - 1 - mid]) lo = mid + 1;
        else hi = mid;
    }
    uint64_t b = d - lo;
    if (lo > 0 && b < nb && ka[lo - 1] == kb[b]) b++;
    a_start[t] = lo;
    b_start[t] = b;
}

// ---- a tile's keys in LDS ---------------------------------------------------------------------------------------------------------
struct JoinTile { uint64_t a0, b0; uint32_t ca, cb; };

// false: the cuts do not describe a tile (a side was not ascending after all) — nothing out of range is touched
__device__ __forceinline__ bool join_tile_load(uint64_t na, const uint64_t *__restrict__ ka, uint64_t nb, const uint64_t *__restrict__ kb,
                                               const uint64_t *__restrict__ a_start, const uint64_t *__restrict__ b_start, uint64_t *keys,
                                               JoinTile *t)
{
    const uint64_t a0 = a_start[blockIdx.x], a1 = a_start[blockIdx.x + 1], b0 = b_start[blockIdx.x], b1 = b_start[blockIdx.x + 1];
    if (a0 > a1 || a1 > na || b0 > b1 || b1 > nb || (a1 - a0) + (b1 - b0) > JT_CAP) return false;
    t->a0 = a0; t->b0 = b0; t->ca = (uint32_t)(a1 - a0); t->cb = (uint32_t)(b1 - b0);
    const uint32_t ca = t->ca, cnt = t->ca + t->cb;
#pragma unroll
    for (int k = 0; k < JT_ITEMS; k++) {
        const uint32_t j = (uint32_t)k * JB + threadIdx.x;
        if (j < ca) keys[j] = ka[a0 + j];
        else if (j < cnt) keys[j] = kb[b0 + (j - ca)];
    }
    __syncthreads();
    return true;
}

// the lowest index in keys[0, n) whose key is not below `key`
__device__ __forceinline__ uint32_t join_lower_bound(const uint64_t *keys, uint32_t n, uint64_t key)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ---- pass 1: outputs per tile -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(JB) void k_join_count(uint64_t na, const uint64_t *__restrict__ ka, uint64_t nb, const uint64_t *__restrict__ kb,
                                                   const uint64_t *__restrict__ a_start, const uint64_t *__restrict__ b_start,
                                                   uint64_t *__restrict__ tile_out /*[ntiles + 1]*/, uint32_t *__restrict__ inconsistent)
{
    __shared__ uint64_t keys[JT_CAP];
    __shared__ uint32_t s_matched;
    if (threadIdx.x == 0) s_matched = 0;
    JoinTile t;
    if (!join_tile_load(na, ka, nb, kb, a_start, b_start, keys, &t)) {  // (block-uniform: the cuts are the same for every thread)
        if (threadIdx.x == 0) { *inconsistent = 1u; tile_out[blockIdx.x] = 0; }
        return;
    }
    uint32_t mine = 0;
#pragma unroll
    for (int k = 0; k < JT_ITEMS; k++) {
        const uint32_t j = (uint32_t)k * JB + threadIdx.x;
        if (j >= t.ca) continue;
        const uint32_t lb = join_lower_bound(keys + t.ca, t.cb, keys[j]);
        mine += lb < t.cb && keys[t.ca + lb] == keys[j];
    }
    if (mine) atomicAdd(&s_matched, mine);
    __syncthreads();
    if (threadIdx.x == 0) tile_out[blockIdx.x] = (uint64_t)(t.ca + t.cb - s_matched);
}

// ---- pass 2: the entries ----------------------------------------------------------------------------------------------------------
// depth: SECOND holds alt + ref (CELLECTOR_JOIN_DEPTH); low[0] = the smallest key whose depth is below its alt count
__global__ __launch_bounds__(JB) void k_join_emit(uint64_t na, const uint64_t *__restrict__ ka, const uint32_t *__restrict__ va, uint64_t nb,
                                                  const uint64_t *__restrict__ kb, const uint32_t *__restrict__ vb,
                                                  const uint64_t *__restrict__ a_start, const uint64_t *__restrict__ b_start,
                                                  const uint64_t *__restrict__ tile_off /*[ntiles + 1], scanned*/, int depth,
                                                  uint32_t *__restrict__ o_locus, uint32_t *__restrict__ o_cell, uint16_t *__restrict__ o_alt,
                                                  uint16_t *__restrict__ o_ref, unsigned long long *__restrict__ low,
                                                  uint32_t *__restrict__ inconsistent)
{
    __shared__ uint64_t keys[JT_CAP];    // FIRST's range, then SECOND's
    __shared__ uint16_t other[JT_CAP];   // per FIRST entry: SECOND's keys below it | 0x8000 when SECOND holds the key itself
    __shared__ uint32_t below[JT_CAP + 1];  // matched FIRST entries in front of FIRST entry j (j = ca: all of them)
    __shared__ uint16_t from[JT_CAP];    // per output entry of the tile: its index in keys
    __shared__ uint32_t part[JB];
    JoinTile t;
    if (!join_tile_load(na, ka, nb, kb, a_start, b_start, keys, &t)) {
        if (threadIdx.x == 0) *inconsistent = 1u;
        return;
    }
    const uint32_t ca = t.ca, cb = t.cb, cnt = ca + cb;
    const uint64_t off = tile_off[blockIdx.x];
    const uint64_t room = tile_off[blockIdx.x + 1] - off;  // what pass 1 counted: nothing is written beyond it
#pragma unroll
    for (int k = 0; k < JT_ITEMS; k++) {
        const uint32_t j = (uint32_t)k * JB + threadIdx.x;
        if (j < JT_CAP) from[j] = JT_NONE;
        if (j >= ca) continue;
        const uint32_t lb = join_lower_bound(keys + ca, cb, keys[j]);
        other[j] = (uint16_t)(lb | ((lb < cb && keys[ca + lb] == keys[j]) ? 0x8000u : 0u));
    }
    __syncthreads();
    // exclusive scan of the match bits over FIRST's entries: a thread sums JT_ITEMS consecutive ones, the block scans the sums
    const uint32_t s0 = threadIdx.x * JT_ITEMS;
    uint32_t sum = 0;
    for (uint32_t j = s0; j < s0 + JT_ITEMS && j < ca; j++) sum += other[j] >> 15;
    part[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < JB; d <<= 1) {
        const uint32_t v = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    uint32_t run = part[threadIdx.x] - sum;
    for (uint32_t j = s0; j < s0 + JT_ITEMS && j < ca; j++) { below[j] = run; run += other[j] >> 15; }
    const uint32_t matched = part[JB - 1];
    if (threadIdx.x == 0) below[ca] = matched;
    __syncthreads();
    const uint32_t n_out = cnt - matched;
    // an entry's place among the tile's outputs = the keys below it on both sides - the pairs among them
#pragma unroll
    for (int k = 0; k < JT_ITEMS; k++) {
        const uint32_t j = (uint32_t)k * JB + threadIdx.x;
        if (j >= cnt) continue;
        uint32_t pos;
        if (j < ca) pos = j + (other[j] & 0x7fffu) - below[j];
        else {
            const uint32_t lb = join_lower_bound(keys, ca, keys[j]);
            if (lb < ca && keys[lb] == keys[j]) continue;  // (FIRST's entry writes the pair)
            pos = lb + (j - ca) - below[lb];
        }
        if (pos < n_out) from[pos] = (uint16_t)j;
        else *inconsistent = 1u;
    }
    __syncthreads();
    if (n_out != room && threadIdx.x == 0) *inconsistent = 1u;
#pragma unroll
    for (int k = 0; k < JT_ITEMS; k++) {
        const uint32_t r = (uint32_t)k * JB + threadIdx.x;
        if (r >= n_out || r >= room) continue;
        const uint32_t j = from[r];
        if (j >= cnt) { *inconsistent = 1u; continue; }
        const uint64_t key = keys[j];
        uint32_t a = 0, b = 0;
        if (j < ca) {
            a = va[t.a0 + j];
            if (other[j] & 0x8000u) b = vb[t.b0 + (other[j] & 0x7fffu)];
        } else
            b = vb[t.b0 + (j - ca)];
        if (depth) {
            if (b < a) { atomicMin(low, (unsigned long long)key); b = a; }
            b -= a;
        }
        o_locus[off + r] = (uint32_t)(key >> 32);
        o_cell[off + r] = (uint32_t)key;
        o_alt[off + r] = (uint16_t)a;
        o_ref[off + r] = (uint16_t)b;
    }
}

// =================================================================================================================================
namespace {

struct JoinStatus {  // the status words of a join on the device: bad[s] check of side s, bad[2 + s] its duplicate, bad[4] depth < alt
    DevBuf<unsigned long long> bad;
    DevBuf<uint32_t> flags;  // [0], [1]: side s is not strictly ascending; [2]: the join kernels met cuts that describe no tile
    unsigned long long h_bad[5] = {~0ull, ~0ull, ~0ull, ~0ull, ~0ull};
    uint32_t h_flags[4] = {0, 0, 0, 0};
    cellector_status init(cellector_ctx *c)
    {
        CHK(dev_alloc(c, &bad, 5)); CHK(dev_alloc(c, &flags, 4));
        HIPCHK(c, hipMemcpyAsync(bad, h_bad, sizeof h_bad, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(flags, h_flags, sizeof h_flags, hipMemcpyHostToDevice, c->stream));
        return CELLECTOR_OK;
    }
    cellector_status read(cellector_ctx *c)
    {
        HIPCHK(c, hipMemcpyAsync(h_bad, bad, sizeof h_bad, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(h_flags, flags, sizeof h_flags, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return CELLECTOR_OK;
    }
};

// (key, count) of a side sorted by key into new arrays, which replace the side's
cellector_status join_sort(cellector_ctx *c, DevBuf<uint64_t> *key, DevBuf<uint32_t> *count, uint64_t n, unsigned end_bit)
{
    DevBuf<uint64_t> key_o;
    DevBuf<uint32_t> count_o;
    DevBuf<char> tmp;
    CHK(dev_alloc(c, &key_o, n)); CHK(dev_alloc(c, &count_o, n));
    size_t tmp_bytes = 0;
    HIPCHK(c, rocprim::radix_sort_pairs(nullptr, tmp_bytes, key->get(), key_o.get(), count->get(), count_o.get(), (size_t)n, 0u, end_bit, c->stream));
    CHK(dev_alloc(c, &tmp, tmp_bytes));
    hipError_t e = rocprim::radix_sort_pairs(tmp.get(), tmp_bytes, key->get(), key_o.get(), count->get(), count_o.get(), (size_t)n, 0u, end_bit,
                                             c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    HIPCHK(c, e);
    *key = std::move(key_o);
    *count = std::move(count_o);
    return CELLECTOR_OK;
}

}  // namespace

cellector_status join_stage(cellector_ctx *c, JoinTokens *first, JoinTokens *second, uint32_t index_base, int mode, StagedCoo *out,
                            cellector_join_summary *sum, JoinPhases *ph)
{
    JoinTokens *side[2] = {first, second};
    DevBuf<uint64_t> key[2];
    JoinStatus js;
    LapTimer lap;
    CHK(js.init(c));
    // ---- checks: the index arrays become one key array per side and go
    for (int s = 0; s < 2; s++) {
        const uint64_t n = side[s]->n;
        CHK(dev_alloc(c, &key[s], n));
        if (n)
            hipLaunchKernelGGL(k_join_check, dim3(jgrid(n)), dim3(JB), 0, c->stream, n, side[s]->locus.get(), side[s]->cell.get(),
                               side[s]->count.get(), index_base, c->total_loci, c->total_cells, key[s].get(), js.bad.get() + s, js.flags.get() + s);
        HIPCHK(c, hipGetLastError());
    }
    CHK(js.read(c));
    for (int s = 0; s < 2; s++) { side[s]->locus.reset(); side[s]->cell.reset(); }
    for (int s = 0; s < 2; s++)
        if (js.h_bad[s] != ~0ull) {
            const unsigned kind = (unsigned)(js.h_bad[s] & ((1u << JE_KIND_BITS) - 1));
            return ctx_fail(c, CELLECTOR_EINVAL, "join: %s entry %llu: %s", je_side[s], js.h_bad[s] >> JE_KIND_BITS, je_what[kind <= JE_COUNT ? kind : 0]);
        }
    ph->checks = lap.lap();
    // ---- order
    const bool asc[2] = {js.h_flags[0] == 0, js.h_flags[1] == 0};
    unsigned end_bit = 33;  // the key's bits in use: 32 of the cell, those of the largest locus
    while (end_bit < 64 && (c->total_loci >> (end_bit - 32)) != 0) end_bit++;
    for (int s = 0; s < 2; s++)
        if (!asc[s]) CHK(join_sort(c, &key[s], &side[s]->count, side[s]->n, end_bit));
    if (!asc[0] || !asc[1]) {
        const uint64_t na = asc[0] ? 0 : side[0]->n, nb = asc[1] ? 0 : side[1]->n, n = na > nb ? na : nb;
        if (n > 1) hipLaunchKernelGGL(k_join_dups, dim3(jgrid(n - 1)), dim3(JB), 0, c->stream, na, key[0].get(), nb, key[1].get(), js.bad.get() + 2);
        HIPCHK(c, hipGetLastError());
        CHK(js.read(c));
        for (int s = 0; s < 2; s++)
            if (js.h_bad[2 + s] != ~0ull)
                return ctx_fail(c, CELLECTOR_EINVAL, "join: %s lists (locus %llu, cell %llu) twice", je_side[s], (js.h_bad[2 + s] >> 32) + 1,
                                (js.h_bad[2 + s] & 0xffffffffull) + 1);
    }
    ph->sorts = lap.lap();
    // ---- the join
    const uint64_t na = side[0]->n, nb = side[1]->n, n = na + nb, ntiles = (n + JOIN_TILE - 1) / JOIN_TILE;
    REQUIRE(c, ntiles <= 0x7fffffffull, "join: more tiles than a grid holds");
    DevBuf<uint64_t> a_start, b_start, tile_off;
    CHK(dev_alloc(c, &a_start, ntiles + 1)); CHK(dev_alloc(c, &b_start, ntiles + 1)); CHK(dev_alloc(c, &tile_off, ntiles + 1));
    EventMarks<2> marks;
    uint64_t n_out = 0;
    marks.mark(0, c->stream);
    if (ntiles) {
        HIPCHK(c, hipMemsetAsync(tile_off, 0, (ntiles + 1) * 8, c->stream));
        hipLaunchKernelGGL(k_join_partition, dim3(jgrid(ntiles + 1)), dim3(JB), 0, c->stream, na, key[0].get(), nb, key[1].get(), ntiles,
                           a_start.get(), b_start.get());
        hipLaunchKernelGGL(k_join_count, dim3((unsigned)ntiles), dim3(JB), 0, c->stream, na, key[0].get(), nb, key[1].get(), a_start.get(),
                           b_start.get(), tile_off.get(), js.flags.get() + 2);
        HIPCHK(c, hipGetLastError());
        CHK(dev_exclusive_scan_u64(c, tile_off, ntiles + 1, &n_out));
    }
    REQUIRE(c, n_out <= n, "join: the tile counts exceed the entries read");  // (never: a tile counts at most what it holds)
    CHK(out->alloc(c, n_out));
    if (ntiles) {
        hipLaunchKernelGGL(k_join_emit, dim3((unsigned)ntiles), dim3(JB), 0, c->stream, na, key[0].get(), side[0]->count.get(), nb, key[1].get(),
                           side[1]->count.get(), a_start.get(), b_start.get(), tile_off.get(), mode == CELLECTOR_JOIN_DEPTH ? 1 : 0,
                           out->locus.get(), out->cell.get(), out->alt.get(), out->ref.get(), js.bad.get() + 4, js.flags.get() + 2);
        HIPCHK(c, hipGetLastError());
    }
    marks.mark(1, c->stream);
    CHK(js.read(c));
    for (int s = 0; s < 2; s++) { key[s].reset(); side[s]->count.reset(); }  // (the tokens go as soon as the COO is written)
    if (js.h_flags[2]) return ctx_fail(c, CELLECTOR_EDEVICE, "join: the merge met a side that does not ascend by (locus, cell)");
    if (js.h_bad[4] != ~0ull)
        return ctx_fail(c, CELLECTOR_EINVAL, "join: depth below alt at (locus %llu, cell %llu)", (js.h_bad[4] >> 32) + 1,
                        (js.h_bad[4] & 0xffffffffull) + 1);
    ph->join = lap.lap();
    float ms = 0.f;
    ph->join_kernels_ms = marks.ms(0, 1, &ms) ? (double)ms : -1.0;
    out->sorted = true;
    if (sum) {
        const uint64_t both = n - n_out;
        *sum = cellector_join_summary{na, nb, both, na - both, nb - both, n_out, asc[0] ? 1u : 0u, asc[1] ? 1u : 0u, JOIN_TILE, 0u};
    }
    return CELLECTOR_OK;
}
