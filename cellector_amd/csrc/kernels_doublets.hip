// cellector_add_doublets: synthetic doublets made of cells the ctx holds.  What the reference's `combiner` announces and never
// does (combiner/src/main.rs:43, "decide which cells are doublets and that mapping"): two droplets' reads in one barcode, so at
// every locus either parent covers the new cell holds the SUM of their counts, added before anything is scored.
//
//   fan     the host turns the pair lists into a CSR over cells: cell c is side s of pair j for every value 2 j + s in
//           fan_val[fan_ptr[c] .. fan_ptr[c + 1])
//   count   one number per tile of DOUBLETS_TILE staged entries: the records its entries emit (an entry of cell c emits one per
//           fan value of c)
//   scan    dev_exclusive_scan_u64 over the tile counts only
//   emit    a block takes its tile in rounds of one entry per thread, scans the round's fan-outs in LDS and then deals the
//           round's RECORDS to its threads, not its entries: the 260 records of a hub cell's entry go to 260 lanes.  A record is
//           the key locus << 32 | (n_ctx + j) and the two thinned counts; a count above DB_LANE_READS is drawn by all 64 lanes of
//           the wave, read r on lane r % 64
//   sort    rocprim::radix_sort_pairs of the records by key (the bits a key can have)
//   sum     head flags (a key that differs from the one before it) + dev_exclusive_scan_u64 number the distinct keys; every
//           record adds its counts to its key's two 32-bit sums (integer atomics: the order does not matter), the head also
//           writes locus and cell; a last pass narrows the sums to 16 bits and keeps the first one above CELLECTOR_MAX_COUNT
//
// The result ascends strictly by (locus, cell): the side cellector_combine's merge takes as it stands.
//
// The draw (doublets.py is the numpy twin): for the parent entry at position i of the arrays the call reads, pair j, side s,
// allele a (0 = ref, 1 = alt) and read r = 0..count-1
//   h = mix64(mix64((seed * GOLD) ^ ((i + 1) * GOLD)) ^ ((2 j + s + 1) * GOLD)),   x = mix64(h + (2 r + a + 1) * GOLD),
//   removed iff (x >> 11) < T,   T = (uint64_t)(downsample_rate * 2^53)
// the inner hash is cellector_restage's entry hash, so a cell that is a parent in many pairs is thinned anew for each.
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "ctx.h"
#include "mix64.h"

// staged entries per tile of the count and emit passes (doublets.py exports it as TILE)
#define DOUBLETS_TILE 2048
#define DB_BLOCK 256
#define DB_ROUNDS (DOUBLETS_TILE / DB_BLOCK)
#define DB_LANE_READS 128u  // a larger count is drawn by the whole wave
#define DB_NONE 0xffffffffffffffffull

static_assert(DOUBLETS_TILE % DB_BLOCK == 0, "a tile is whole rounds of the block");

static inline unsigned db_grid(uint64_t n) { return (unsigned)((n + DB_BLOCK - 1) / DB_BLOCK ? (n + DB_BLOCK - 1) / DB_BLOCK : 1); }

// ---- count pass: records per tile ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DB_BLOCK) void k_db_count(uint64_t n, uint64_t tc, const uint32_t *__restrict__ cell,
                                                       const uint64_t *__restrict__ fan_ptr /*[tc + 1]*/, uint64_t *__restrict__ tile_cnt)
{
    __shared__ uint64_t part[DB_BLOCK];
    const uint64_t base = (uint64_t)blockIdx.x * DOUBLETS_TILE;
    uint64_t cnt = 0;
#pragma unroll 4
    for (int k = 0; k < DB_ROUNDS; k++) {
        const uint64_t i = base + (uint64_t)k * DB_BLOCK + threadIdx.x;
        if (i < n) {
            const uint32_t c0 = cell[i];
            if (c0 < tc) cnt += fan_ptr[c0 + 1] - fan_ptr[c0];
        }
    }
    part[threadIdx.x] = cnt;
    __syncthreads();
#pragma unroll
    for (int off = DB_BLOCK / 2; off; off >>= 1) {
        if ((int)threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = part[0];
}

// ---- emit pass ------------------------------------------------------------------------------------------------------------------
// reads of one count that survive, drawn by one lane
__device__ __forceinline__ uint32_t db_thin_lane(uint64_t h, uint32_t count, uint32_t allele, uint64_t T)
{
    uint32_t kept = 0;
    for (uint32_t r = 0; r < count; r++) {
        const uint64_t x = mix64(h + (uint64_t)(2u * r + allele + 1u) * GOLD);
        kept += (x >> 11) < T ? 0u : 1u;
    }
    return kept;
}

// ... of the counts of every lane of a wave (all 64 lanes call it together; a lane without a record passes count 0): a count of
// at most DB_LANE_READS is its own lane's loop, a larger one is taken in turn and drawn by all lanes, read r on lane r % 64, so
// 65535 reads are 1024 steps per lane instead of 65535 on one lane with 63 waiting
__device__ __forceinline__ uint32_t db_thin_wave(uint64_t h, uint32_t count, uint32_t allele, uint64_t T, int lane)
{
    uint32_t kept = count <= DB_LANE_READS ? db_thin_lane(h, count, allele, T) : 0u;
    uint64_t big = __ballot(count > DB_LANE_READS);
    while (big) {
        const int src = __ffsll((unsigned long long)big) - 1;
        big &= big - 1;
        const uint64_t hs = (uint64_t)(uint32_t)__shfl((int)(uint32_t)(h >> 32), src, 64) << 32 | (uint32_t)__shfl((int)(uint32_t)h, src, 64);
        const uint32_t cs = (uint32_t)__shfl((int)count, src, 64);
        uint32_t part = 0;
        for (uint32_t r = (uint32_t)lane; r < cs; r += 64u) {
            const uint64_t x = mix64(hs + (uint64_t)(2u * r + allele + 1u) * GOLD);
            part += (x >> 11) < T ? 0u : 1u;
        }
#pragma unroll
        for (int off = 32; off; off >>= 1) part += (uint32_t)__shfl_xor((int)part, off, 64);
        if (lane == src) kept = part;
    }
    return kept;
}

template <bool THIN>
__global__ __launch_bounds__(DB_BLOCK) void k_db_emit(uint64_t n, uint64_t tc, const uint32_t *__restrict__ locus,
                                                      const uint32_t *__restrict__ cell, const uint16_t *__restrict__ alt,
                                                      const uint16_t *__restrict__ ref, const uint64_t *__restrict__ fan_ptr,
                                                      const uint64_t *__restrict__ fan_val, uint64_t n_fan,
                                                      const uint64_t *__restrict__ tile_off, uint64_t n_rec, uint64_t T, uint64_t seed_gold,
                                                      uint64_t *__restrict__ o_key, uint32_t *__restrict__ o_val)
{
    __shared__ uint64_t incl[DB_BLOCK];   // inclusive scan of the round's fan-outs
    __shared__ uint64_t first[DB_BLOCK];  // fan_ptr of the round's entries' cells
    const int lane = threadIdx.x & 63;
    const uint64_t base = (uint64_t)blockIdx.x * DOUBLETS_TILE;
    uint64_t pos = tile_off[blockIdx.x];
    for (int k = 0; k < DB_ROUNDS; k++) {
        const uint64_t i = base + (uint64_t)k * DB_BLOCK + threadIdx.x;
        uint64_t f0 = 0, d = 0;
        if (i < n) {
            const uint32_t c0 = cell[i];
            if (c0 < tc) { f0 = fan_ptr[c0]; d = fan_ptr[c0 + 1] - f0; }
        }
        first[threadIdx.x] = f0;
        incl[threadIdx.x] = d;
        __syncthreads();
#pragma unroll
        for (int off = 1; off < DB_BLOCK; off <<= 1) {
            const uint64_t below = (int)threadIdx.x >= off ? incl[threadIdx.x - off] : 0;
            __syncthreads();
            incl[threadIdx.x] += below;
            __syncthreads();
        }
        const uint64_t total = incl[DB_BLOCK - 1];  // the same in every thread: the loop below is uniform over the block
        for (uint64_t q0 = 0; q0 < total; q0 += DB_BLOCK) {
            const uint64_t q = q0 + threadIdx.x;
            const bool live = q < total;
            uint64_t key = 0, h = 0;
            uint32_t a = 0, r = 0;
            if (live) {
                uint32_t lo = 0, hi = DB_BLOCK - 1;  // the entry the record belongs to: the first e with incl[e] > q
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (incl[mid] > q) hi = mid;
                    else lo = mid + 1;
                }
                const uint64_t before = lo ? incl[lo - 1] : 0;
                const uint64_t at = first[lo] + (q - before);  // (below n_fan: the record is one of the cell's fan values)
                const uint64_t e = base + (uint64_t)k * DB_BLOCK + lo;
                const uint64_t fv = at < n_fan ? fan_val[at] : 0;
                key = (uint64_t)locus[e] << 32 | (uint64_t)(uint32_t)(tc + (fv >> 1));
                a = alt[e]; r = ref[e];
                if (THIN) h = mix64(mix64(seed_gold ^ ((e + 1) * GOLD)) ^ ((fv + 1) * GOLD));
            }
            if (THIN) {  // (every lane of the wave goes through the draw together)
                r = db_thin_wave(h, r, 0u, T, lane);
                a = db_thin_wave(h, a, 1u, T, lane);
            }
            if (live && pos + q < n_rec) {  // (always: the count pass saw the same fan-outs)
                o_key[pos + q] = key;
                o_val[pos + q] = r << 16 | a;
            }
        }
        pos += total;
        __syncthreads();  // (the next round writes incl and first)
    }
}

// ---- segmented sum --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool db_head(const uint64_t *__restrict__ key, uint64_t i) { return i == 0 || key[i] != key[i - 1]; }

__global__ __launch_bounds__(DB_BLOCK) void k_db_heads(uint64_t m, const uint64_t *__restrict__ key, uint64_t *__restrict__ scan /*[m + 1]*/)
{
    const uint64_t i = (uint64_t)blockIdx.x * DB_BLOCK + threadIdx.x;
    if (i > m) return;
    scan[i] = i < m && db_head(key, i) ? 1u : 0u;
}

// first[0]: the lowest 2 * entry + allele (0 = ref, 1 = alt) whose sum does not fit; a 32-bit sum that wraps is one of them
__device__ __forceinline__ void db_add(uint32_t *__restrict__ sum, uint32_t v, uint64_t code, unsigned long long *__restrict__ first)
{
    if (!v) return;
    const uint32_t old = atomicAdd(sum, v);
    if (old + v < old) atomicMin(first, (unsigned long long)code);
}

__global__ __launch_bounds__(DB_BLOCK) void k_db_sum(uint64_t m, uint64_t n_out, const uint64_t *__restrict__ key, const uint32_t *__restrict__ val,
                                                     const uint64_t *__restrict__ scan, uint32_t *__restrict__ o_locus,
                                                     uint32_t *__restrict__ o_cell, uint32_t *__restrict__ sum_ref,
                                                     uint32_t *__restrict__ sum_alt, unsigned long long *__restrict__ first)
{
    const uint64_t i = (uint64_t)blockIdx.x * DB_BLOCK + threadIdx.x;
    if (i >= m) return;
    const bool head = db_head(key, i);
    const uint64_t d = scan[i] + (head ? 1u : 0u) - 1u;  // heads up to and including i, less one (record 0 is a head)
    if (d >= n_out) return;                              // (never)
    const uint32_t v = val[i];
    db_add(sum_ref + d, v >> 16, 2 * d, first);
    db_add(sum_alt + d, v & 0xffffu, 2 * d + 1, first);
    if (head) {
        const uint64_t k = key[i];
        o_locus[d] = (uint32_t)(k >> 32);
        o_cell[d] = (uint32_t)k;
    }
}

__global__ __launch_bounds__(DB_BLOCK) void k_db_narrow(uint64_t n_out, const uint32_t *__restrict__ sum_ref, const uint32_t *__restrict__ sum_alt,
                                                        uint16_t *__restrict__ o_ref, uint16_t *__restrict__ o_alt,
                                                        unsigned long long *__restrict__ first)
{
    const uint64_t d = (uint64_t)blockIdx.x * DB_BLOCK + threadIdx.x;
    if (d >= n_out) return;
    const uint32_t r = sum_ref[d], a = sum_alt[d];
    if (r > CELLECTOR_MAX_COUNT) atomicMin(first, (unsigned long long)(2 * d));
    else if (a > CELLECTOR_MAX_COUNT) atomicMin(first, (unsigned long long)(2 * d + 1));
    o_ref[d] = (uint16_t)r;
    o_alt[d] = (uint16_t)a;
}

// ---- the new cells' origin: that of side a ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(DB_BLOCK) void k_db_origin(uint64_t n_pairs, uint64_t tc, const uint32_t *__restrict__ cell_a,
                                                        const uint32_t *__restrict__ old_origin /*null: identity*/, uint32_t *__restrict__ origin)
{
    const uint64_t j = (uint64_t)blockIdx.x * DB_BLOCK + threadIdx.x;
    if (j >= n_pairs) return;
    const uint32_t a = cell_a[j];
    origin[j] = old_origin && a < tc ? old_origin[a] : a;
}

cellector_status doublets_origin(cellector_ctx *c, const uint32_t *host_cell_a, uint64_t n_pairs, uint64_t tc, const uint32_t *old_origin,
                                 DevBuf<uint32_t> *origin)
{
    DevBuf<uint32_t> a;
    CHK(dev_alloc(c, &a, n_pairs)); CHK(dev_alloc(c, origin, n_pairs));
    HIPCHK(c, hipMemcpyAsync(a, host_cell_a, n_pairs * 4, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_db_origin, dim3(db_grid(n_pairs)), dim3(DB_BLOCK), 0, c->stream, n_pairs, tc, a.get(), old_origin, origin->get());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (a goes with this scope; the host array is the caller's)
    return CELLECTOR_OK;
}

// ---- the doublet side -------------------------------------------------------------------------------------------------------------
cellector_status doublets_build(cellector_ctx *c, const CooView &in, uint64_t tc, uint64_t total_loci, const uint64_t *host_fan_ptr,
                                const uint64_t *host_fan_val, uint64_t n_fan, uint64_t T, uint64_t seed, StagedCoo *out,
                                bool *overflow, uint64_t *over_pair, uint32_t *over_locus, int *over_allele)
{
    *overflow = false;
    const uint64_t n = in.n, ntiles = (n + DOUBLETS_TILE - 1) / DOUBLETS_TILE;
    DevBuf<uint64_t> fan_ptr, fan_val, tile_cnt;
    CHK(dev_alloc(c, &fan_ptr, tc + 1)); CHK(dev_alloc(c, &fan_val, n_fan)); CHK(dev_alloc(c, &tile_cnt, ntiles + 1));
    HIPCHK(c, hipMemcpyAsync(fan_ptr, host_fan_ptr, (tc + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(fan_val, host_fan_val, n_fan * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(tile_cnt + ntiles, 0, 8, c->stream));
    if (ntiles) hipLaunchKernelGGL(k_db_count, dim3((unsigned)ntiles), dim3(DB_BLOCK), 0, c->stream, n, tc, in.cell, fan_ptr.get(), tile_cnt.get());
    HIPCHK(c, hipGetLastError());
    uint64_t m = 0;  // records
    CHK(dev_exclusive_scan_u64(c, tile_cnt, ntiles + 1, &m));
    if (m == 0) {  // (every parent's row is empty)
        HIPCHK(c, hipStreamSynchronize(c->stream));
        out->sorted = true;
        return out->alloc(c, 0);
    }
    DevBuf<uint64_t> key, key_o;
    DevBuf<uint32_t> val, val_o;
    CHK(dev_alloc(c, &key, m)); CHK(dev_alloc(c, &val, m));
    if (T)
        hipLaunchKernelGGL(k_db_emit<true>, dim3((unsigned)ntiles), dim3(DB_BLOCK), 0, c->stream, n, tc, in.locus, in.cell, in.alt, in.ref,
                           fan_ptr.get(), fan_val.get(), n_fan, tile_cnt.get(), m, T, seed * GOLD, key.get(), val.get());
    else
        hipLaunchKernelGGL(k_db_emit<false>, dim3((unsigned)ntiles), dim3(DB_BLOCK), 0, c->stream, n, tc, in.locus, in.cell, in.alt, in.ref,
                           fan_ptr.get(), fan_val.get(), n_fan, tile_cnt.get(), m, T, seed * GOLD, key.get(), val.get());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (the host's fan table is read)
    fan_ptr.reset(); fan_val.reset(); tile_cnt.reset();
    {
        // the bits a key can have: 32 of the cell, those of the largest locus
        unsigned end_bit = 33;
        while (end_bit < 64 && ((total_loci ? total_loci - 1 : 0) >> (end_bit - 32))) end_bit++;
        DevBuf<char> tmp;
        CHK(dev_alloc(c, &key_o, m)); CHK(dev_alloc(c, &val_o, m));
        size_t tmp_bytes = 0;
        HIPCHK(c, rocprim::radix_sort_pairs(nullptr, tmp_bytes, key.get(), key_o.get(), val.get(), val_o.get(), (size_t)m, 0u, end_bit, c->stream));
        CHK(dev_alloc(c, &tmp, tmp_bytes));
        hipError_t e = rocprim::radix_sort_pairs(tmp.get(), tmp_bytes, key.get(), key_o.get(), val.get(), val_o.get(), (size_t)m, 0u, end_bit, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        HIPCHK(c, e);
    }
    key.reset(); val.reset();
    DevBuf<uint64_t> scan;
    CHK(dev_alloc(c, &scan, m + 1));
    hipLaunchKernelGGL(k_db_heads, dim3(db_grid(m + 1)), dim3(DB_BLOCK), 0, c->stream, m, key_o.get(), scan.get());
    HIPCHK(c, hipGetLastError());
    uint64_t n_out = 0;
    CHK(dev_exclusive_scan_u64(c, scan, m + 1, &n_out));
    DevBuf<uint32_t> sum_ref, sum_alt;
    DevBuf<unsigned long long> first;
    CHK(out->alloc(c, n_out)); CHK(dev_alloc(c, &sum_ref, n_out)); CHK(dev_alloc(c, &sum_alt, n_out)); CHK(dev_alloc(c, &first, 1));
    HIPCHK(c, hipMemsetAsync(sum_ref, 0, n_out * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(sum_alt, 0, n_out * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(first, 0xff, 8, c->stream));
    hipLaunchKernelGGL(k_db_sum, dim3(db_grid(m)), dim3(DB_BLOCK), 0, c->stream, m, n_out, key_o.get(), val_o.get(), scan.get(), out->locus.get(),
                       out->cell.get(), sum_ref.get(), sum_alt.get(), first.get());
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_db_narrow, dim3(db_grid(n_out)), dim3(DB_BLOCK), 0, c->stream, n_out, sum_ref.get(), sum_alt.get(), out->ref.get(),
                       out->alt.get(), first.get());
    HIPCHK(c, hipGetLastError());
    unsigned long long code = DB_NONE;
    HIPCHK(c, hipMemcpyAsync(&code, first, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (code != DB_NONE) {
        const uint64_t d = code >> 1;
        if (d >= n_out) return ctx_fail(c, CELLECTOR_EDEVICE, "add_doublets: the sum pass names entry %llu of %llu", (unsigned long long)d, (unsigned long long)n_out);
        uint32_t lc[2] = {0, 0};
        HIPCHK(c, hipMemcpyAsync(&lc[0], out->locus + d, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(&lc[1], out->cell + d, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        *overflow = true;
        *over_pair = (uint64_t)lc[1] - tc;
        *over_locus = lc[0];
        *over_allele = (int)(code & 1);
    }
    out->sorted = true;
    return CELLECTOR_OK;
}
