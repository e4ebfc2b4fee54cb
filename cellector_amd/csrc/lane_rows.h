// The lane-per-column geometry of the cell passes that score every row of a CSR against a handful of columns: the restarts' clusters
// (kernels_cluster.hip), the donors (kernels_donors.hip), the grid points of an ambient profile (kernels_ambient.hip) or of a donor
// pair's mixing share (kernels_pair_fraction.hip).  The shape is stated here once; those files say only what their columns and their
// table rows are.
//
// A group of P lanes (P = the power of two >= the columns, 64 / P rows per wave) owns one row, and a lane is one column: it owns the
// (row, column) sum and walks the row's entries in order, so every sum is strictly sequential (the bits depend on the matrix alone)
// and every entry costs the group one contiguous read of its columns.  The table loads of LANE_AHEAD entries are issued before the
// first of their ordered adds.  A term is a rounded product per allele and their rounded sum (-ffp-contract=off), then one add onto
// the sum; a masked locus adds nothing and is not counted.  Behind the walk comes a tail in which EVERY lane of the wave takes part in
// the shuffles, whatever its row and column: a lane without a row or a column walks nothing and carries a neutral value.
//
// The entry loop itself stays in each kernel (k_cluster_e, k_donor_e, k_donor_fit, k_ambient_e, k_pair_fraction_e, and over loci
// k_donor_match; each loop names the others): one loop behind a callable for the table lookup was measured and did not hold the speed of the separate
// loops in every pass.  What is shared is everything around it: the constants, the geometry, the argmax of the tails, and
// on the host the grid, the width, the width dispatch, the mask and the timing events.
//
// A block's waves take the groups g = wave0, wave0 + n_waves, ...; the grid is lane_grid(groups, LANE_WAVES, 8 per CU).
#pragma once
#include "ctx.h"

#include <type_traits>

#define LANE_THREADS 256
#define LANE_WAVES (LANE_THREADS / 64)
#define LANE_AHEAD 4  // entries whose loads are issued before the first of their ordered adds

// where this lane stands: row sub of the wave's RPW, column col (ok: below the columns in use), base = the group's first lane
template <int P>
struct LaneGeom {
    static constexpr int RPW = 64 / P;
    const int sub = (int)(threadIdx.x & 63) / P, col = (int)(threadIdx.x & 63) % P;
    const bool ok;
    const int base = sub * P;
    const uint64_t n_groups;
    const uint64_t wave0 = (uint64_t)blockIdx.x * LANE_WAVES + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * LANE_WAVES;
    __device__ LaneGeom(uint64_t n_rows, uint32_t cols) : ok((uint32_t)col < cols), n_groups((n_rows + RPW - 1) / RPW) {}
    __device__ uint64_t row(uint64_t g) const { return g * RPW + sub; }  // (may be past the last row: the caller's have)
};

// (value, index) maximum over the group's P lanes, the smallest index among equal values: every lane of the wave takes part
template <int P>
__device__ __forceinline__ void lane_argmax(double &v, int &idx)
{
#pragma unroll
    for (int off = P / 2; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off, 64);
        const int oi = __shfl_xor(idx, off, 64);
        if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// blocks for n items at per_block a block: at least one, at most cap
static inline unsigned lane_grid(uint64_t n, unsigned per_block, unsigned cap)
{
    uint64_t g = (n + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (unsigned)g;
}

// the power of two >= cols, at least min (a power of two)
static inline int lane_width(uint32_t cols, int min)
{
    int p = min;
    while ((uint32_t)p < cols) p <<= 1;
    return p;
}

// the grid of a walk over n_rows rows at width p
static inline unsigned lane_walk_grid(uint64_t n_rows, int p, int n_cu)
{
    return lane_grid((n_rows + 64 / p - 1) / (64 / p), LANE_WAVES, (unsigned)n_cu * 8);
}

// f(std::integral_constant<int, P>) for the run-time width p among the powers of two MIN ... MAX; nothing for any other p
template <int MIN, int MAX, typename F>
static inline void lane_dispatch(int p, F &&f)
{
    if (p == MIN) f(std::integral_constant<int, MIN>());
    else if constexpr (MIN < MAX) lane_dispatch<2 * MIN, MAX>(p, f);
}

// a call's loci mask on the device: get() is null while no mask is set, which is what the kernels take for "every locus"
struct LociMask {
    DevBuf<uint8_t> buf;  // [L]
    bool have = false;
    cellector_status set(cellector_ctx *c, const uint8_t *host_mask /*or null*/, uint64_t L)
    {
        have = host_mask != nullptr;
        if (have && L) HIPCHK(c, hipMemcpyAsync(buf, host_mask, L, hipMemcpyHostToDevice, c->stream));
        return CELLECTOR_OK;
    }
    const uint8_t *get() const { return have ? buf.get() : nullptr; }
};

// CELLECTOR_TIMING=1: N events recorded into a stream between its launches; ms(i, j) = the GPU time between two of them, read once
// the stream is idle.  Without the variable nothing is created or recorded.
template <int N>
struct EventMarks {
    const bool on = getenv("CELLECTOR_TIMING") != nullptr;
    hipEvent_t ev[N] = {};
    EventMarks() = default;
    EventMarks(const EventMarks &) = delete;
    ~EventMarks()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    void mark(int i, hipStream_t stream)
    {
        if (!on) return;
        if (!ev[i] && hipEventCreate(&ev[i]) != hipSuccess) return;
        (void)hipEventRecord(ev[i], stream);
    }
    bool ms(int i, int j, float *out) const { return ev[i] && ev[j] && hipEventElapsedTime(out, ev[i], ev[j]) == hipSuccess; }
};
