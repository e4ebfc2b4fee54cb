// C-ABI layer of libcellector_hip.so (include/cellector_ffi.h): argument checking, state machine,
// host<->device copies and the host-side scalar arithmetic of the scoring loop (threshold, priors).
// All matrix work is in the HIP kernels (kernels_*.hip); there is no CPU fallback.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include <algorithm>
#include <chrono>
#include <vector>
#include <unordered_map>
#include <mutex>
#include <system_error>
#include <thread>

#include "ctx.h"
#include "multi.h"
#include "ref_log.h"
#include "assign_host.h"
#include "genotype_host.h"

cellector_status ctx_fail(const cellector_ctx *c, cellector_status s, const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return s;
}

// ---- timing -----------------------------------------------------------------------------------------
void timer_begin(cellector_ctx *c, int which)
{
    if (!c->timing) return;
    // an event pair costs a few microseconds of idle queue (2 % of an iteration at 10^6 cells x 200k loci): level 2 keeps only the
    // pair the roofline figure needs, level 3 records that pair around every fourth launch only
    KernelTimer &t = c->timers[which];
    t.open = false;
    if (c->timing >= 2 && which != (c->engine == 2 ? CELLECTOR_K_TILE_LL : CELLECTOR_K_CELL_LL)) return;
    if (c->timing == 3 && (t.calls++ & 3u) != 0) return;
    hipEvent_t a = nullptr, b = nullptr;
    if (c->ev_pool.size() >= 2) {
        a = c->ev_pool.back(); c->ev_pool.pop_back();
        b = c->ev_pool.back(); c->ev_pool.pop_back();
    } else if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) {
        return;
    }
    t.start.push_back(a);
    t.stop.push_back(b);
    t.open = true;
    (void)hipEventRecord(a, c->stream);
}
// the event pair of a launch whose start and stop ride on the kernel's own dispatch (hipExtLaunchKernelGGL): no barrier packets
// in the queue, i.e. none of the idle time a recorded pair costs.  False: this launch is not timed.
bool timer_take(cellector_ctx *c, int which, hipEvent_t *a_out, hipEvent_t *b_out)
{
    if (!c->timing) return false;
    KernelTimer &t = c->timers[which];
    if (c->timing >= 2 && which != (c->engine == 2 ? CELLECTOR_K_TILE_LL : CELLECTOR_K_CELL_LL)) return false;
    if (c->timing == 3 && (t.calls++ & 3u) != 0) return false;
    hipEvent_t a = nullptr, b = nullptr;
    if (c->ev_pool.size() >= 2) {
        a = c->ev_pool.back(); c->ev_pool.pop_back();
        b = c->ev_pool.back(); c->ev_pool.pop_back();
    } else if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) {
        return false;
    }
    // (kept apart from the recorded pairs' open / close bookkeeping: both events belong to one dispatch)
    t.start.insert(t.start.begin(), a);
    t.stop.insert(t.stop.begin(), b);
    *a_out = a; *b_out = b;
    return true;
}
void timer_end(cellector_ctx *c, int which)
{
    KernelTimer &t = c->timers[which];
    if (!t.open || t.stop.empty()) return;  // (timer_begin recorded nothing for this launch)
    t.open = false;
    (void)hipEventRecord(t.stop.back(), c->stream);
}
void timer_collect(cellector_ctx *c)
{
    for (int k = 0; k < CELLECTOR_K_COUNT; k++) {
        KernelTimer &t = c->timers[k];
        // (a pair whose stop event is still to be recorded — the first half of a cell pass queued ahead by em_finish — stays)
        const size_t n_done = t.start.size() - (t.open && !t.start.empty() ? 1 : 0);
        for (size_t i = 0; i < n_done; i++) {
            float ms = 0.f;
            if (hipEventSynchronize(t.stop[i]) == hipSuccess &&
                hipEventElapsedTime(&ms, t.start[i], t.stop[i]) == hipSuccess) {
                t.total_ms += ms;
                t.launches++;
            } else {
                (void)hipGetLastError();  // (an event that was never recorded: not this call's caller's error)
            }
            c->ev_pool.push_back(t.start[i]);
            c->ev_pool.push_back(t.stop[i]);
        }
        t.start.erase(t.start.begin(), t.start.begin() + (long)n_done);
        t.stop.erase(t.stop.begin(), t.stop.begin() + (long)n_done);
    }
}

// A reload (and cellector_destroy) drops what was built and what was staged, each group as a whole (ctx.h).
static void drop_matrix(cellector_ctx *c)
{
    drop_built(c);
    static_cast<CtxStaged &>(*c) = CtxStaged();
}

// the side stream gets the lowest priority the device offers: its kernels should only fill slots the main stream's
// kernels leave idle
static bool create_side_stream(hipStream_t *out)
{
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) least = 0;
    return hipStreamCreateWithPriority(out, hipStreamNonBlocking, least) == hipSuccess;
}

// ---- caching layer under dev_alloc / DevBuf (see ctx.h) ---------------------------------------------------------
namespace {
struct DevBlock { void *p; size_t bytes; int device; };
std::mutex g_cache_mu;
std::vector<DevBlock> g_cache_free;                 // freed, still mapped
std::unordered_map<void *, DevBlock> g_cache_live;  // handed out by dev_cache_malloc
const size_t CACHE_MIN = 64ull << 20;               // smaller blocks go straight to the driver
}  // namespace

hipError_t dev_cache_malloc(void **p, size_t bytes)
{
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (bytes >= CACHE_MIN) {
        std::lock_guard<std::mutex> lk(g_cache_mu);
        size_t best = (size_t)-1;
        for (size_t i = 0; i < g_cache_free.size(); i++) {
            const DevBlock &b = g_cache_free[i];
            // fits, is at most twice the request, and is the tightest such block
            if (b.device == dev && b.bytes >= bytes && b.bytes - bytes <= bytes &&
                (best == (size_t)-1 || b.bytes < g_cache_free[best].bytes))
                best = i;
        }
        if (best != (size_t)-1) {
            DevBlock b = g_cache_free[best];
            g_cache_free.erase(g_cache_free.begin() + (long)best);
            g_cache_live[b.p] = b;
            *p = b.p;
            return hipSuccess;
        }
    }
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) {  // out of memory: give the cached blocks back and try once more
        (void)hipGetLastError();
        dev_cache_trim();
        e = hipMalloc(p, bytes);
    }
    if (e == hipSuccess && bytes >= CACHE_MIN) {
        std::lock_guard<std::mutex> lk(g_cache_mu);
        g_cache_live[*p] = DevBlock{*p, bytes, dev};
    }
    return e;
}

void dev_cache_free(void *p)
{
    if (!p) return;
    DevBlock blk{};
    bool cached = false;
    {
        std::lock_guard<std::mutex> lk(g_cache_mu);
        auto it = g_cache_live.find(p);
        if (it != g_cache_live.end()) {
            blk = it->second;
            g_cache_live.erase(it);
            cached = true;
        }
    }
    if (!cached) {
        (void)hipFree(p);
        return;
    }
    // hipFree would have waited for the block's device; a block handed out again must not still be in use either.  The wait is
    // for the BLOCK's device (a shard thread may free another shard's block) and happens outside the lock: other shards'
    // allocations do not queue behind it.
    int cur = 0;
    (void)hipGetDevice(&cur);
    if (cur != blk.device) (void)hipSetDevice(blk.device);
    (void)hipDeviceSynchronize();
    if (cur != blk.device) (void)hipSetDevice(cur);
    std::lock_guard<std::mutex> lk(g_cache_mu);
    g_cache_free.push_back(blk);
}

// a block nobody has used yet goes to the free list as it is (no device synchronisation needed)
void dev_cache_park(void *p, size_t bytes, int device)
{
    std::lock_guard<std::mutex> lk(g_cache_mu);
    g_cache_free.push_back(DevBlock{p, bytes, device});
}

void dev_cache_trim(int device)
{
    std::vector<DevBlock> blocks;
    {
        std::lock_guard<std::mutex> lk(g_cache_mu);
        if (device < 0) blocks.swap(g_cache_free);
        else {  // only this device's blocks: the other shards of a multi-device ctx may still be building from theirs
            std::vector<DevBlock> keep;
            for (const DevBlock &b : g_cache_free) (b.device == device ? blocks : keep).push_back(b);
            g_cache_free.swap(keep);
        }
    }
    int cur = 0;
    (void)hipGetDevice(&cur);
    for (const DevBlock &b : blocks) {
        (void)hipSetDevice(b.device);
        (void)hipFree(b.p);
    }
    (void)hipSetDevice(cur);
}

extern "C" {

const char *cellector_version(void) { return "cellector_amd 0.1 (gfx950)"; }

cellector_status cellector_create(cellector_ctx **out, int device_id)
{
    if (!out) return CELLECTOR_EINVAL;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device_id < 0 || device_id >= n) return CELLECTOR_EDEVICE;
    if (hipSetDevice(device_id) != hipSuccess) return CELLECTOR_EDEVICE;
    cellector_ctx *c = new (std::nothrow) cellector_ctx();
    if (!c) return CELLECTOR_ENOMEM;
    c->device = device_id;
    (void)hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, device_id);
    // ln(FCACHE[x]), x = 0..170: statrs' factorial cache, logs taken with the host libm like the reference
    double lf[LF_TABLE_N], f = 1.0;
    lf[0] = std::log(1.0);
    for (int i = 1; i < LF_TABLE_N; i++) {
        f *= (double)i;
        lf[i] = std::log(f);
    }
    bool ok = dev_alloc(c, &c->lf, LF_TABLE_N) == CELLECTOR_OK &&
              hipMemcpy(c->lf, lf, sizeof lf, hipMemcpyHostToDevice) == hipSuccess &&
              dev_alloc(c, &c->d_counters, 8) == CELLECTOR_OK &&
              dev_alloc(c, &c->sel_hist, CELLECTOR_SEL_HIST_WORDS) == CELLECTOR_OK &&
              hipMemset(c->sel_hist, 0, CELLECTOR_SEL_HIST_WORDS * sizeof(uint32_t)) == hipSuccess &&  // k_sel_finish re-zeroes
              dev_alloc(c, &c->sel_state, 4 * SEL_T) == CELLECTOR_OK &&
              dev_alloc(c, &c->sel_out, 16) == CELLECTOR_OK &&
              hipHostMalloc((void **)&c->h_sel, 32 * sizeof(double)) == hipSuccess &&
              (memset(c->h_sel, 0, 32 * sizeof(double)), true) &&
              hipHostGetDevicePointer((void **)&c->h_sum_dev, c->h_sel, 0) == hipSuccess &&
              dev_alloc(c, &c->t2_ctr, T2_CTR_N) == CELLECTOR_OK &&
              hipMemset(c->t2_ctr, 0, T2_CTR_N * sizeof(uint32_t)) == hipSuccess &&  // (the caching passes' counters start clear)
              create_side_stream(&c->side) &&
              create_side_stream(&c->side2) &&
              hipEventCreateWithFlags(&c->ev_t2tab, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&c->ev_help, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&c->ev_join2, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&c->ev_sum, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&c->ev_tab, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        cellector_destroy(c);
        return CELLECTOR_EDEVICE;
    }
    *out = c;
    return CELLECTOR_OK;
}

cellector_status cellector_device_count(int *out)
{
    if (!out) return CELLECTOR_EINVAL;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); n = 0; }
    *out = n;
    return CELLECTOR_OK;
}

cellector_status cellector_create_multi(cellector_ctx **out, const int *device_ids, int n_devices)
{
    if (!out || !device_ids || n_devices < 1 || n_devices > CELLECTOR_MAX_SHARDS) return CELLECTOR_EINVAL;
    *out = nullptr;
    if (n_devices == 1) return cellector_create(out, device_ids[0]);  // a plain single-shard ctx: nothing to exchange
    return multi_create(out, device_ids, n_devices);
}

cellector_status cellector_comm_unique_id(void *out_128_bytes)
{
    if (!out_128_bytes) return CELLECTOR_EINVAL;
    const char *why = nullptr;
    const int st = comm_rccl_unique_id(out_128_bytes, &why);
    if (st != CELLECTOR_OK) fprintf(stderr, "cellector_comm_unique_id: %s\n", why ? why : "RCCL error");
    return (cellector_status)st;
}

cellector_status cellector_comm_init_rank(cellector_ctx *c, const void *unique_id_128, int n_ranks, int rank)
{
    if (!c || !unique_id_128) return CELLECTOR_EINVAL;
    REQUIRE(c, !c->multi, "a multi-device ctx has its communicator already");
    REQUIRE(c, c->state == cellector_ctx::ST_EMPTY, "attach the communicator before the ingest");
    REQUIRE(c, !comm_active(c->comm), "ctx already has a communicator");
    REQUIRE(c, n_ranks >= 1 && rank >= 0 && rank < n_ranks, "bad rank / rank count");
    // (a one-rank communicator is made only on request: CELLECTOR_COMM_SELFTEST runs the RCCL calls of the sharded path on one GPU)
    if (n_ranks == 1 && !getenv("CELLECTOR_COMM_SELFTEST")) return CELLECTOR_OK;
    c->norm_zero = false;  // the NORM slices are all-gathered inside the library
    return (cellector_status)comm_rccl_init_rank(c, unique_id_128, n_ranks, rank);
}

void cellector_destroy(cellector_ctx *c)
{
    if (!c) return;
    if (c->multi) { multi_destroy(c); return; }
    (void)hipSetDevice(c->device);
    if (c->stream && c->owns_stream) (void)hipStreamSynchronize(c->stream);
    comm_destroy(c);
    if (c->side) (void)hipStreamSynchronize(c->side);
    if (c->side2) (void)hipStreamSynchronize(c->side2);
    timer_collect(c);
    for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
    c->ev_pool.clear();
    // (the device buffers go before the streams)
    drop_matrix(c);
    c->lf.reset(); c->d_counters.reset(); c->t2_ctr.reset(); c->sel_hist.reset(); c->sel_state.reset(); c->sel_out.reset();
    c->sel_list.reset(); c->seld_hist.reset(); c->seld_state.reset();
    c->res_cnt.reset(); c->res_dev.reset();
    if (c->h_sel) (void)hipHostFree(c->h_sel);
    if (c->side) (void)hipStreamDestroy(c->side);
    if (c->side2) (void)hipStreamDestroy(c->side2);
    if (c->stream && c->owns_stream) (void)hipStreamDestroy(c->stream);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->ev_join2) (void)hipEventDestroy(c->ev_join2);
    if (c->ev_sum) (void)hipEventDestroy(c->ev_sum);
    if (c->ev_tab) (void)hipEventDestroy(c->ev_tab);
    if (c->ev_t2tab) (void)hipEventDestroy(c->ev_t2tab);
    if (c->ev_help) (void)hipEventDestroy(c->ev_help);
    delete c;
    dev_cache_trim();
}

const char *cellector_last_error(const cellector_ctx *c) { return c ? c->err.c_str() : "null ctx"; }

cellector_status cellector_set_stream(cellector_ctx *c, void *s)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return ctx_fail(c, CELLECTOR_EINVAL, "a multi-device ctx runs every shard on a stream of its own");
    if (c->owns_stream) return ctx_fail(c, CELLECTOR_EINVAL, "this shard's stream belongs to its multi-device ctx");
    c->stream = (hipStream_t)s;
    return CELLECTOR_OK;
}

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

// The locus moments sum count planes over all cells: one device holding every cell.  (Summing the planes across shards needs an
// exchange the public LOCUS buffer has no room for.)
static cellector_status locus_moments_scope(const cellector_ctx *c, const char *what)
{
    if (c->multi) return ctx_fail(c, CELLECTOR_EINVAL, "%s works on a single-device ctx: the shards' count planes are not exchanged", what);
    if (comm_active(c->comm))
        return ctx_fail(c, CELLECTOR_EINVAL, "%s works on a ctx without a communicator: the shards' count planes are not exchanged", what);
    if (c->state == cellector_ctx::ST_READY ? c->nloc != c->total_cells : c->req_cell_begin != 0)
        return ctx_fail(c, CELLECTOR_EINVAL, "%s works on a ctx that holds all cells, not on a cellector_set_shard range: the shards' "
                                             "count planes are not exchanged", what);
    if (c->state == cellector_ctx::ST_READY && c->nnz >= (1ull << 32))  // (kernels_locus_moments.hip refuses the same: no counter may wrap)
        return ctx_fail(c, CELLECTOR_EINVAL, "%s: %llu entries, the locus histograms count in 32 bits (below 2^32 entries)", what,
                        (unsigned long long)c->nnz);
    return CELLECTOR_OK;
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
        if (v) CHK(locus_moments_scope(c, "locus_moments 1"));
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

// ---- ingest -------------------------------------------------------------------------------------------
static cellector_status begin_ingest(cellector_ctx *c, uint64_t total_loci, uint64_t total_cells)
{
    SETDEV(c);
    drop_matrix(c);  // (an ingest from outside: cellector_cell_origin is the identity again, cellector_cell_source all 0)
    // a caller-bound PASS1 buffer serves every matrix, with its whole capacity (n_pass1 is what the last one used of it)
    if (c->pass1_bound) { c->x_pass1 = c->pass1_bound; c->n_pass1 = c->pass1_bound_cap; }
    REQUIRE(c, total_loci <= 0xffffffffull && total_cells <= 0xffffffffull, "dims exceed 32-bit indices");
    c->total_loci = total_loci;
    c->total_cells = total_cells;
    if (c->ingest_all_cells) {
        c->cell_begin = 0;
        c->cell_end = total_cells;
    } else if (comm_active(c->comm)) {  // rank r owns the r-th contiguous range: equal ranges, or the partition it was given
        if (c->comm.has_bounds && c->comm.bounds[c->comm.n] != total_cells)
            return ctx_fail(c, CELLECTOR_EINVAL, "the partition covers %llu cells, the matrix has %llu",
                            (unsigned long long)c->comm.bounds[c->comm.n], (unsigned long long)total_cells);
        comm_range(c->comm, total_cells, c->comm.rank, &c->cell_begin, &c->cell_end);
    } else {
        c->cell_begin = c->req_cell_begin;
        c->cell_end = c->req_cell_end;
    }
    if (c->cell_end > total_cells) c->cell_end = total_cells;
    if (c->cell_begin > c->cell_end) c->cell_begin = c->cell_end;
    c->nloc = c->cell_end - c->cell_begin;
    const uint64_t need = (uint64_t)P1_PLANES * total_loci;
    if (c->x_pass1) {
        REQUIRE(c, c->n_pass1 >= need, "bound PASS1 exchange buffer too small");
    } else {
        CHK(dev_alloc(c, &c->x_pass1_own, need));
        c->x_pass1 = c->x_pass1_own;
    }
    c->n_pass1 = need;
    return CELLECTOR_OK;
}

cellector_status cellector_ingest_coo(cellector_ctx *c, uint64_t total_loci, uint64_t total_cells, uint64_t nnz,
                                      const uint32_t *locus0, const uint32_t *cell0, const uint32_t *alt,
                                      const uint32_t *ref)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return multi_ingest_coo(c, total_loci, total_cells, nnz, locus0, cell0, alt, ref);
    REQUIRE(c, nnz == 0 || (locus0 && cell0 && alt && ref), "null COO array");
    CHK(begin_ingest(c, total_loci, total_cells));
    CHK(ingest_stage_host_coo(c, nnz, locus0, cell0, alt, ref));
    CHK(ingest_pass1(c));
    c->state = cellector_ctx::ST_STAGED;
    return CELLECTOR_OK;
}

cellector_status cellector_ingest_mtx(cellector_ctx *c, const char *alt_path, const char *ref_path)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return multi_ingest_mtx(c, alt_path, ref_path);
    REQUIRE(c, alt_path && ref_path, "null path");
    const bool timing = getenv("CELLECTOR_TIMING") != nullptr && c->comm.rank == 0;
    LapTimer t;
    MtxInput *in = nullptr;
    uint64_t tl = 0, tc = 0;
    CHK(ctx_mtx_open(c, alt_path, ref_path, &in, &tl, &tc, true));
    if (timing) fprintf(stderr, "[timing]   open / inflate          %8.3f s\n", t.lap());
    cellector_status s = begin_ingest(c, tl, tc);
    if (s == CELLECTOR_OK) s = ingest_stage_mtx_device(c, in);  // tokenised and converted on the GPU
    mtx_input_close(in);
    CHK(s);
    if (timing) fprintf(stderr, "[timing]   upload + device parse   %8.3f s\n", t.lap());
    CHK(ingest_pass1(c));
    c->state = cellector_ctx::ST_STAGED;
    return CELLECTOR_OK;
}

}  // extern "C"

// ---- the joined ingests: two count streams keyed by (locus, cell) (kernels_join.hip) ------------------------------------------------
// why a ctx cannot take a joined ingest, or null: the scope of cellector_restage, before anything is staged
static const char *join_scope(const cellector_ctx *c, uint64_t total_cells)
{
    if (c->multi) return "is a multi-device ctx: its staged entries are sharded";
    if (comm_active(c->comm)) return "has a communicator: every rank stages its own cells";
    if (c->req_cell_begin != 0 || c->req_cell_end < total_cells) return "holds a cellector_set_shard range, not all cells";
    return nullptr;
}
static cellector_status join_mode_check(const cellector_ctx *c, int mode)
{
    if (mode != CELLECTOR_JOIN_REF && mode != CELLECTOR_JOIN_DEPTH)
        return ctx_fail(c, CELLECTOR_EINVAL, "join: mode must be CELLECTOR_JOIN_REF (1) or CELLECTOR_JOIN_DEPTH (2)");
    return CELLECTOR_OK;
}
// tokens -> staged COO -> PASS1; the ctx has been through begin_ingest
static cellector_status join_finish_stage(cellector_ctx *c, JoinTokens *first, JoinTokens *second, uint32_t index_base, int mode,
                                          cellector_join_summary *out, JoinPhases *ph)
{
    StagedCoo coo;
    CHK(join_stage(c, first, second, index_base, mode, &coo, out, ph));
    c->coo = std::move(coo);
    CHK(ingest_pass1(c));
    c->state = cellector_ctx::ST_STAGED;
    if (getenv("CELLECTOR_TIMING"))
        fprintf(stderr, "[timing]   join: tokens FIRST %.4f s, tokens SECOND %.4f s, checks %.4f s, sorts %.4f s, join %.4f s (its kernels %.3f ms)\n",
                ph->tokens_first, ph->tokens_second, ph->checks, ph->sorts, ph->join, ph->join_kernels_ms);
    return CELLECTOR_OK;
}

extern "C" {

cellector_status cellector_ingest_mtx_joined(cellector_ctx *c, const char *first_path, const char *second_path, int mode,
                                             cellector_join_summary *out)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return ctx_fail(c, CELLECTOR_EINVAL, "ingest_mtx_joined: ctx %s", join_scope(c, 0));
    REQUIRE(c, first_path && second_path, "null path");
    CHK(join_mode_check(c, mode));
    MtxInput *in = nullptr;
    uint64_t tl = 0, tc = 0, first_hint = 0;
    CHK(ctx_mtx_open(c, first_path, second_path, &in, &tl, &tc, true));
    struct Closer { MtxInput *in; ~Closer() { mtx_input_close(in); } } closer{in};
    CHK(join_size_lines(c, in, &first_hint));
    if (const char *why = join_scope(c, tc)) return ctx_fail(c, CELLECTOR_EINVAL, "ingest_mtx_joined: ctx %s", why);
    // ---- validated: from here the ctx changes as in cellector_ingest_mtx
    CHK(begin_ingest(c, tl, tc));
    JoinTokens first, second;
    JoinPhases ph;
    CHK(join_parse_pair(c, in, first_hint, &first, &second, &ph));
    return join_finish_stage(c, &first, &second, 1u, mode, out, &ph);
}

cellector_status cellector_ingest_coo_joined(cellector_ctx *c, uint64_t total_loci, uint64_t total_cells, uint64_t n_first,
                                             const uint32_t *locus0_a, const uint32_t *cell0_a, const uint32_t *count_a, uint64_t n_second,
                                             const uint32_t *locus0_b, const uint32_t *cell0_b, const uint32_t *count_b, int mode,
                                             cellector_join_summary *out)
{
    if (!c) return CELLECTOR_EINVAL;
    if (const char *why = join_scope(c, total_cells)) return ctx_fail(c, CELLECTOR_EINVAL, "ingest_coo_joined: ctx %s", why);
    REQUIRE(c, n_first == 0 || (locus0_a && cell0_a && count_a), "null COO array");
    REQUIRE(c, n_second == 0 || (locus0_b && cell0_b && count_b), "null COO array");
    CHK(join_mode_check(c, mode));
    CHK(begin_ingest(c, total_loci, total_cells));
    JoinTokens side[2];
    JoinPhases ph;
    LapTimer t;
    const uint64_t n[2] = {n_first, n_second};
    const uint32_t *src[2][3] = {{locus0_a, cell0_a, count_a}, {locus0_b, cell0_b, count_b}};
    for (int s = 0; s < 2; s++) {
        DevBuf<uint32_t> *dst[3] = {&side[s].locus, &side[s].cell, &side[s].count};
        side[s].n = n[s];
        for (int k = 0; k < 3; k++) {
            CHK(dev_alloc(c, dst[k], n[s]));
            if (n[s]) HIPCHK(c, hipMemcpyAsync(dst[k]->get(), src[s][k], n[s] * 4, hipMemcpyHostToDevice, c->stream));
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
        (s ? ph.tokens_second : ph.tokens_first) = t.lap();
    }
    return join_finish_stage(c, &side[0], &side[1], 0u, mode, out, &ph);
}

cellector_status cellector_load_mtx_joined(cellector_ctx *c, const char *first_path, const char *second_path, int mode, uint64_t min_alt,
                                           uint64_t min_ref, cellector_join_summary *out)
{
    CHK(cellector_ingest_mtx_joined(c, first_path, second_path, mode, out));
    return cellector_ingest_finish(c, min_alt, min_ref);
}

}  // extern "C"

// Multi-device text ingest, step 1: shard `c` tokenises the whole pair and stages the entries of ALL cells (global cell index).
cellector_status ffi_stage_mtx_all_cells(cellector_ctx *c, const char *alt_path, const char *ref_path, cellector_ctx *helper)
{
    REQUIRE(c, alt_path && ref_path, "null path");
    MtxInput *in = nullptr;
    uint64_t tl = 0, tc = 0;
    CHK(ctx_mtx_open(c, alt_path, ref_path, &in, &tl, &tc));
    c->ingest_all_cells = true;
    cellector_status s = begin_ingest(c, tl, tc);
    if (s == CELLECTOR_OK) s = ingest_stage_mtx_device(c, in, helper);
    c->ingest_all_cells = false;
    mtx_input_close(in);
    return s;
}
// ... step 2: a shard takes over its routed entries (arrays on its own device, cell index local, file order) as its staged COO.
cellector_status ffi_adopt_staged(cellector_ctx *c, uint64_t total_loci, uint64_t total_cells, StagedCoo &&coo)
{
    CHK(begin_ingest(c, total_loci, total_cells));
    c->coo = std::move(coo);
    CHK(ingest_pass1(c));
    c->state = cellector_ctx::ST_STAGED;
    return CELLECTOR_OK;
}

// The EM state a load leaves, queued on the stream: all loci used, no cell excluded, the outputs zero (cellector_ingest_finish,
// cellector_em_reset)
static cellector_status em_state_clear(cellector_ctx *c)
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

extern "C" {

cellector_status cellector_ingest_synthetic(cellector_ctx *c, uint64_t total_loci, uint64_t total_cells,
                                            double density, uint64_t seed, double minority_fraction,
                                            double doublet_fraction)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return multi_ingest_synthetic(c, total_loci, total_cells, density, seed, minority_fraction, doublet_fraction);
    CHK(begin_ingest(c, total_loci, total_cells));
    CHK(synth_generate(c, density, seed, minority_fraction, doublet_fraction));
    CHK(ingest_pass1(c));
    c->state = cellector_ctx::ST_STAGED;
    return CELLECTOR_OK;
}

cellector_status cellector_write_staged_mtx(cellector_ctx *c, const char *alt_path, const char *ref_path)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return ctx_fail(c, CELLECTOR_EINVAL, "write_staged_mtx works on a single-device ctx (the staged entries of a multi-device ctx are sharded)");
    REQUIRE(c, alt_path && ref_path, "null path");
    REQUIRE(c, c->state != cellector_ctx::ST_EMPTY, "write_staged_mtx without a staged matrix");
    SETDEV(c);
    return synth_write_mtx(c, alt_path, ref_path);
}

cellector_status cellector_ingest_finish(cellector_ctx *c, uint64_t min_alt, uint64_t min_ref)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return multi_ingest_finish(c, min_alt, min_ref);
    REQUIRE(c, c->state == cellector_ctx::ST_STAGED, "ingest_finish without a staged matrix");
    SETDEV(c);
    const bool timing = getenv("CELLECTOR_TIMING") != nullptr && c->comm.rank == 0;
    LapTimer t;
    if (comm_active(c->comm)) {  // exchange point 1: global pass-1 counts and allele totals (every shard applies the same locus filter)
        CHK((cellector_status)comm_allreduce_sum(c, c->x_pass1, (uint64_t)P1_PLANES * c->total_loci));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    CHK(ingest_build(c, min_alt, min_ref));
    if (timing) fprintf(stderr, "[timing]   CSC / CSR build         %8.3f s\n", t.lap());
    const uint64_t L = c->L, n = c->nloc;
    CHK(dev_alloc(c, &c->ab, L)); CHK(dev_alloc(c, &c->ab6, 8 * L));
    CHK(dev_alloc(c, &c->mask, L)); CHK(dev_alloc(c, &c->mask_next, L));
    CHK(dev_alloc(c, &c->flags, n)); CHK(dev_alloc(c, &c->flags_new, n));
    CHK(dev_alloc(c, &c->ll, n)); CHK(dev_alloc(c, &c->ell, n)); CHK(dev_alloc(c, &c->nloci, n));
    CHK(dev_alloc(c, &c->post, 4 * n));
    // (with a communicator every rank owns an equal slot of NORM: the in-place all-gather's layout)
    const uint64_t need_norm = comm_active(c->comm) ? comm_cells_per_rank(c->total_cells, c->comm.n) * (uint64_t)c->comm.n : c->total_cells;
    const uint64_t need_locus = (uint64_t)LB_PLANES * L + LC_COUNTERS;
    if (c->x_norm) REQUIRE(c, c->n_norm >= need_norm, "bound NORM exchange buffer too small");
    else { CHK(dev_alloc(c, &c->x_norm_own, need_norm)); c->x_norm = c->x_norm_own; }
    if (c->x_locus) REQUIRE(c, c->n_locus >= need_locus, "bound LOCUS exchange buffer too small");
    else { CHK(dev_alloc(c, &c->x_locus_own, need_locus)); c->x_locus = c->x_locus_own; }
    c->n_norm = need_norm;
    c->n_locus = need_locus;
    CHK(em_state_clear(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    {
        // The near-tie band of cellector_iter_summary.n_near_threshold follows the matrix' depth: the reference's ln_gamma
        // differences (stats.rs:41-53) carry ~eps * lnGamma(alpha + beta) of cancellation error per term, which the device's
        // product form does not reproduce — 1e-11 on a normalised LL at alpha + beta ~ 1e4 (vartrix-like depth), 1e-8 at 1e6.
        // band = max(1e-9, 8 eps lnGamma(max over the used loci of S_alt + S_ref + 2)), relative to max(1, |threshold|);
        // the global totals are the same on every shard.
        std::vector<double> sa(L), sr(L);
        if (L) {
            HIPCHK(c, hipMemcpy(sa.data(), c->s_alt, L * 8, hipMemcpyDeviceToHost));
            HIPCHK(c, hipMemcpy(sr.data(), c->s_ref, L * 8, hipMemcpyDeviceToHost));
        }
        double max_ab = 2.0;
        for (uint64_t l = 0; l < L; l++) max_ab = std::max(max_ab, sa[l] + sr[l] + 2.0);
        c->near_rel = std::max(CELLECTOR_NEAR_TIE_REL, 8.0 * 2.220446049250313e-16 * lgamma(max_ab));
    }
    if (c->engine == 2) {
        CHK(tiled_build(c));
        // the packed by-locus CSC (8 B per entry: 16 GB at 2e9 entries) is only streamed by engine 1; engine 2 has built
        // its compact CSC and overflow CSC from it.  Engine 1 must therefore be chosen BEFORE the ingest.
        c->csc_ent.reset();
    }
    if (timing) fprintf(stderr, "[timing]   tiled layouts           %8.3f s\n", t.lap());
    dev_cache_trim(c->device);  // the ingest's big temporaries are done: hand this device's cached blocks back
    c->state = cellector_ctx::ST_READY;
    c->em_phase = 0; c->iteration = 0; c->have_iter = false; c->n_excluded_global = 0;
    return CELLECTOR_OK;
}

cellector_status cellector_load_mtx(cellector_ctx *c, const char *a, const char *r, uint64_t min_alt, uint64_t min_ref)
{
    CHK(cellector_ingest_mtx(c, a, r));
    return cellector_ingest_finish(c, min_alt, min_ref);
}

cellector_status cellector_load_coo(cellector_ctx *c, uint64_t tl, uint64_t tc, uint64_t nnz, const uint32_t *l,
                                    const uint32_t *ce, const uint32_t *a, const uint32_t *r, uint64_t min_alt,
                                    uint64_t min_ref)
{
    CHK(cellector_ingest_coo(c, tl, tc, nnz, l, ce, a, r));
    return cellector_ingest_finish(c, min_alt, min_ref);
}

// ---- accessors ----------------------------------------------------------------------------------------
cellector_status cellector_dims(const cellector_ctx *c, cellector_dims_t *o)
{
    if (!c || !o) return CELLECTOR_EINVAL;
    if (c->multi) return multi_dims(c, o);
    o->total_cells = c->total_cells; o->total_loci = c->total_loci; o->loci_used = c->L;
    o->cell_begin = c->cell_begin; o->cell_end = c->cell_end; o->nnz_used = c->nnz;
    return CELLECTOR_OK;
}

#define READY(c) REQUIRE(c, (c) && (c)->state == cellector_ctx::ST_READY, "no matrix loaded")
// per-locus state is replicated on every shard: shard 0 of a multi-device ctx answers
#define SHARD0(c, call)                                                      \
    do {                                                                     \
        if ((c)->multi) {                                                    \
            const cellector_ctx *s0__ = multi_shard0(c);                     \
            const cellector_status st__ = (call);                            \
            if (st__ != CELLECTOR_OK) (c)->err = s0__->err;                  \
            return st__;                                                     \
        }                                                                    \
    } while (0)

cellector_status cellector_locus_ids(const cellector_ctx *c, uint64_t *out)
{
    if (!c) return CELLECTOR_EINVAL;
    SHARD0(c, cellector_locus_ids(s0__, out));
    READY(c);
    return d2h(c, out, c->locus_ids, c->L * 8);
}

cellector_status cellector_locus_counts(const cellector_ctx *c, double *out)
{
    if (!c) return CELLECTOR_EINVAL;
    SHARD0(c, cellector_locus_counts(s0__, out));
    READY(c);
    std::vector<double> a(c->L), r(c->L);
    CHK(d2h(c, a.data(), c->s_alt, c->L * 8));
    CHK(d2h(c, r.data(), c->s_ref, c->L * 8));
    for (uint64_t l = 0; l < c->L; l++) { out[2 * l] = r[l]; out[2 * l + 1] = a[l]; }
    return CELLECTOR_OK;
}

cellector_status cellector_entries_per_cell(const cellector_ctx *c, uint32_t *out)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return multi_entries_per_cell(c, out);
    READY(c);
    std::vector<uint64_t> p(c->nloc + 1);
    CHK(d2h(c, p.data(), c->csr_ptr, (c->nloc + 1) * 8));
    for (uint64_t i = 0; i < c->nloc; i++) out[i] = (uint32_t)(p[i + 1] - p[i]);
    return CELLECTOR_OK;
}

cellector_status cellector_csr_rows(const cellector_ctx *c, uint64_t rb, uint64_t re, uint64_t *row_ptr,
                                    uint64_t *entries, uint64_t capacity)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return multi_csr_rows(c, rb, re, row_ptr, entries, capacity);
    READY(c);
    REQUIRE(c, rb <= re && re <= c->nloc && row_ptr, "bad row range");
    CHK(d2h(c, row_ptr, c->csr_ptr + rb, (re - rb + 1) * 8));
    const uint64_t base = row_ptr[0], cnt = row_ptr[re - rb] - base;
    for (uint64_t i = 0; i <= re - rb; i++) row_ptr[i] -= base;
    if (entries) {
        REQUIRE(c, capacity >= cnt, "entries capacity too small");
        CHK(d2h(c, entries, c->csr_ent + base, cnt * 8));
    }
    return CELLECTOR_OK;
}

// ---- exchange buffers ---------------------------------------------------------------------------------
cellector_status cellector_exchange_buffer(cellector_ctx *c, cellector_xchg which, void **dev_ptr, uint64_t *n)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return ctx_fail(c, CELLECTOR_EINVAL, "the exchange buffers of a multi-device ctx are internal");
    double *p = nullptr;
    uint64_t cnt = 0;
    switch (which) {
    case CELLECTOR_XCHG_PASS1: p = c->x_pass1; cnt = c->n_pass1; break;
    case CELLECTOR_XCHG_NORM:
        p = c->x_norm; cnt = c->state == cellector_ctx::ST_READY ? c->total_cells : c->n_norm; break;
    case CELLECTOR_XCHG_LOCUS:
        p = c->x_locus;
        cnt = c->state == cellector_ctx::ST_READY ? (uint64_t)LB_PLANES * c->L + LC_COUNTERS : c->n_locus; break;
    default: return ctx_fail(c, CELLECTOR_EINVAL, "unknown exchange buffer");
    }
    if (dev_ptr) *dev_ptr = p;
    if (n) *n = cnt;
    return CELLECTOR_OK;
}

cellector_status cellector_bind_exchange_buffer(cellector_ctx *c, cellector_xchg which, void *dev_ptr, uint64_t n)
{
    if (!c || !dev_ptr) return CELLECTOR_EINVAL;
    if (c->multi || comm_active(c->comm)) return ctx_fail(c, CELLECTOR_EINVAL, "a ctx with a communicator owns its exchange buffers");
    double *p = (double *)dev_ptr;
    c->tables_prebuilt = false;  // (tables built ahead read the old buffers)
    switch (which) {
    case CELLECTOR_XCHG_PASS1:
        REQUIRE(c, c->state == cellector_ctx::ST_EMPTY, "bind PASS1 before ingest");
        c->x_pass1_own.reset();
        c->x_pass1 = c->pass1_bound = p; c->n_pass1 = c->pass1_bound_cap = n;
        break;
    case CELLECTOR_XCHG_NORM:
        REQUIRE(c, c->state != cellector_ctx::ST_READY || n >= c->total_cells, "NORM buffer too small");
        c->x_norm_own.reset();
        c->x_norm = p; c->n_norm = n;
        break;
    case CELLECTOR_XCHG_LOCUS:
        REQUIRE(c, c->state != cellector_ctx::ST_READY || n >= (uint64_t)LB_PLANES * c->L + LC_COUNTERS,
                "LOCUS buffer too small");
        if (c->state == cellector_ctx::ST_READY) {
            // carry the current tallies over (they seed the next alpha/beta update)
            HIPCHK(c, hipMemcpyAsync(p, c->x_locus, ((uint64_t)LB_PLANES * c->L + LC_COUNTERS) * 8,
                                     hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        c->x_locus_own.reset();
        c->x_locus = p; c->n_locus = n;
        break;
    default: return ctx_fail(c, CELLECTOR_EINVAL, "unknown exchange buffer");
    }
    return CELLECTOR_OK;
}

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
    if (c->locus_moments) CHK(locus_moments_scope(c, "locus_moments 1"));  // (before anything of this phase is queued)
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
    CHK(locus_moments_scope(c, "locus_moments"));
    READY(c);
    REQUIRE(c, c->em_phase == 0, "locus_moments: iteration in flight (finish it with cellector_em_finish)");
    REQUIRE(c, (alpha && beta) || c->L == 0, "locus_moments: null alpha/beta");
    REQUIRE(c, flags || c->nloc == 0, "locus_moments: null flags");
    SETDEV(c);
    return locus_moments_run(c, alpha, beta, mask, flags, exp_min, exp_maj, var_min, var_maj);
}

cellector_status cellector_locus_total_counts(cellector_ctx *c, const uint8_t *flags, uint32_t *out)
{
    if (!c) return CELLECTOR_EINVAL;
    CHK(locus_moments_scope(c, "locus_total_counts"));
    READY(c);
    REQUIRE(c, c->em_phase == 0, "locus_total_counts: iteration in flight (finish it with cellector_em_finish)");
    REQUIRE(c, out || c->L == 0, "locus_total_counts: null output");
    SETDEV(c);
    return locus_total_counts_run(c, flags, out);
}

cellector_status cellector_iter_locus_moments(const cellector_ctx *c, double *exp_min, double *exp_maj, double *var_min, double *var_maj)
{
    if (!c) return CELLECTOR_EINVAL;
    CHK(locus_moments_scope(c, "iter_locus_moments"));
    READY(c);
    REQUIRE(c, c->em_phase == 0, "iter_locus_moments: iteration in flight (finish it with cellector_em_finish)");
    REQUIRE(c, c->lm_formed, "iter_locus_moments: not formed (the last finished iteration ran with option locus_moments 0, or none "
                             "has finished since the load / cellector_em_reset)");
    const uint64_t L = c->L;
    double *const out[4] = {exp_min, exp_maj, var_min, var_maj};
    for (int k = 0; k < 4; k++)
        if (out[k] && L) CHK(d2h(c, out[k], c->lm_out + (uint64_t)k * L, L * 8));
    return CELLECTOR_OK;
}

// ---- K-genotype classes: kernels_classes.hip ------------------------------------------------------------
// what every class call checks before anything is written or launched
static cellector_status class_call_check(cellector_ctx *c, const char *what, const uint8_t *labels, uint32_t K, const double *scale,
                                         const double *log_prior)
{
    CHK(locus_moments_scope(c, what));
    READY(c);
    if (c->em_phase != 0) return ctx_fail(c, CELLECTOR_EINVAL, "%s: iteration in flight (finish it with cellector_em_finish)", what);
    if (!labels) return ctx_fail(c, CELLECTOR_EINVAL, "%s: null labels", what);
    if (K < 1 || K > 16) return ctx_fail(c, CELLECTOR_EINVAL, "%s: %u classes, 1..16 are supported", what, K);
    bool any = false;
    for (uint64_t i = 0; i < c->nloc; i++) {
        if (labels[i] >= K && labels[i] != 255)
            return ctx_fail(c, CELLECTOR_EINVAL, "%s: cell %llu has label %u, neither below the %u classes nor 255 (unlabelled)", what,
                            (unsigned long long)i, (unsigned)labels[i], K);
        any = any || labels[i] != 255;
    }
    if (!any) return ctx_fail(c, CELLECTOR_EINVAL, "%s: every cell is unlabelled: all %u classes are dead", what, K);
    for (uint32_t k = 0; scale && k < K; k++)
        if (!std::isfinite(scale[k]) || scale[k] < 0.0)
            return ctx_fail(c, CELLECTOR_EINVAL, "%s: scale[%u] = %g is not a finite value >= 0", what, k, scale[k]);
    for (uint32_t k = 0; log_prior && k < K; k++)
        if (std::isnan(log_prior[k])) return ctx_fail(c, CELLECTOR_EINVAL, "%s: log_prior[%u] is NaN", what, k);
    return CELLECTOR_OK;
}

// step 1 of the class model: the exact integer tallies of a labelling (main.rs:598-611 sums the same counts for two classes)
cellector_status cellector_class_tallies(cellector_ctx *c, const uint8_t *labels, uint32_t n_classes, uint64_t *cells, uint64_t *alt,
                                         uint64_t *ref)
{
    if (!c) return CELLECTOR_EINVAL;
    CHK(class_call_check(c, "class_tallies", labels, n_classes, nullptr, nullptr));
    SETDEV(c);
    return classes_tallies_run(c, labels, n_classes, nullptr, cells, alt, ref, nullptr, nullptr);
}

// step 2: init_alpha_betas (main.rs:598-611) for K classes
cellector_status cellector_class_alpha_betas(cellector_ctx *c, const uint8_t *labels, uint32_t n_classes, const double *scale, double *alpha,
                                             double *beta)
{
    if (!c) return CELLECTOR_EINVAL;
    CHK(class_call_check(c, "class_alpha_betas", labels, n_classes, scale, nullptr));
    SETDEV(c);
    return classes_tallies_run(c, labels, n_classes, scale, nullptr, nullptr, nullptr, alpha, beta);
}

// steps 1-6: get_cell_log_likelihoods (main.rs:541-591) per class and the prior / logsumexp chain of main.rs:264-276 over K terms
cellector_status cellector_class_posteriors(cellector_ctx *c, const uint8_t *labels, uint32_t n_classes, const double *scale,
                                            const double *log_prior, const uint8_t *mask, double *ll, double *posterior, uint8_t *best,
                                            uint64_t *qual)
{
    if (!c) return CELLECTOR_EINVAL;
    CHK(class_call_check(c, "class_posteriors", labels, n_classes, scale, log_prior));
    SETDEV(c);
    const cellector_status st = classes_run(c, labels, n_classes, scale, log_prior, mask, 0, 1, nullptr, nullptr, ll, posterior, best, qual);
    if (c->timing) timer_collect(c);
    return st;
}

// step 7: the hard-EM loop over steps 1-6 (the outer loop of main.rs:42-46, with K classes in place of the exclusion set)
cellector_status cellector_refine_classes(cellector_ctx *c, uint8_t *labels, uint32_t n_classes, const double *scale, const double *log_prior,
                                          const uint8_t *mask, uint32_t max_iter, uint64_t min_loci, cellector_refine_summary *out, double *ll,
                                          double *posterior, uint64_t *qual)
{
    if (!c) return CELLECTOR_EINVAL;
    CHK(class_call_check(c, "refine_classes", labels, n_classes, scale, log_prior));
    REQUIRE(c, min_loci >= 1, "refine_classes: min_loci must be at least 1");
    SETDEV(c);
    const cellector_status st = classes_run(c, labels, n_classes, scale, log_prior, mask, max_iter, min_loci, labels, out, ll, posterior,
                                            nullptr, qual);
    if (c->timing) timer_collect(c);
    return st;
}

// ---- doublet classes over the K classes: the second half of kernels_classes.hip ------------------------------
// what the doublet calls check on top of class_call_check: a live class must remain once the held cells are out
static cellector_status doublet_call_check(cellector_ctx *c, const char *what, const uint8_t *labels, const uint8_t *held, uint32_t K,
                                           const double *scale, const double *pair_scale, const double *log_prior,
                                           const double *log_pair_prior)
{
    CHK(class_call_check(c, what, labels, K, scale, log_prior));
    bool any = !held;
    for (uint64_t i = 0; held && !any && i < c->nloc; i++) any = labels[i] != 255 && !held[i];
    if (!any) return ctx_fail(c, CELLECTOR_EINVAL, "%s: every labelled cell is held: all %u classes are dead", what, K);
    for (uint32_t k = 0; pair_scale && k < K; k++)
        if (!std::isfinite(pair_scale[k]) || pair_scale[k] < 0.0)
            return ctx_fail(c, CELLECTOR_EINVAL, "%s: pair_scale[%u] = %g is not a finite value >= 0", what, k, pair_scale[k]);
    for (uint32_t p = 0; log_pair_prior && p < K * (K - 1) / 2; p++)
        if (std::isnan(log_pair_prior[p])) return ctx_fail(c, CELLECTOR_EINVAL, "%s: log_pair_prior[%u] is NaN", what, p);
    return CELLECTOR_OK;
}

// step 3 of the doublet model: the P pair distributions (main.rs:245-246 for K = 2)
cellector_status cellector_class_pair_alpha_betas(cellector_ctx *c, const uint8_t *labels, const uint8_t *held, uint32_t n_classes,
                                                  const double *pair_scale, double *alpha, double *beta)
{
    if (!c) return CELLECTOR_EINVAL;
    CHK(doublet_call_check(c, "class_pair_alpha_betas", labels, held, n_classes, nullptr, pair_scale, nullptr, nullptr));
    SETDEV(c);
    return class_pairs_run(c, labels, held, n_classes, pair_scale, alpha, beta);
}

// steps 1-6: the K singlets and the P pairs in one chain (calculate_posteriors, main.rs:228-280, is K = 2), and the call of
// main.rs:150
cellector_status cellector_class_doublets(cellector_ctx *c, const uint8_t *labels, const uint8_t *held, uint32_t n_classes,
                                          const double *scale, const double *pair_scale, const double *log_prior,
                                          const double *log_pair_prior, const uint8_t *mask, double *ll, double *ll_pair, double *posterior,
                                          double *doublet_posterior, uint8_t *best, uint8_t *best_pair, uint8_t *call, uint64_t *qual)
{
    if (!c) return CELLECTOR_EINVAL;
    CHK(doublet_call_check(c, "class_doublets", labels, held, n_classes, scale, pair_scale, log_prior, log_pair_prior));
    SETDEV(c);
    const cellector_status st = class_doublets_run(c, labels, held, n_classes, scale, pair_scale, log_prior, log_pair_prior, mask, 0.5, 0, 1,
                                                   nullptr, nullptr, nullptr, ll, ll_pair, posterior, doublet_posterior, best, best_pair, call,
                                                   qual);
    if (c->timing) timer_collect(c);
    return st;
}

// step 7: the held-out refine
cellector_status cellector_refine_class_doublets(cellector_ctx *c, uint8_t *labels, uint8_t *held, uint32_t n_classes, const double *scale,
                                                 const double *pair_scale, const double *log_prior, const double *log_pair_prior,
                                                 const uint8_t *mask, double doublet_threshold, uint32_t max_iter, uint64_t min_loci,
                                                 cellector_refine_doublets_summary *out, double *ll, double *ll_pair, double *posterior,
                                                 double *doublet_posterior, uint8_t *best_pair, uint64_t *qual)
{
    if (!c) return CELLECTOR_EINVAL;
    CHK(doublet_call_check(c, "refine_class_doublets", labels, held, n_classes, scale, pair_scale, log_prior, log_pair_prior));
    REQUIRE(c, min_loci >= 1, "refine_class_doublets: min_loci must be at least 1");
    if (!(doublet_threshold >= 0.0 && doublet_threshold <= 1.0))
        return ctx_fail(c, CELLECTOR_EINVAL, "refine_class_doublets: doublet_threshold = %g is not within [0, 1]", doublet_threshold);
    SETDEV(c);
    const cellector_status st = class_doublets_run(c, labels, held, n_classes, scale, pair_scale, log_prior, log_pair_prior, mask,
                                                   doublet_threshold, max_iter, min_loci, labels, held, out, ll, ll_pair, posterior,
                                                   doublet_posterior, nullptr, best_pair, nullptr, qual);
    if (c->timing) timer_collect(c);
    return st;
}

// ---- genotype clusters without labels: kernels_cluster.hip ----------------------------------------------------
cellector_status cellector_cluster_default_params(cellector_cluster_params *out)
{
    if (!out) return CELLECTOR_EINVAL;
    out->theta_floor = 0.01;
    out->anneal_base = 20.0;
    out->tol = 0.01;
    out->anneal_steps = 9;
    out->max_iter = 50;
    out->min_loci = 1;
    return CELLECTOR_OK;
}

// what every cluster call checks before anything is written or launched
static cellector_status cluster_call_check(cellector_ctx *c, const char *what, double theta_floor)
{
    CHK(locus_moments_scope(c, what));
    READY(c);
    if (c->em_phase != 0) return ctx_fail(c, CELLECTOR_EINVAL, "%s: iteration in flight (finish it with cellector_em_finish)", what);
    if (!(theta_floor > 0.0 && theta_floor < 0.5))
        return ctx_fail(c, CELLECTOR_EINVAL, "%s: theta_floor = %g is not within (0, 0.5)", what, theta_floor);
    return CELLECTOR_OK;
}
static cellector_status cluster_columns_check(cellector_ctx *c, const char *what, uint32_t K, uint32_t R)
{
    if (K < 2 || K > 16) return ctx_fail(c, CELLECTOR_EINVAL, "%s: %u clusters, 2..16 are supported", what, K);
    if (R < 1) return ctx_fail(c, CELLECTOR_EINVAL, "%s: at least one restart is needed", what);
    if ((uint64_t)K * R > 64) return ctx_fail(c, CELLECTOR_EINVAL, "%s: %u clusters x %u restarts = %llu columns, at most 64 are supported", what, K, R,
                                              (unsigned long long)K * R);
    return CELLECTOR_OK;
}

cellector_status cellector_cluster(cellector_ctx *c, uint32_t n_clusters, uint32_t n_restarts, uint64_t seed, const cellector_cluster_params *p,
                                   const uint8_t *mask, uint8_t *labels, double *ll, double *posterior, double *theta, double *objective,
                                   cellector_cluster_summary *out)
{
    if (!c) return CELLECTOR_EINVAL;
    cellector_cluster_params prm;
    cellector_cluster_default_params(&prm);
    if (p) prm = *p;
    CHK(cluster_call_check(c, "cluster", prm.theta_floor));
    CHK(cluster_columns_check(c, "cluster", n_clusters, n_restarts));
    if (prm.anneal_steps < 1 || prm.anneal_steps > 16)
        return ctx_fail(c, CELLECTOR_EINVAL, "cluster: anneal_steps = %u is not within 1..16", prm.anneal_steps);
    if (!std::isfinite(prm.anneal_base) || prm.anneal_base <= 0.0)
        return ctx_fail(c, CELLECTOR_EINVAL, "cluster: anneal_base = %g is not a finite value > 0", prm.anneal_base);
    if (!std::isfinite(prm.tol) || prm.tol <= 0.0) return ctx_fail(c, CELLECTOR_EINVAL, "cluster: tol = %g is not a finite value > 0", prm.tol);
    REQUIRE(c, prm.min_loci >= 1, "cluster: min_loci must be at least 1");
    SETDEV(c);
    return cluster_run(c, n_clusters, n_restarts, seed, &prm, mask, labels, ll, posterior, theta, objective, out);
}

cellector_status cellector_cluster_m_step(cellector_ctx *c, const double *w, uint32_t J, const uint8_t *mask, double theta_floor, double *A,
                                          double *T, double *theta, double *tab)
{
    if (!c) return CELLECTOR_EINVAL;
    CHK(cluster_call_check(c, "cluster_m_step", theta_floor));
    if (J < 1 || J > 64) return ctx_fail(c, CELLECTOR_EINVAL, "cluster_m_step: %u columns, 1..64 are supported", J);
    REQUIRE(c, w != nullptr, "cluster_m_step: null w");
    for (uint64_t i = 0, n = c->nloc * J; i < n; i++)
        if (!(w[i] >= 0.0))
            return ctx_fail(c, CELLECTOR_EINVAL, "cluster_m_step: w of cell %llu, column %llu is %g: neither NaN nor a negative value is a weight",
                            (unsigned long long)(i / J), (unsigned long long)(i % J), w[i]);
    SETDEV(c);
    return cluster_m_step_run(c, w, J, mask, theta_floor, A, T, theta, tab);
}

cellector_status cellector_cluster_e_step(cellector_ctx *c, const double *tab, uint32_t K, uint32_t R, const double *temp, const uint8_t *mask,
                                          double *s, double *w, double *objective)
{
    if (!c) return CELLECTOR_EINVAL;
    CHK(cluster_call_check(c, "cluster_e_step", 0.25));
    CHK(cluster_columns_check(c, "cluster_e_step", K, R));
    REQUIRE(c, tab != nullptr, "cluster_e_step: null tab");
    for (uint64_t i = 0; temp && i < c->nloc; i++)
        if (!(temp[i] >= 1.0))
            return ctx_fail(c, CELLECTOR_EINVAL, "cluster_e_step: temp of cell %llu is %g: a temperature is a value >= 1", (unsigned long long)i, temp[i]);
    SETDEV(c);
    return cluster_e_step_run(c, tab, K, R, temp, mask, s, w, objective);
}

// ---- donor demultiplexing: kernels_donors.hip -------------------------------------------------------------------
cellector_status cellector_donor_default_params(cellector_donor_params *out)
{
    if (!out) return CELLECTOR_EINVAL;
    out->err = 0.01;
    out->ambient = 0.03;
    out->doublet_rate = 0.1;
    out->posterior_threshold = 0.999;
    out->min_loci = 1;
    return CELLECTOR_OK;
}

// what every donor call checks before anything is written or launched (the scope first: class_call_check's own for the match)
// (calls: gt, or the gp of a soft call; null_name: what the message calls it)
static cellector_status donor_params_check(cellector_ctx *c, const char *what, const void *calls, const char *null_name, uint32_t D,
                                           const cellector_donor_params *p)
{
    if (D < 1 || D > 64) return ctx_fail(c, CELLECTOR_EINVAL, "%s: %u donors, 1..64 are supported", what, D);
    if (!calls) return ctx_fail(c, CELLECTOR_EINVAL, "%s: null %s", what, null_name);
    if (!(p->err > 0.0 && p->err < 0.5)) return ctx_fail(c, CELLECTOR_EINVAL, "%s: err = %g is not within (0, 0.5)", what, p->err);
    if (!(p->ambient >= 0.0 && p->ambient < 1.0)) return ctx_fail(c, CELLECTOR_EINVAL, "%s: ambient = %g is not within [0, 1)", what, p->ambient);
    if (!(p->doublet_rate >= 0.0 && p->doublet_rate < 1.0))
        return ctx_fail(c, CELLECTOR_EINVAL, "%s: doublet_rate = %g is not within [0, 1)", what, p->doublet_rate);
    if (!(p->posterior_threshold >= 0.0 && p->posterior_threshold <= 1.0))
        return ctx_fail(c, CELLECTOR_EINVAL, "%s: posterior_threshold = %g is not within [0, 1]", what, p->posterior_threshold);
    if (p->min_loci < 1) return ctx_fail(c, CELLECTOR_EINVAL, "%s: min_loci must be at least 1", what);
    return CELLECTOR_OK;
}
static cellector_status donor_args_check(cellector_ctx *c, const char *what, const uint8_t *gt, uint32_t D, const cellector_donor_params *p)
{
    CHK(donor_params_check(c, what, gt, "gt", D, p));
    const uint64_t TL = c->total_loci;
    for (uint32_t d = 0; d < D; d++)
        for (uint64_t t = 0; t < TL; t++)
            if (gt[(uint64_t)d * TL + t] > 3)
                return ctx_fail(c, CELLECTOR_EINVAL, "%s: gt of donor %u at locus %llu is %u: 0 = 0/0, 1 = 0/1, 2 = 1/1, 3 = no call", what, d,
                                (unsigned long long)t, (unsigned)gt[(uint64_t)d * TL + t]);
    return CELLECTOR_OK;
}
static cellector_status donor_call_check(cellector_ctx *c, const char *what, const uint8_t *gt, uint32_t D, const cellector_donor_params *p)
{
    CHK(locus_moments_scope(c, what));
    READY(c);
    if (c->em_phase != 0) return ctx_fail(c, CELLECTOR_EINVAL, "%s: iteration in flight (finish it with cellector_em_finish)", what);
    return donor_args_check(c, what, gt, D, p);
}
// the soft calls: every row of gp is three NaN (no call) or three finite weights >= 0 that are not all zero
static cellector_status donor_gp_check(cellector_ctx *c, const char *what, const float *gp, uint32_t D, const cellector_donor_params *p)
{
    CHK(donor_params_check(c, what, gp, "gp", D, p));
    const uint64_t TL = c->total_loci;
    for (uint32_t d = 0; d < D; d++)
        for (uint64_t t = 0; t < TL; t++) {
            const float *r = gp + ((uint64_t)d * TL + t) * 3;
            if (std::isnan(r[0]) && std::isnan(r[1]) && std::isnan(r[2])) continue;
            bool fine = r[0] > 0.f || r[1] > 0.f || r[2] > 0.f;
            for (int g = 0; g < 3; g++) fine = fine && r[g] >= 0.f && std::isfinite(r[g]);
            if (!fine)
                return ctx_fail(c, CELLECTOR_EINVAL, "%s: gp of donor %u at locus %llu is (%g, %g, %g): three NaN (no call), or three finite weights >= 0 that are not all zero",
                                what, d, (unsigned long long)t, (double)r[0], (double)r[1], (double)r[2]);
        }
    return CELLECTOR_OK;
}
static cellector_status donor_gp_call_check(cellector_ctx *c, const char *what, const float *gp, uint32_t D, const cellector_donor_params *p)
{
    CHK(locus_moments_scope(c, what));
    READY(c);
    if (c->em_phase != 0) return ctx_fail(c, CELLECTOR_EINVAL, "%s: iteration in flight (finish it with cellector_em_finish)", what);
    return donor_gp_check(c, what, gp, D, p);
}

cellector_status cellector_donor_tables(cellector_ctx *c, const uint8_t *gt, uint32_t n_donors, const cellector_donor_params *p,
                                        const uint8_t *mask, double *tab1, double *tab2, uint64_t *packed)
{
    if (!c) return CELLECTOR_EINVAL;
    cellector_donor_params prm;
    cellector_donor_default_params(&prm);
    if (p) prm = *p;
    CHK(donor_call_check(c, "donor_tables", gt, n_donors, &prm));
    SETDEV(c);
    return donor_tables_run(c, gt, n_donors, &prm, mask, tab1, tab2, packed);
}

// the prior and the anchors of a cell call; lp [64]: the caller's prior, or zeros
static cellector_status donor_prior_anchor_check(cellector_ctx *c, const char *what, uint32_t D, const double *log_prior, const uint8_t *anchor,
                                                 double *lp)
{
    bool any = !log_prior;
    for (uint32_t d = 0; log_prior && d < D; d++) {
        if (std::isnan(log_prior[d]) || log_prior[d] == INFINITY)
            return ctx_fail(c, CELLECTOR_EINVAL, "%s: log_prior[%u] = %g is neither a finite value nor -inf", what, d, log_prior[d]);
        any = any || log_prior[d] != -INFINITY;
        lp[d] = log_prior[d];
    }
    if (!any) return ctx_fail(c, CELLECTOR_EINVAL, "%s: log_prior is -inf for every donor", what);
    for (uint64_t i = 0; anchor && i < c->nloc; i++)
        if (anchor[i] >= D)
            return ctx_fail(c, CELLECTOR_EINVAL, "%s: anchor of cell %llu is %u, not below the %u donors", what, (unsigned long long)i,
                            (unsigned)anchor[i], D);
    return CELLECTOR_OK;
}

// cellector_donor_posteriors (gp null) and cellector_donor_posteriors_gp (gt null): the same checks, the same run
static cellector_status donor_posteriors_call(cellector_ctx *c, const char *what, const uint8_t *gt, const float *gp, uint32_t n_donors,
                                              const cellector_donor_params *p, const double *log_prior, const uint8_t *anchor,
                                              const uint8_t *mask, double *ll, double *pair_ll, double *posterior, double *pair_posterior,
                                              double *doublet_posterior, uint8_t *best, uint8_t *second, uint8_t *best_pair,
                                              uint32_t *n_entries, uint8_t *status, uint8_t *anchor_out, cellector_donor_summary *out,
                                              double *tab1, double *tab2, bool soft)
{
    if (!c) return CELLECTOR_EINVAL;
    cellector_donor_params prm;
    cellector_donor_default_params(&prm);
    if (p) prm = *p;
    if (soft) CHK(donor_gp_call_check(c, what, gp, n_donors, &prm));
    else CHK(donor_call_check(c, what, gt, n_donors, &prm));
    const uint32_t D = n_donors;
    double lp[64] = {};
    CHK(donor_prior_anchor_check(c, what, D, log_prior, anchor, lp));
    const double log_singlet = std::log(1.0 - prm.doublet_rate);
    const double log_pair = D > 1 ? std::log(prm.doublet_rate / (double)(D - 1)) : 0.0;
    SETDEV(c);
    return donor_posteriors_run(c, gt, gp, D, &prm, lp, anchor, mask, log_singlet, log_pair, ll, pair_ll, posterior, pair_posterior,
                                doublet_posterior, best, second, best_pair, n_entries, status, anchor_out, out, tab1, tab2, nullptr);
}

cellector_status cellector_donor_posteriors(cellector_ctx *c, const uint8_t *gt, uint32_t n_donors, const cellector_donor_params *p,
                                            const double *log_prior, const uint8_t *anchor, const uint8_t *mask, double *ll, double *pair_ll,
                                            double *posterior, double *pair_posterior, double *doublet_posterior, uint8_t *best,
                                            uint8_t *second, uint8_t *best_pair, uint32_t *n_entries, uint8_t *status, uint8_t *anchor_out,
                                            cellector_donor_summary *out, double *tab1, double *tab2)
{
    return donor_posteriors_call(c, "donor_posteriors", gt, nullptr, n_donors, p, log_prior, anchor, mask, ll, pair_ll, posterior, pair_posterior,
                                 doublet_posterior, best, second, best_pair, n_entries, status, anchor_out, out, tab1, tab2, false);
}

cellector_status cellector_match_donors(cellector_ctx *c, const uint8_t *labels, uint32_t n_classes, const uint8_t *gt, uint32_t n_donors,
                                        const cellector_donor_params *p, const uint8_t *mask, double *ll, uint8_t *best, double *margin,
                                        uint64_t *cells)
{
    if (!c) return CELLECTOR_EINVAL;
    cellector_donor_params prm;
    cellector_donor_default_params(&prm);
    if (p) prm = *p;
    CHK(class_call_check(c, "match_donors", labels, n_classes, nullptr, nullptr));
    CHK(donor_args_check(c, "match_donors", gt, n_donors, &prm));
    SETDEV(c);
    return donor_match_run(c, labels, n_classes, gt, nullptr, n_donors, &prm, mask, ll, best, margin, cells);
}

// ---- the fit of the called hypothesis: k_donor_moments and k_donor_fit of kernels_donors.hip -------------------------------------
cellector_status cellector_donor_fit_default_params(cellector_donor_fit_params *out)
{
    if (!out) return CELLECTOR_EINVAL;
    out->iqr_multiple = 3.0;
    out->min_cells = 8;
    return CELLECTOR_OK;
}

cellector_status cellector_donor_moment_tables(cellector_ctx *c, const cellector_donor_params *p, const uint8_t *mask, double *mom1, double *mom2)
{
    if (!c) return CELLECTOR_EINVAL;
    cellector_donor_params prm;
    cellector_donor_default_params(&prm);
    if (p) prm = *p;
    CHK(locus_moments_scope(c, "donor_moment_tables"));
    READY(c);
    if (c->em_phase != 0) return ctx_fail(c, CELLECTOR_EINVAL, "donor_moment_tables: iteration in flight (finish it with cellector_em_finish)");
    CHK(donor_params_check(c, "donor_moment_tables", &prm /*(the tables depend on no donor)*/, "gt", 1, &prm));
    SETDEV(c);
    return donor_moment_tables_run(c, &prm, mask, mom1, mom2);
}

cellector_status cellector_donor_fit(cellector_ctx *c, const uint8_t *gt, uint32_t n_donors, const cellector_donor_params *p,
                                     const cellector_donor_fit_params *fit, const double *log_prior, const uint8_t *anchor, const uint8_t *mask,
                                     double *fit_e, double *fit_v, double *pair_e, double *pair_v, double *z, double *pair_z, double *call_z,
                                     uint8_t *hyp_a, uint8_t *hyp_b, uint8_t *status, uint8_t *unmatched, cellector_donor_fit_summary *out,
                                     double *mom1, double *mom2)
{
    if (!c) return CELLECTOR_EINVAL;
    cellector_donor_params prm;
    cellector_donor_default_params(&prm);
    if (p) prm = *p;
    cellector_donor_fit_params fp;
    cellector_donor_fit_default_params(&fp);
    if (fit) fp = *fit;
    CHK(donor_call_check(c, "donor_fit", gt, n_donors, &prm));
    if (!(fp.iqr_multiple >= 0.0)) return ctx_fail(c, CELLECTOR_EINVAL, "donor_fit: iqr_multiple = %g is not a value >= 0", fp.iqr_multiple);
    if (fp.min_cells < 4) return ctx_fail(c, CELLECTOR_EINVAL, "donor_fit: min_cells must be at least 4");
    const uint32_t D = n_donors;
    double lp[64] = {};
    CHK(donor_prior_anchor_check(c, "donor_fit", D, log_prior, anchor, lp));
    const double log_singlet = std::log(1.0 - prm.doublet_rate);
    const double log_pair = D > 1 ? std::log(prm.doublet_rate / (double)(D - 1)) : 0.0;
    SETDEV(c);
    return donor_fit_run(c, gt, D, &prm, &fp, lp, anchor, mask, log_singlet, log_pair, fit_e, fit_v, pair_e, pair_v, z, pair_z, call_z, hyp_a,
                         hyp_b, status, unmatched, out, mom1, mom2);
}

// ---- the donor calls from genotype probabilities: the soft kernels of kernels_donors.hip ------------------------------------------
cellector_status cellector_donor_posteriors_gp(cellector_ctx *c, const float *gp, uint32_t n_donors, const cellector_donor_params *p,
                                               const double *log_prior, const uint8_t *anchor, const uint8_t *mask, double *ll, double *pair_ll,
                                               double *posterior, double *pair_posterior, double *doublet_posterior, uint8_t *best,
                                               uint8_t *second, uint8_t *best_pair, uint32_t *n_entries, uint8_t *status, uint8_t *anchor_out,
                                               cellector_donor_summary *out, double *tab1, double *tab2)
{
    return donor_posteriors_call(c, "donor_posteriors_gp", nullptr, gp, n_donors, p, log_prior, anchor, mask, ll, pair_ll, posterior,
                                 pair_posterior, doublet_posterior, best, second, best_pair, n_entries, status, anchor_out, out, tab1, tab2, true);
}

cellector_status cellector_donor_weights(cellector_ctx *c, const float *gp, uint32_t n_donors, double *w, uint8_t *kind)
{
    if (!c) return CELLECTOR_EINVAL;
    cellector_donor_params prm;
    cellector_donor_default_params(&prm);
    CHK(donor_gp_call_check(c, "donor_weights", gp, n_donors, &prm));
    SETDEV(c);
    return donor_weights_run(c, gp, n_donors, w, kind);
}

cellector_status cellector_match_donors_gp(cellector_ctx *c, const uint8_t *labels, uint32_t n_classes, const float *gp, uint32_t n_donors,
                                           const cellector_donor_params *p, const uint8_t *mask, double *ll, uint8_t *best, double *margin,
                                           uint64_t *cells)
{
    if (!c) return CELLECTOR_EINVAL;
    cellector_donor_params prm;
    cellector_donor_default_params(&prm);
    if (p) prm = *p;
    CHK(class_call_check(c, "match_donors_gp", labels, n_classes, nullptr, nullptr));
    CHK(donor_gp_check(c, "match_donors_gp", gp, n_donors, &prm));
    SETDEV(c);
    return donor_match_run(c, labels, n_classes, nullptr, gp, n_donors, &prm, mask, ll, best, margin, cells);
}

// ---- ambient fraction estimation: kernels_ambient.hip --------------------------------------------------------------
cellector_status cellector_ambient_default_params(cellector_ambient_params *out)
{
    if (!out) return CELLECTOR_EINVAL;
    out->err = 0.01;
    out->lo = 0.0;
    out->hi = 0.5;
    out->grid = 16;
    out->rounds = 3;
    out->min_loci = 1;
    return CELLECTOR_OK;
}

// what every ambient call checks before anything is written or launched: the scope of the donor calls, then the arguments all share
static cellector_status ambient_scope_check(cellector_ctx *c, const char *what, uint32_t G, double err)
{
    CHK(locus_moments_scope(c, what));
    READY(c);
    if (c->em_phase != 0) return ctx_fail(c, CELLECTOR_EINVAL, "%s: iteration in flight (finish it with cellector_em_finish)", what);
    if (G < 4 || G > 32) return ctx_fail(c, CELLECTOR_EINVAL, "%s: %u grid points, 4..32 are supported", what, G);
    if (!(err > 0.0 && err < 0.5)) return ctx_fail(c, CELLECTOR_EINVAL, "%s: err = %g is not within (0, 0.5)", what, err);
    return CELLECTOR_OK;
}
static cellector_status ambient_grid_check(cellector_ctx *c, const char *what, const double *rho, uint32_t G)
{
    if (!rho) return ctx_fail(c, CELLECTOR_EINVAL, "%s: null rho", what);
    for (uint32_t j = 0; j < G; j++)
        if (!(rho[j] >= 0.0 && rho[j] < 1.0)) return ctx_fail(c, CELLECTOR_EINVAL, "%s: rho[%u] = %g is not within [0, 1)", what, j, rho[j]);
    return CELLECTOR_OK;
}
static cellector_status ambient_sources_check(cellector_ctx *c, const char *what, const uint8_t *gt, uint32_t S, const uint8_t *assign,
                                              uint64_t min_loci)
{
    if (S < 1 || S > 64) return ctx_fail(c, CELLECTOR_EINVAL, "%s: %u sources, 1..64 are supported", what, S);
    if (!gt) return ctx_fail(c, CELLECTOR_EINVAL, "%s: null gt", what);
    if (!assign) return ctx_fail(c, CELLECTOR_EINVAL, "%s: null assign", what);
    if (min_loci < 1) return ctx_fail(c, CELLECTOR_EINVAL, "%s: min_loci must be at least 1", what);
    const uint64_t TL = c->total_loci;
    for (uint32_t s = 0; s < S; s++)
        for (uint64_t t = 0; t < TL; t++)
            if (gt[(uint64_t)s * TL + t] > 3)
                return ctx_fail(c, CELLECTOR_EINVAL, "%s: gt of source %u at locus %llu is %u: 0 = 0/0, 1 = 0/1, 2 = 1/1, 3 = no call", what, s,
                                (unsigned long long)t, (unsigned)gt[(uint64_t)s * TL + t]);
    for (uint64_t i = 0; i < c->nloc; i++)
        if (assign[i] != 255 && assign[i] >= S)
            return ctx_fail(c, CELLECTOR_EINVAL, "%s: assign of cell %llu is %u, neither 255 nor below the %u sources", what,
                            (unsigned long long)i, (unsigned)assign[i], S);
    return CELLECTOR_OK;
}

cellector_status cellector_ambient_tables(cellector_ctx *c, const double *rho, uint32_t n_grid, double err, const uint8_t *mask, double *tab)
{
    if (!c) return CELLECTOR_EINVAL;
    CHK(ambient_scope_check(c, "ambient_tables", n_grid, err));
    CHK(ambient_grid_check(c, "ambient_tables", rho, n_grid));
    SETDEV(c);
    return ambient_tables_run(c, rho, n_grid, err, mask, tab);
}

cellector_status cellector_ambient_profile(cellector_ctx *c, const uint8_t *gt, uint32_t n_sources, const uint8_t *assign, const double *rho,
                                           uint32_t n_grid, double err, uint64_t min_loci, const uint8_t *mask, double *ll, double *total,
                                           double *source_total, uint64_t *source_cells, uint32_t *n_entries, double *cell_rho,
                                           double *cell_se, double *tab)
{
    if (!c) return CELLECTOR_EINVAL;
    CHK(ambient_scope_check(c, "ambient_profile", n_grid, err));
    CHK(ambient_grid_check(c, "ambient_profile", rho, n_grid));
    CHK(ambient_sources_check(c, "ambient_profile", gt, n_sources, assign, min_loci));
    SETDEV(c);
    return ambient_profile_run(c, gt, n_sources, assign, rho, n_grid, err, min_loci, mask, ll, total, source_total, source_cells, n_entries,
                               cell_rho, cell_se, tab);
}

cellector_status cellector_estimate_ambient(cellector_ctx *c, const uint8_t *gt, uint32_t n_sources, const uint8_t *assign,
                                            const cellector_ambient_params *params, const uint8_t *mask, cellector_ambient_summary *summary,
                                            double *cell_rho, double *cell_se, uint32_t *n_entries)
{
    if (!c) return CELLECTOR_EINVAL;
    cellector_ambient_params prm;
    cellector_ambient_default_params(&prm);
    if (params) prm = *params;
    CHK(ambient_scope_check(c, "estimate_ambient", prm.grid, prm.err));
    if (!(prm.lo >= 0.0 && prm.lo < prm.hi && prm.hi < 1.0))
        return ctx_fail(c, CELLECTOR_EINVAL, "estimate_ambient: lo = %g, hi = %g do not satisfy 0 <= lo < hi < 1", prm.lo, prm.hi);
    if (prm.rounds < 1 || prm.rounds > 8) return ctx_fail(c, CELLECTOR_EINVAL, "estimate_ambient: %u rounds, 1..8 are supported", prm.rounds);
    CHK(ambient_sources_check(c, "estimate_ambient", gt, n_sources, assign, prm.min_loci));
    SETDEV(c);
    return ambient_estimate_run(c, gt, n_sources, assign, &prm, mask, summary, cell_rho, cell_se, n_entries);
}

// ---- donor pair fractions: kernels_pair_fraction.hip ----------------------------------------------------------------
cellector_status cellector_pair_fraction_default_params(cellector_pair_fraction_params *out)
{
    if (!out) return CELLECTOR_EINVAL;
    out->min_fraction = 0.1;
    out->min_loci = 1;
    return CELLECTOR_OK;
}

// the grid of a pair fraction call: the caller's, checked, or the default j / 16.0; grid [32] receives it
static cellector_status pair_fraction_grid_check(cellector_ctx *c, const char *what, const double *frac, uint32_t *G, double *grid)
{
    if (!frac) {
        *G = 17;
        for (uint32_t j = 0; j < 17; j++) grid[j] = (double)j / 16.0;
        return CELLECTOR_OK;
    }
    if (*G < 4 || *G > 32) return ctx_fail(c, CELLECTOR_EINVAL, "%s: %u grid points, 4..32 are supported", what, *G);
    for (uint32_t j = 0; j < *G; j++) {
        if (!(frac[j] >= 0.0 && frac[j] <= 1.0)) return ctx_fail(c, CELLECTOR_EINVAL, "%s: frac[%u] = %g is not within [0, 1]", what, j, frac[j]);
        if (j && !(frac[j] > frac[j - 1]))
            return ctx_fail(c, CELLECTOR_EINVAL, "%s: frac[%u] = %g is not above frac[%u] = %g: the grid ascends strictly", what, j, frac[j],
                            j - 1, frac[j - 1]);
        grid[j] = frac[j];
    }
    return CELLECTOR_OK;
}

cellector_status cellector_pair_fraction_tables(cellector_ctx *c, const cellector_donor_params *donor_params, const double *frac, uint32_t n_grid,
                                                const uint8_t *mask, double *tab)
{
    if (!c) return CELLECTOR_EINVAL;
    cellector_donor_params prm;
    cellector_donor_default_params(&prm);
    if (donor_params) prm = *donor_params;
    CHK(locus_moments_scope(c, "pair_fraction_tables"));
    READY(c);
    if (c->em_phase != 0) return ctx_fail(c, CELLECTOR_EINVAL, "pair_fraction_tables: iteration in flight (finish it with cellector_em_finish)");
    CHK(donor_params_check(c, "pair_fraction_tables", &prm /*(the tables depend on no donor)*/, "gt", 1, &prm));
    double grid[32];
    uint32_t G = n_grid;
    CHK(pair_fraction_grid_check(c, "pair_fraction_tables", frac, &G, grid));
    SETDEV(c);
    return pair_fraction_tables_run(c, &prm, grid, G, mask, tab);
}

cellector_status cellector_donor_pair_fractions(cellector_ctx *c, const uint8_t *gt, uint32_t n_donors, const cellector_donor_params *donor_params,
                                                const cellector_pair_fraction_params *params, const uint8_t *pair_a, const uint8_t *pair_b,
                                                const double *frac, uint32_t n_grid, const uint8_t *mask, double *ll, uint32_t *n_entries,
                                                double *cell_frac, double *cell_se, uint8_t *j_star, uint8_t *kind,
                                                cellector_pair_fraction_summary *summary, double *tab)
{
    if (!c) return CELLECTOR_EINVAL;
    const char *what = "donor_pair_fractions";
    cellector_donor_params prm;
    cellector_donor_default_params(&prm);
    if (donor_params) prm = *donor_params;
    cellector_pair_fraction_params fp;
    cellector_pair_fraction_default_params(&fp);
    if (params) fp = *params;
    CHK(donor_call_check(c, what, gt, n_donors, &prm));
    const uint32_t D = n_donors;
    if (!pair_a) return ctx_fail(c, CELLECTOR_EINVAL, "%s: null pair_a", what);
    if (!pair_b) return ctx_fail(c, CELLECTOR_EINVAL, "%s: null pair_b", what);
    for (uint64_t i = 0; i < c->nloc; i++) {
        if (pair_a[i] == 255) continue;
        if (pair_a[i] >= D)
            return ctx_fail(c, CELLECTOR_EINVAL, "%s: pair_a of cell %llu is %u, neither 255 nor below the %u donors", what, (unsigned long long)i,
                            (unsigned)pair_a[i], D);
        if (pair_b[i] >= D)
            return ctx_fail(c, CELLECTOR_EINVAL, "%s: pair_b of cell %llu is %u, not below the %u donors", what, (unsigned long long)i,
                            (unsigned)pair_b[i], D);
        if (pair_b[i] == pair_a[i])
            return ctx_fail(c, CELLECTOR_EINVAL, "%s: pair_b of cell %llu is %u, its pair_a: a pair is two donors", what, (unsigned long long)i,
                            (unsigned)pair_b[i]);
    }
    double grid[32];
    uint32_t G = n_grid;
    CHK(pair_fraction_grid_check(c, what, frac, &G, grid));
    if (!(fp.min_fraction >= 0.0 && fp.min_fraction <= 0.5))
        return ctx_fail(c, CELLECTOR_EINVAL, "%s: min_fraction = %g is not within [0, 0.5]", what, fp.min_fraction);
    if (fp.min_loci < 1) return ctx_fail(c, CELLECTOR_EINVAL, "%s: min_loci must be at least 1", what);
    SETDEV(c);
    return pair_fractions_run(c, gt, D, &prm, &fp, pair_a, pair_b, grid, G, mask, ll, n_entries, cell_frac, cell_se, j_star, kind, summary, tab);
}

// ---- class genotypes: kernels_genotypes.hip and genotype_host.h ---------------------------------------------
// load_mtx_final + the rule of output_final_vcf (main.rs:52-131) for the K classes of a labelling
cellector_status cellector_class_genotypes(cellector_ctx *c, const uint8_t *labels, uint32_t n_classes, double ambient, double gt_threshold,
                                           uint64_t *cells, uint64_t *alt, uint64_t *ref, uint8_t *gt, double *gp, double *gp3)
{
    if (!c) return CELLECTOR_EINVAL;
    CHK(class_call_check(c, "class_genotypes", labels, n_classes, nullptr, nullptr));
    if (!(ambient >= 0.0 && ambient <= 1.0)) return ctx_fail(c, CELLECTOR_EINVAL, "class_genotypes: ambient = %g is not within [0, 1]", ambient);
    if (!(gt_threshold >= 0.0 && gt_threshold <= 1.0))
        return ctx_fail(c, CELLECTOR_EINVAL, "class_genotypes: gt_threshold = %g is not within [0, 1]", gt_threshold);
    REQUIRE(c, c->keep_coo && (c->coo.locus || !c->nnz), "final tallies need the staged COO (option keep_coo=1)");
    SETDEV(c);
    const uint32_t K = n_classes;
    const uint64_t TL = c->total_loci, n = c->nloc, planes = (uint64_t)(K + 1) * 2;
    // every buffer first: on CELLECTOR_ENOMEM nothing has been written
    DevBuf<uint64_t> d_acc;
    DevBuf<uint8_t> d_lab;
    CHK(dev_alloc(c, &d_acc, planes * TL));
    CHK(dev_alloc(c, &d_lab, n));
    std::vector<uint64_t> h;
    try {
        if (alt || ref || gt || gp || gp3) h.resize(planes * TL);
    } catch (const std::bad_alloc &) {
        return ctx_fail(c, CELLECTOR_ENOMEM, "class_genotypes: out of host memory");
    }
    if (n) HIPCHK(c, hipMemcpyAsync(d_lab, labels, n, hipMemcpyHostToDevice, c->stream));
    CHK(launch_genotype_tallies(c, d_lab, K, d_acc));
    const bool rule = gt || gp || gp3;
    if ((alt || ref || rule) && TL) CHK(d2h(c, h.data(), d_acc, planes * TL * 8));
    else HIPCHK(c, hipStreamSynchronize(c->stream));  // (the caller's labels have been read, the scratch may go)
    d_acc.reset();
    d_lab.reset();
    if (cells) {
        for (uint32_t k = 0; k <= K; k++) cells[k] = 0;
        for (uint64_t i = 0; i < n; i++) cells[labels[i] == 255 ? K : labels[i]]++;
    }
    for (uint32_t k = 0; k <= K && TL; k++) {
        if (alt) memcpy(alt + (uint64_t)k * TL, h.data() + (uint64_t)k * 2 * TL, TL * 8);
        if (ref) memcpy(ref + (uint64_t)k * TL, h.data() + ((uint64_t)k * 2 + 1) * TL, TL * 8);
    }
    if (!rule) return CELLECTOR_OK;
    for (uint64_t l = 0; l < TL; l++) {
        uint64_t A = 0, R = 0;
        for (uint32_t k = 0; k <= K; k++) { A += h[(uint64_t)k * 2 * TL + l]; R += h[((uint64_t)k * 2 + 1) * TL + l]; }
        const GenotypeLocus g = genotype_locus(A, R, ambient);
        for (uint32_t k = 0; k < K; k++) {
            const GenotypeCall q = genotype_call(g, h[(uint64_t)k * 2 * TL + l], h[((uint64_t)k * 2 + 1) * TL + l], gt_threshold);
            const uint64_t o = (uint64_t)k * TL + l;
            if (gt) gt[o] = q.gt;
            if (gp) gp[o] = q.gp;
            if (gp3) { gp3[3 * o] = q.q[0]; gp3[3 * o + 1] = q.q[1]; gp3[3 * o + 2] = q.q[2]; }
        }
    }
    return CELLECTOR_OK;
}

// ---- donor genotype refinement: kernels_donor_genotypes.hip ------------------------------------------------
cellector_status cellector_donor_genotypes_default_params(cellector_donor_genotypes_params *out)
{
    if (!out) return CELLECTOR_EINVAL;
    out->err = 0.01;
    out->ambient = 0.03;
    out->gt_threshold = 0.99;
    out->prior_floor = 0.01;
    return CELLECTOR_OK;
}

cellector_status cellector_donor_genotypes(cellector_ctx *c, const uint8_t *assign, const float *prior, uint32_t n_donors,
                                           const cellector_donor_genotypes_params *params, uint64_t *cells, uint64_t *alt, uint64_t *ref,
                                           double *q, uint8_t *gt_out, uint8_t *kind, cellector_donor_genotypes_summary *summary, double *tab,
                                           double *pass_ms)
{
    if (!c) return CELLECTOR_EINVAL;
    const char *what = "donor_genotypes";
    cellector_donor_genotypes_params prm;
    cellector_donor_genotypes_default_params(&prm);
    if (params) prm = *params;
    CHK(locus_moments_scope(c, what));
    READY(c);
    if (c->em_phase != 0) return ctx_fail(c, CELLECTOR_EINVAL, "%s: iteration in flight (finish it with cellector_em_finish)", what);
    cellector_donor_params dp;  // (err and ambient are the donor call's, and so are their checks)
    cellector_donor_default_params(&dp);
    dp.err = prm.err;
    dp.ambient = prm.ambient;
    const uint32_t D = n_donors;
    CHK(donor_params_check(c, what, &dp /*(a NULL prior is no error)*/, "prior", D, &dp));
    if (!(prm.gt_threshold >= 0.0 && prm.gt_threshold <= 1.0))
        return ctx_fail(c, CELLECTOR_EINVAL, "%s: gt_threshold = %g is not within [0, 1]", what, prm.gt_threshold);
    if (!(prm.prior_floor >= 0.0 && prm.prior_floor <= 1.0))
        return ctx_fail(c, CELLECTOR_EINVAL, "%s: prior_floor = %g is not within [0, 1]", what, prm.prior_floor);
    if (!assign) return ctx_fail(c, CELLECTOR_EINVAL, "%s: null assign", what);
    for (uint64_t i = 0; i < c->nloc; i++)
        if (assign[i] >= D && assign[i] != 255)
            return ctx_fail(c, CELLECTOR_EINVAL, "%s: assign of cell %llu is %u, neither below the %u donors nor 255 (no part)", what,
                            (unsigned long long)i, (unsigned)assign[i], D);
    if (prior) CHK(donor_gp_check(c, what, prior, D, &dp));
    REQUIRE(c, c->keep_coo && (c->coo.locus || !c->nnz), "donor_genotypes needs the staged COO (option keep_coo=1)");
    SETDEV(c);
    return donor_genotypes_run(c, assign, prior, D, &prm, cells, alt, ref, q, gt_out, kind, summary, tab, pass_ms);
}

// ---- posteriors ---------------------------------------------------------------------------------------
// the minority fraction and the three log priors of calculate_posteriors, from the current exclusion set
struct PosteriorPriors { double mf0, lp_min, lp_maj, lp_dbl; };
static PosteriorPriors posterior_priors(const cellector_ctx *c)
{
    PosteriorPriors p;
    const double N = (double)c->total_cells;
    p.mf0 = ((double)c->n_excluded_global + 1.0) / (N + 1.0);             // main.rs:240
    const double mf = std::fmax(p.mf0, 0.01);                             // main.rs:250
    p.lp_dbl = std::log(N / 1000.0 / 100.0 * std::fmax(mf, 0.1));         // main.rs:259
    p.lp_min = std::log(mf);                                              // main.rs:264-265
    p.lp_maj = std::log(1.0 - mf);
    return p;
}

cellector_status cellector_posterior_alpha_betas(cellector_ctx *c, int which, double *alpha, double *beta)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) {  // per-locus state is replicated: shard 0 answers
        cellector_ctx *s0 = multi_shard0(c);
        const cellector_status st = cellector_posterior_alpha_betas(s0, which, alpha, beta);
        if (st != CELLECTOR_OK) c->err = s0->err;
        return st;
    }
    READY(c);
    REQUIRE(c, c->em_phase == 0, "posterior_alpha_betas: iteration in flight (finish it with cellector_em_finish)");
    REQUIRE(c, which >= 0 && which <= 2, "posterior_alpha_betas: which is 0 (minority), 1 (majority) or 2 (doublet)");
    SETDEV(c);
    const uint64_t L = c->L;
    DevBuf<double> ab6;  // the kernel's [8 L] layout: min, maj, dbl pairs and a pad per locus
    CHK(dev_alloc(c, &ab6, 8 * L));
    CHK(launch_ab_posterior_into(c, posterior_priors(c).mf0, ab6.get()));
    std::vector<double> h(8 * L);
    CHK(d2h(c, h.data(), ab6, 8 * L * sizeof(double)));
    for (uint64_t l = 0; l < L; l++) {
        if (alpha) alpha[l] = h[8 * l + 2 * (uint64_t)which];
        if (beta) beta[l] = h[8 * l + 2 * (uint64_t)which + 1];
    }
    return CELLECTOR_OK;
}

// the posterior phase of a single-device ctx; sdbl (device, [nloc] or null): the doublet set's per-cell sums as well
static cellector_status posteriors_run(cellector_ctx *c, double *posterior, double *doublet, double *ll_maj, double *ll_min,
                                       double *sdbl)
{
    READY(c);
    REQUIRE(c, c->em_phase == 0, "iteration in flight");
    SETDEV(c);
    const PosteriorPriors pr = posterior_priors(c);
    if (c->engine == 2) CHK(tiled_posteriors(c, pr.mf0, pr.lp_min, pr.lp_maj, pr.lp_dbl, sdbl));
    else CHK(launch_posteriors(c, pr.mf0, pr.lp_min, pr.lp_maj, pr.lp_dbl, sdbl));
    const size_t b = c->nloc * 8;
    if (posterior) CHK(d2h(c, posterior, c->post, b));
    if (doublet) CHK(d2h(c, doublet, c->post + c->nloc, b));
    if (ll_maj) CHK(d2h(c, ll_maj, c->post + 2 * c->nloc, b));
    if (ll_min) CHK(d2h(c, ll_min, c->post + 3 * c->nloc, b));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->timing) timer_collect(c);
    return CELLECTOR_OK;
}

cellector_status cellector_posteriors(cellector_ctx *c, double *posterior, double *doublet, double *ll_maj,
                                      double *ll_min)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return multi_posteriors(c, posterior, doublet, ll_maj, ll_min);
    return posteriors_run(c, posterior, doublet, ll_maj, ll_min, nullptr);
}

// ---- posteriors + the labelling rule ------------------------------------------------------------------
// The chain and the rule for the cells [lo, hi) of the list (option resolve_posteriors): per-cell independent, so any split
// over threads gives the same bits.
static void assign_finish_range(const uint32_t *ids, const double *ll3, size_t n_list, size_t lo, size_t hi, double lp_min, double lp_maj,
                                double lp_dbl, double thr, uint64_t min_loci, const uint32_t *ent, double *p, double *d, double *lmaj,
                                double *lmin, uint8_t *pa, uint64_t *q)
{
    for (size_t j = lo; j < hi; j++) {
        const uint32_t i = ids[j];
        const double s_min = ll3[j], s_maj = ll3[n_list + j], s_dbl = ll3[2 * n_list + j];
        assign_posterior(s_min, s_maj, s_dbl, lp_min, lp_maj, lp_dbl, &p[i], &d[i]);
        lmaj[i] = s_maj;
        lmin[i] = s_min;
        pa[i] = assign_label(p[i], d[i], ent[i], thr, min_loci);
        q[i] = assign_qual(p[i]);
    }
}

cellector_status cellector_assign(cellector_ctx *c, double posterior_threshold, uint64_t min_loci_used, double *posterior,
                                  double *doublet, double *ll_maj, double *ll_min, uint8_t *posterior_assignment,
                                  uint8_t *anomaly_assignment, uint64_t *qual)
{
    if (!c) return CELLECTOR_EINVAL;
    const int mode = c->multi ? 0 : c->resolve_posteriors;
    if (!c->multi) {
        READY(c);
        REQUIRE(c, c->em_phase == 0, "iteration in flight");
        REQUIRE(c, !mode || !comm_active(c->comm), "resolve_posteriors works on a single-device ctx");
        c->pa_last_mode = 0;
        c->pa_labels_changed = c->pa_qual_changed = 0;
        c->pa_ids.clear();
    }
    cellector_dims_t dm;
    CHK(cellector_dims(c, &dm));
    const size_t n = c->multi ? (size_t)dm.total_cells : (size_t)(dm.cell_end - dm.cell_begin);
    try {
        std::vector<double> &p = c->pa_host.p, &d = c->pa_host.d, &lmaj = c->pa_host.lmaj, &lmin = c->pa_host.lmin;
        std::vector<uint8_t> &excl = c->pa_host.excl, &pa = c->pa_host.pa;
        std::vector<uint32_t> &ent = c->pa_host.ent;
        std::vector<uint64_t> &q = c->pa_host.q;
        p.resize(n); d.resize(n); lmaj.resize(n); lmin.resize(n);
        excl.resize(n); pa.resize(n); ent.resize(n); q.resize(n);
        if (c->multi) CHK(cellector_posteriors(c, p.data(), d.data(), lmaj.data(), lmin.data()));
        else {
            if (mode == 1 && !c->pa_sdbl) {  // the mark kernel also reads the doublet set's sums
                SETDEV(c);
                CHK(dev_alloc(c, &c->pa_sdbl, c->nloc));
            }
            CHK(posteriors_run(c, p.data(), d.data(), lmaj.data(), lmin.data(), mode == 1 ? c->pa_sdbl.get() : nullptr));
        }
        CHK(cellector_excluded(c, excl.data()));
        CHK(cellector_entries_per_cell(c, ent.data()));
        for (size_t i = 0; i < n; i++) {  // the rule on the device's values
            pa[i] = assign_label(p[i], d[i], ent[i], posterior_threshold, min_loci_used);
            q[i] = assign_qual(p[i]);
        }
        if (mode) {
            SETDEV(c);
            const PosteriorPriors pr = posterior_priors(c);
            const double lp_min = pr.lp_min, lp_maj = pr.lp_maj, lp_dbl = pr.lp_dbl;
            std::vector<uint32_t> ids;
            std::vector<double> ll3;
            CHK(assign_resolve(c, mode, posterior_threshold, lp_min, lp_maj, lp_dbl, &ids, &ll3));
            const size_t m = ids.size();
            std::vector<uint8_t> pa_dev(m);
            std::vector<uint64_t> q_dev(m);
            for (size_t j = 0; j < m; j++) { pa_dev[j] = pa[ids[j]]; q_dev[j] = q[ids[j]]; }
            // ~10 C-library calls a cell: over up to 8 threads when the list is long (each writes its own cells only)
            size_t nt = m / 32768;
            if (nt > 8) nt = 8;
            if (nt < 1) nt = 1;
            std::vector<std::thread> th;
            th.reserve(8);
            size_t done = 0;
            for (size_t t = 1; t < nt; t++) {
                const size_t lo = m * t / nt, hi = m * (t + 1) / nt;
                try {
                    th.emplace_back(assign_finish_range, ids.data(), ll3.data(), m, lo, hi, lp_min, lp_maj, lp_dbl, posterior_threshold,
                                    min_loci_used, ent.data(), p.data(), d.data(), lmaj.data(), lmin.data(), pa.data(), q.data());
                    done = hi;
                } catch (const std::system_error &) {  // no more threads: this one takes the rest
                    break;
                }
            }
            // the first share, and whatever no thread could be made for
            assign_finish_range(ids.data(), ll3.data(), m, 0, m / nt, lp_min, lp_maj, lp_dbl, posterior_threshold, min_loci_used,
                                ent.data(), p.data(), d.data(), lmaj.data(), lmin.data(), pa.data(), q.data());
            if (nt > 1 && done < m)
                assign_finish_range(ids.data(), ll3.data(), m, std::max(done, m / nt), m, lp_min, lp_maj, lp_dbl, posterior_threshold,
                                    min_loci_used, ent.data(), p.data(), d.data(), lmaj.data(), lmin.data(), pa.data(), q.data());
            for (std::thread &t : th) t.join();
            for (size_t j = 0; j < m; j++) {
                c->pa_labels_changed += pa_dev[j] != pa[ids[j]] ? 1 : 0;
                c->pa_qual_changed += q_dev[j] != q[ids[j]] ? 1 : 0;
            }
            c->pa_ids.swap(ids);
            c->pa_last_mode = mode;
        }
        const size_t b = n * 8;
        if (posterior) memcpy(posterior, p.data(), b);
        if (doublet) memcpy(doublet, d.data(), b);
        if (ll_maj) memcpy(ll_maj, lmaj.data(), b);
        if (ll_min) memcpy(ll_min, lmin.data(), b);
        if (posterior_assignment) memcpy(posterior_assignment, pa.data(), n);
        if (anomaly_assignment)
            for (size_t i = 0; i < n; i++) anomaly_assignment[i] = excl[i] ? 0 : 1;  // main.rs:161-163
        if (qual) memcpy(qual, q.data(), b);
    } catch (const std::bad_alloc &) {
        return ctx_fail(c, CELLECTOR_ENOMEM, "cellector_assign: out of host memory");
    }
    return CELLECTOR_OK;
}

cellector_status cellector_assign_resolution(const cellector_ctx *c, cellector_assign_resolution_t *out)
{
    if (!c || !out) return CELLECTOR_EINVAL;
    memset(out, 0, sizeof *out);
    if (c->multi || !c->pa_last_mode) return CELLECTOR_OK;  // (the last cellector_assign resolved nothing)
    out->n_evaluated = c->pa_ids.size();
    out->n_labels_changed = c->pa_labels_changed;
    out->n_qual_changed = c->pa_qual_changed;
    out->mode = (uint32_t)c->pa_last_mode;
    return CELLECTOR_OK;
}

cellector_status cellector_assign_resolved_cells(const cellector_ctx *c, uint32_t *ids)
{
    if (!c || !ids) return CELLECTOR_EINVAL;
    if (c->multi || !c->pa_last_mode) return CELLECTOR_OK;
    if (!c->pa_ids.empty()) memcpy(ids, c->pa_ids.data(), c->pa_ids.size() * sizeof(uint32_t));
    return CELLECTOR_OK;
}

cellector_status cellector_final_allele_tallies(cellector_ctx *c, uint64_t *alt_min, uint64_t *ref_min,
                                                uint64_t *alt_maj, uint64_t *ref_maj)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return multi_final_allele_tallies(c, alt_min, ref_min, alt_maj, ref_maj);
    READY(c);
    REQUIRE(c, c->keep_coo, "final tallies need the staged COO (option keep_coo=1)");
    SETDEV(c);
    const uint64_t TL = c->total_loci;
    DevBuf<uint64_t> d;
    CHK(dev_alloc(c, &d, 4 * TL));
    CHK(launch_final_tallies(c, d));
    std::vector<uint64_t> h(4 * TL);
    CHK(d2h(c, h.data(), d, 4 * TL * 8));
    d.reset();
    if (alt_min) memcpy(alt_min, h.data(), TL * 8);
    if (ref_min) memcpy(ref_min, h.data() + TL, TL * 8);
    if (alt_maj) memcpy(alt_maj, h.data() + 2 * TL, TL * 8);
    if (ref_maj) memcpy(ref_maj, h.data() + 3 * TL, TL * 8);
    return CELLECTOR_OK;
}

cellector_status cellector_engine_info(const cellector_ctx *c, cellector_engine_info_t *o)
{
    if (!c || !o) return CELLECTOR_EINVAL;
    if (c->multi) return multi_engine_info(c, o);
    memset(o, 0, sizeof *o);
    o->engine = (uint64_t)c->engine;
    if (c->tiled_ready) {
        o->nnz_regular = c->nnz - c->ovf_n;
        o->nnz_overflow = c->ovf_n;
        o->cell_blocks = c->t_nb; o->locus_chunks = c->t_nj; o->chunk_groups = c->t_groups;
        const uint64_t elems = c->t_elems + (uint64_t)c->t_nb * c->t_nj * 128;  // slices + slice headers (u16 units)
        o->tile_bytes = elems * 2;
        o->tile_lookups = c->t_elems - (uint64_t)c->t_nb * c->t_nj * T_ROWS_PER_TILE;  // a row = its cell id + K entries
    }
    return CELLECTOR_OK;
}

// ---- timing -------------------------------------------------------------------------------------------
cellector_status cellector_kernel_time(cellector_ctx *c, cellector_kernel_id which, double *total_ms, uint64_t *launches)
{
    if (!c || which < 0 || which >= CELLECTOR_K_COUNT) return CELLECTOR_EINVAL;
    if (c->multi) return cellector_kernel_time(multi_shard0(c), which, total_ms, launches);
    (void)hipSetDevice(c->device);
    timer_collect(c);
    if (total_ms) *total_ms = c->timers[which].total_ms;
    if (launches) *launches = c->timers[which].launches;
    return CELLECTOR_OK;
}

}  // extern "C"
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

extern "C" {

cellector_status cellector_order_statistics(cellector_ctx *c, const double *keys, uint64_t n, double iqr_multiple, double *out3)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return multi_order_statistics(c, keys, n, iqr_multiple, out3);
    REQUIRE(c, !comm_active(c->comm) || c->comm.n == 1,
            "order statistics on one rank of a communicator: every rank would have to call with its slice");
    return ffi_order_statistics(c, keys, n, n, iqr_multiple, out3);
}

cellector_status cellector_reset_timing(cellector_ctx *c)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return multi_reset_timing(c);
    (void)hipSetDevice(c->device);
    timer_collect(c);
    for (int k = 0; k < CELLECTOR_K_COUNT; k++) { c->timers[k].total_ms = 0.0; c->timers[k].launches = 0; }
    return CELLECTOR_OK;
}

}  // extern "C"
