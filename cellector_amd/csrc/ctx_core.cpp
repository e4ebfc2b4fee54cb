// The core of the C ABI (include/cellector_ffi.h): ctx_fail, the kernel timers, and a ctx's life: create, create_multi, destroy,
// set_stream, device_count, the communicator calls, engine_info, kernel_time, reset_timing.  It drives no kernels_*.hip of its own.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>

#include "ctx.h"
#include "multi.h"

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

// the side stream gets the lowest priority the device offers: its kernels should only fill slots the main stream's
// kernels leave idle
static bool create_side_stream(hipStream_t *out)
{
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) least = 0;
    return hipStreamCreateWithPriority(out, hipStreamNonBlocking, least) == hipSuccess;
}

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

cellector_status cellector_reset_timing(cellector_ctx *c)
{
    if (!c) return CELLECTOR_EINVAL;
    if (c->multi) return multi_reset_timing(c);
    (void)hipSetDevice(c->device);
    timer_collect(c);
    for (int k = 0; k < CELLECTOR_K_COUNT; k++) { c->timers[k].total_ms = 0.0; c->timers[k].launches = 0; }
    return CELLECTOR_OK;
}
