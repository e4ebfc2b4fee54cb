// cellector_write_mtx / cellector_format_mtx: the staged entries as MatrixMarket body lines, made on the device.
//
// A window of entries becomes a window of text in three steps, per file:
//   length  k_mw_length: a block of MW_TILE entries adds up the bytes its lines take (digit counts from compares, mtx_format.h);
//           one u64 per block, and the window's line and both-zero counts on two device counters
//   scan    dev_exclusive_scan_u64 over the block totals only: the block's first byte in the window
//   format  k_mw_format: the lengths again, a block scan of them (per slab of 256 entries, so that neighbouring lanes load
//           neighbouring entries), every thread renders its lines into the block's LDS image at the block-local byte offset; the block then copies the image to the window buffer.  The image starts at the byte
//           (block offset mod 16) of its first 16-byte unit, so that unit u of the image is an aligned unit of the buffer: whole
//           units go out as 16-byte stores, the ragged head and tail units a block shares with its neighbours bytewise.
// Lines are data-dependent in length (6 to 29 bytes) and a dropped entry (SPARSE / DEPTH) has none; nothing outside the window's
// [0, bytes) is written.  The host side windows the entries, copies a window to pinned memory on a second stream while the next
// one is formatted, and writes it from a thread of its own while the one after that is copied (mtx_write_file).
// cellector_write_mtx_bgzf puts kernels_bgzf.hip between the format kernel and the copy: the window's text joins what the window before
// left behind its last whole block (MwBgzf), the whole blocks of the FILE's text become BGZF members, and those are what is copied
// and written; the rest is carried on.  The file's bytes do not depend on the window.
#include <fcntl.h>
#include <unistd.h>

#include <cerrno>
#include <future>

#include "ctx.h"
#include "bgzf_format.h"
#include "mtx_format.h"

#define MW_BLOCK 256
#define MW_ITEMS 4
#define MW_TILE (MW_BLOCK * MW_ITEMS)                // entries of a block: its image is at most 15 + 1024 * 29 bytes
#define MW_IMAGE (((15 + MW_TILE * MTXF_MAX_LINE) + 15) / 16 * 16)
#define MW_WINDOW_DEFAULT (1ull << 23)               // entries of a window: at most 232 MB of text

// the value and length of entry i's line in the file (0: no line)
__device__ __forceinline__ uint32_t mw_entry(const CooView &v, uint64_t i, int which, int mode, uint32_t *locus0, uint32_t *cell0,
                                             uint32_t *value, bool *both_zero)
{
    const uint32_t a = v.alt[i], r = v.ref[i];
    *locus0 = v.locus[i];
    *cell0 = v.cell[i];
    *both_zero = (a | r) == 0;
    return mtxf_value(a, r, which, mode, value) ? mtxf_line_len(*locus0, *cell0, *value) : 0u;
}

// sum over the block, in every thread (MW_BLOCK / 64 waves)
__device__ __forceinline__ uint32_t mw_block_sum(uint32_t x, uint32_t *wsum /*[MW_BLOCK / 64]*/)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    __syncthreads();  // (wsum may still be read from the call before)
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = x;
    __syncthreads();
    uint32_t t = 0;
#pragma unroll
    for (int k = 0; k < MW_BLOCK / 64; k++) t += wsum[k];
    return t;
}

__global__ __launch_bounds__(MW_BLOCK) void k_mw_length(CooView v, int which, int mode, uint64_t *__restrict__ blk_bytes,
                                                        unsigned long long *__restrict__ counters /*[2]: lines, both-zero entries*/)
{
    __shared__ uint32_t wsum[MW_BLOCK / 64];
    const uint64_t base = (uint64_t)blockIdx.x * MW_TILE + threadIdx.x;  // entry base + k * MW_BLOCK: neighbouring lanes, neighbouring entries
    uint32_t bytes = 0, lines = 0, zeros = 0;
#pragma unroll
    for (int k = 0; k < MW_ITEMS; k++) {
        const uint64_t i = base + (uint64_t)k * MW_BLOCK;
        if (i >= v.n) break;
        uint32_t l0, c0, val;
        bool z;
        const uint32_t len = mw_entry(v, i, which, mode, &l0, &c0, &val, &z);
        bytes += len;
        lines += len != 0;
        zeros += z;
    }
    bytes = mw_block_sum(bytes, wsum);
    lines = mw_block_sum(lines, wsum);
    zeros = mw_block_sum(zeros, wsum);
    if (threadIdx.x == 0) {
        blk_bytes[blockIdx.x] = bytes;
        if (lines) atomicAdd(&counters[0], (unsigned long long)lines);
        if (zeros) atomicAdd(&counters[1], (unsigned long long)zeros);
    }
}

__global__ __launch_bounds__(MW_BLOCK) void k_mw_format(CooView v, int which, int mode, uint8_t sep, const uint64_t *__restrict__ blk_off,
                                                        uint8_t *__restrict__ out /*16-byte aligned*/)
{
    __shared__ __attribute__((aligned(16))) uint8_t image[MW_IMAGE];
    __shared__ uint32_t wsum[MW_ITEMS][MW_BLOCK / 64];
    // the block's entries as MW_ITEMS slabs of MW_BLOCK: thread t holds entry t of every slab (neighbouring lanes load neighbouring
    // entries), and the byte offsets come from one scan per slab, the slabs one behind the other
    const uint64_t base = (uint64_t)blockIdx.x * MW_TILE + threadIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t l0[MW_ITEMS], c0[MW_ITEMS], val[MW_ITEMS], len[MW_ITEMS], inc[MW_ITEMS];
#pragma unroll
    for (int k = 0; k < MW_ITEMS; k++) {
        const uint64_t i = base + (uint64_t)k * MW_BLOCK;
        len[k] = 0;
        bool z;
        if (i < v.n) len[k] = mw_entry(v, i, which, mode, &l0[k], &c0[k], &val[k], &z);
        inc[k] = len[k];  // inclusive scan over the wave
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t o = __shfl_up(inc[k], off, 64);
            if (lane >= off) inc[k] += o;
        }
        if (lane == 63) wsum[k][w] = inc[k];
    }
    __syncthreads();
    uint32_t at[MW_ITEMS], total = 0;  // the line's first byte among the block's; the block's bytes
#pragma unroll
    for (int k = 0; k < MW_ITEMS; k++) {
        uint32_t before = 0, slab = 0;
#pragma unroll
        for (int j = 0; j < MW_BLOCK / 64; j++) {
            if (j < w) before += wsum[k][j];
            slab += wsum[k][j];
        }
        at[k] = total + before + (inc[k] - len[k]);
        total += slab;
    }
    if (total == 0) return;  // (a block of dropped entries emits no byte)
    const uint64_t off0 = blk_off[blockIdx.x];
    const uint32_t lead = (uint32_t)(off0 & 15u);  // the image's byte `lead` is the window's byte off0
#pragma unroll
    for (int k = 0; k < MW_ITEMS; k++)
        if (len[k]) mtxf_render(image + lead + at[k], l0[k], c0[k], val[k], sep);
    __syncthreads();
    // image bytes [lead, end) -> window bytes [off0, off0 + total); unit u of the image is the aligned unit at dst + 16 u
    uint8_t *dst = out + (off0 - lead);
    const uint32_t end = lead + total, n_units = (end + 15u) >> 4;
    for (uint32_t u = threadIdx.x; u < n_units; u += MW_BLOCK) {
        const uint32_t b0 = u << 4, lo = b0 < lead ? lead : b0, hi = b0 + 16u < end ? b0 + 16u : end;
        if (hi - lo == 16u) {
            *reinterpret_cast<uint4 *>(dst + b0) = *reinterpret_cast<const uint4 *>(image + b0);
        } else {
            for (uint32_t b = lo; b < hi; b++) dst[b] = image[b];
        }
    }
}

// ---- a window on the device ---------------------------------------------------------------------------------------------------
struct MwScratch {
    DevBuf<uint64_t> blk;                  // [blocks of a window + 1] byte counts, then offsets
    DevBuf<unsigned long long> counters;   // [2]
    uint64_t window = 0;                   // entries the scratch serves
    // CELLECTOR_TIMING=1: the two kernels' GPU time between events, summed over the windows (the format kernel is then awaited)
    bool timed = false;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    double ms_length = 0, ms_format = 0;
    ~MwScratch()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

static cellector_status mw_scratch(cellector_ctx *c, MwScratch *s, uint64_t window)
{
    s->window = window;
    CHK(dev_alloc(c, &s->blk, (window + MW_TILE - 1) / MW_TILE + 1));
    if (getenv("CELLECTOR_TIMING")) {
        for (hipEvent_t &e : s->ev) HIPCHK(c, hipEventCreate(&e));
        s->timed = true;
    }
    return dev_alloc(c, &s->counters, 2);
}

// The lines of the entries v (at most s->window) in file `which`: their bytes, lines and both-zero entries; with `out` (a device
// buffer of at least 29 bytes per entry, 16-byte aligned) also the text.  The format kernel is queued, not awaited.
static cellector_status mw_window(cellector_ctx *c, MwScratch *s, const CooView &v, int which, int mode, uint8_t sep, uint8_t *out,
                                  uint64_t *bytes, uint64_t *lines, uint64_t *zeros)
{
    *bytes = *lines = *zeros = 0;
    if (v.n == 0) return CELLECTOR_OK;
    const uint64_t nb = (v.n + MW_TILE - 1) / MW_TILE;
    HIPCHK(c, hipMemsetAsync(s->counters, 0, 16, c->stream));
    HIPCHK(c, hipMemsetAsync(s->blk + nb, 0, 8, c->stream));
    if (s->timed) HIPCHK(c, hipEventRecord(s->ev[0], c->stream));
    hipLaunchKernelGGL(k_mw_length, dim3((unsigned)nb), dim3(MW_BLOCK), 0, c->stream, v, which, mode, s->blk.get(), s->counters.get());
    HIPCHK(c, hipGetLastError());
    if (s->timed) HIPCHK(c, hipEventRecord(s->ev[1], c->stream));
    unsigned long long cnt[2];
    HIPCHK(c, hipMemcpyAsync(cnt, s->counters, 16, hipMemcpyDeviceToHost, c->stream));
    CHK(dev_exclusive_scan_u64(c, s->blk, nb + 1, bytes));  // (synchronises: cnt has arrived)
    *lines = cnt[0];
    *zeros = cnt[1];
    float ms = 0;
    if (s->timed && hipEventElapsedTime(&ms, s->ev[0], s->ev[1]) == hipSuccess) s->ms_length += ms;
    if (out && *bytes) {
        if (s->timed) HIPCHK(c, hipEventRecord(s->ev[2], c->stream));
        hipLaunchKernelGGL(k_mw_format, dim3((unsigned)nb), dim3(MW_BLOCK), 0, c->stream, v, which, mode, sep, (const uint64_t *)s->blk.get(), out);
        HIPCHK(c, hipGetLastError());
        if (s->timed) {
            HIPCHK(c, hipEventRecord(s->ev[3], c->stream));
            HIPCHK(c, hipEventSynchronize(s->ev[3]));
            if (hipEventElapsedTime(&ms, s->ev[2], s->ev[3]) == hipSuccess) s->ms_format += ms;
        }
    }
    return CELLECTOR_OK;
}

static CooView mw_slice(const cellector_ctx *c, uint64_t first, uint64_t n)
{
    return {c->coo.locus + first, c->coo.cell + first, c->coo.alt + first, c->coo.ref + first, n};
}

uint64_t mtx_write_window(const cellector_ctx *c) { return c->write_window_opt > 0 ? (uint64_t)c->write_window_opt : MW_WINDOW_DEFAULT; }

// cellector_format_mtx behind its checks: counts alone (out null), or the text of the range into host memory
cellector_status mtx_format_range(cellector_ctx *c, int which, int mode, uint8_t sep, uint64_t first, uint64_t n, uint8_t *out,
                                  uint64_t capacity, uint64_t *n_bytes, uint64_t *n_lines)
{
    const uint64_t W = mtx_write_window(c), w_cap = n < W ? n : W;
    MwScratch s;
    CHK(mw_scratch(c, &s, w_cap));
    uint64_t bytes = 0, lines = 0;
    for (uint64_t at = 0; at < n; at += W) {
        uint64_t b, l, z;
        CHK(mw_window(c, &s, mw_slice(c, first + at, n - at < W ? n - at : W), which, mode, sep, nullptr, &b, &l, &z));
        bytes += b;
        lines += l;
    }
    *n_bytes = bytes;
    *n_lines = lines;
    if (!out) return CELLECTOR_OK;
    if (capacity < bytes)
        return ctx_fail(c, CELLECTOR_EINVAL, "format_mtx: capacity %llu is below the %llu bytes of the range", (unsigned long long)capacity,
                        (unsigned long long)bytes);
    DevBuf<uint8_t> text;
    CHK(dev_alloc(c, &text, w_cap * MTXF_MAX_LINE + 16));
    uint64_t done = 0;
    for (uint64_t at = 0; at < n; at += W) {
        uint64_t b, l, z;
        CHK(mw_window(c, &s, mw_slice(c, first + at, n - at < W ? n - at : W), which, mode, sep, text, &b, &l, &z));
        CHK(d2h(c, out + done, text, b));  // (exactly the window's bytes: nothing behind n_bytes is touched)
        done += b;
    }
    return CELLECTOR_OK;
}

// ---- a file ---------------------------------------------------------------------------------------------------------------------
// 0, or the errno of the write that failed (the caller may be another thread than the one that reports it)
static int write_all(int fd, const uint8_t *p, uint64_t n)
{
    while (n) {
        const ssize_t k = write(fd, p, n < (1ull << 30) ? n : (1ull << 30));
        if (k < 0 && errno == EINTR) continue;
        if (k < 0) return errno;
        if (k == 0) return EIO;
        p += k;
        n -= (uint64_t)k;
    }
    return 0;
}

// the two pinned buffers, the two device buffers, the copy stream and its events of one cellector_write_mtx call
struct MwPipe {
    DevBuf<uint8_t> dev[2];
    uint8_t *host[2] = {nullptr, nullptr};
    hipStream_t copy = nullptr;
    hipEvent_t formatted[2] = {nullptr, nullptr}, copied[2] = {nullptr, nullptr};
    ~MwPipe()
    {
        for (int b = 0; b < 2; b++) {
            if (host[b]) (void)hipHostFree(host[b]);
            if (formatted[b]) (void)hipEventDestroy(formatted[b]);
            if (copied[b]) (void)hipEventDestroy(copied[b]);
        }
        if (copy) (void)hipStreamDestroy(copy);
    }
};

static cellector_status mw_pipe(cellector_ctx *c, MwPipe *p, uint64_t cap /*bytes of a buffer*/)
{
    for (int b = 0; b < 2; b++) {
        CHK(dev_alloc(c, &p->dev[b], cap));
        if (hipHostMalloc((void **)&p->host[b], cap) != hipSuccess) {
            p->host[b] = nullptr;
            return ctx_fail(c, CELLECTOR_ENOMEM, "write_mtx: no pinned buffer of %llu bytes", (unsigned long long)cap);
        }
        HIPCHK(c, hipEventCreateWithFlags(&p->formatted[b], hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&p->copied[b], hipEventDisableTiming));
    }
    HIPCHK(c, hipStreamCreateWithFlags(&p->copy, hipStreamNonBlocking));
    return CELLECTOR_OK;
}

// The text of one file on its way into BGZF blocks.  Blocks are cut at multiples of BGZF_PAYLOAD in the file's text: the header lines
// go in front of the first window's text, and the ragged tail a window leaves (below BGZF_PAYLOAD bytes) is moved to the front of
// the buffer for the next one by a device copy.
#define MW_HEAD_MAX 160
struct MwBgzf {
    BzScratch scratch;
    DevBuf<uint8_t> stage;  // a window's text as k_mw_format writes it (16-byte aligned)
    DevBuf<uint8_t> text;   // what is carried | the window's text
    uint64_t fill = 0;      // bytes in `text`
    uint64_t file_bytes = 0, blocks = 0, stored = 0;  // of the file being written, so far
};

static uint64_t mwz_text_capacity(uint64_t w_cap) { return BGZF_PAYLOAD + MW_HEAD_MAX + w_cap * MTXF_MAX_LINE + 16; }

static cellector_status mwz_init(cellector_ctx *c, MwBgzf *z, uint64_t w_cap)
{
    CHK(bz_scratch(c, &z->scratch, bz_blocks(mwz_text_capacity(w_cap))));
    CHK(dev_alloc(c, &z->stage, w_cap * MTXF_MAX_LINE + 16));
    return dev_alloc(c, &z->text, mwz_text_capacity(w_cap));
}

// m bytes from the host (the header lines) or from z->stage (a window) join the text; its whole blocks (all of it with `flush`) go to
// `out` as members, the rest to the front.  Queued on c->stream behind the format kernel; the compaction is not awaited.
static cellector_status mwz_push(cellector_ctx *c, MwBgzf *z, const void *host_src, uint64_t m, bool flush, uint8_t *out, uint64_t *out_bytes)
{
    *out_bytes = 0;
    if (m) HIPCHK(c, hipMemcpyAsync(z->text + z->fill, host_src ? host_src : (const void *)z->stage.get(), m,
                                    host_src ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->stream));
    z->fill += m;
    if (!out) return CELLECTOR_OK;
    const uint64_t take = flush ? z->fill : z->fill / BGZF_PAYLOAD * BGZF_PAYLOAD, rest = z->fill - take;
    uint64_t blocks = 0, stored = 0;
    CHK(bz_compress(c, &z->scratch, z->text, take, out, out_bytes, &blocks, &stored));
    // (take >= BGZF_PAYLOAD > rest: the two ranges do not overlap)
    if (rest && take) HIPCHK(c, hipMemcpyAsync(z->text, z->text + take, rest, hipMemcpyDeviceToDevice, c->stream));
    z->fill = rest;
    z->file_bytes += *out_bytes;
    z->blocks += blocks;
    z->stored += stored;
    return CELLECTOR_OK;
}

// One file: header, then the windows.  Window w is formatted into device buffer w & 1 while window w - 1 is copied to its pinned
// buffer on the copy stream and window w - 2 is written by a thread of its own; a buffer is taken again only after its copy and
// its write have ended.  `count` is the size line's third number.  Nothing is removed on a failure.  With z the file is the BGZF
// stream of that text: a window's step compresses the text's whole blocks so far, one more step flushes the rest, and the EOF member
// follows; file_bytes stays the size of the TEXT (z->file_bytes is the file's).
static cellector_status mtx_write_file(cellector_ctx *c, MwScratch *s, MwPipe *p, MwBgzf *z, const char *path, int which, int mode, uint8_t sep,
                                       uint64_t count, uint64_t *file_bytes, uint64_t *file_lines, uint64_t *zeros, uint64_t *n_windows,
                                       double *phase_s /*[3]: format, wait for copies, wait for writes; may be null*/)
{
    const int fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (fd < 0) return ctx_fail(c, CELLECTOR_EIO, "write_mtx: cannot create %s: %s", path, strerror(errno));
    char head[160];
    const int hn = snprintf(head, sizeof head, "%%%%MatrixMarket matrix coordinate real general\n%% written by sprs\n%llu%c%llu%c%llu\n",
                            (unsigned long long)c->total_loci, (char)sep, (unsigned long long)c->total_cells, (char)sep, (unsigned long long)count);
    cellector_status st = CELLECTOR_OK;
    int io_err = 0;
    uint64_t none = 0;
    if (z) {
        z->fill = z->file_bytes = z->blocks = z->stored = 0;
        st = mwz_push(c, z, head, (uint64_t)hn, false, nullptr, &none);
    } else {
        io_err = write_all(fd, (const uint8_t *)head, (uint64_t)hn);
    }
    const uint64_t n = c->coo.n, W = mtx_write_window(c), n_win = (n + W - 1) / W, n_steps = n_win + (z ? 1 : 0);
    uint64_t bytes_of[2] = {0, 0}, total = (uint64_t)hn, lines = 0, zz = 0, nw = 0;  // nw: steps taken
    std::future<int> writing;  // the write of the window before the last one copied
    LapTimer lt;
    auto lap = [&](int k) { const double d = lt.lap(); if (phase_s) phase_s[k] += d; };
    auto join_write = [&]() {
        if (!writing.valid()) return;
        const int e = writing.get();
        if (e && !io_err) io_err = e;
    };
    auto hand_to_writer = [&](int b) {  // window in pinned buffer b: copied -> written
        hipError_t e = hipEventSynchronize(p->copied[b]);
        lap(1);
        if (e != hipSuccess) { st = ctx_fail(c, CELLECTOR_EDEVICE, "write_mtx: %s", hipGetErrorString(e)); return; }
        const uint8_t *src = p->host[b];
        const uint64_t m = bytes_of[b];
        writing = std::async(std::launch::async, [fd, src, m]() { return write_all(fd, src, m); });
    };
    for (; nw < n_steps && st == CELLECTOR_OK && !io_err; nw++) {
        const int b = (int)(nw & 1);
        const uint64_t at = nw * W;
        uint64_t text = 0, l = 0, zeros_here = 0;
        if (nw < n_win)
            st = mw_window(c, s, mw_slice(c, at, n - at < W ? n - at : W), which, mode, sep, z ? z->stage.get() : p->dev[b].get(), &text, &l,
                           &zeros_here);
        bytes_of[b] = text;
        if (z && st == CELLECTOR_OK) st = mwz_push(c, z, nullptr, text, nw == n_win, p->dev[b], &bytes_of[b]);
        lap(0);
        if (st != CELLECTOR_OK) break;
        total += text; lines += l; zz += zeros_here;
        join_write();  // (window nw - 2 has left pinned buffer b)
        lap(2);
        hipError_t e = hipEventRecord(p->formatted[b], c->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(p->copy, p->formatted[b], 0);
        if (e == hipSuccess && bytes_of[b]) e = hipMemcpyAsync(p->host[b], p->dev[b], bytes_of[b], hipMemcpyDeviceToHost, p->copy);
        if (e == hipSuccess) e = hipEventRecord(p->copied[b], p->copy);
        if (e != hipSuccess) { st = ctx_fail(c, CELLECTOR_EDEVICE, "write_mtx: %s", hipGetErrorString(e)); break; }
        if (nw > 0) hand_to_writer(b ^ 1);
    }
    if (nw > 0 && st == CELLECTOR_OK && !io_err) {
        join_write();
        lap(2);
        hand_to_writer((int)((nw - 1) & 1));
    }
    join_write();
    lap(2);
    // (nothing of this call may still be in flight when its buffers go)
    (void)hipStreamSynchronize(p->copy);
    (void)hipStreamSynchronize(c->stream);
    if (z && st == CELLECTOR_OK && !io_err) {
        io_err = write_all(fd, BGZF_EOF, BGZF_EOF_BYTES);
        z->file_bytes += BGZF_EOF_BYTES;
    }
    if (close(fd) != 0 && !io_err) io_err = errno ? errno : EIO;
    if (st == CELLECTOR_OK && io_err) st = ctx_fail(c, CELLECTOR_EIO, "write_mtx: cannot write %s: %s", path, strerror(io_err));
    *file_bytes = total;
    *file_lines = lines;
    *zeros = zz;
    *n_windows = nw < n_win ? nw : n_win;
    return st;
}

// cellector_write_mtx (gz null) / cellector_write_mtx_bgzf behind their checks
cellector_status mtx_write_pair(cellector_ctx *c, const char *first_path, const char *second_path, int mode, uint32_t flags,
                                cellector_write_summary *sum, cellector_write_bgzf_summary *gz)
{
    const uint8_t sep = (flags & CELLECTOR_MTX_SPACE) ? ' ' : '\t';
    const uint64_t n = c->coo.n, W = mtx_write_window(c), w_cap = n < W ? n : W;
    MwScratch s;
    MwPipe p;
    MwBgzf z;
    CHK(mw_scratch(c, &s, w_cap));
    if (gz) CHK(mwz_init(c, &z, w_cap));
    CHK(mw_pipe(c, &p, gz ? bz_out_capacity(z.scratch.cap_blocks) : w_cap * MTXF_MAX_LINE + 16));
    cellector_write_bgzf_summary zout = {};
    const bool timing = getenv("CELLECTOR_TIMING") != nullptr;
    double phase[3] = {0, 0, 0};
    cellector_write_summary out = {};
    out.n_entries = n;
    for (int which = 0; which < 2; which++) {
        // the size line's count: 0 as the combiner writes it, or the file's lines, which the dropping modes know only after a
        // length pass over every window
        uint64_t count = 0;
        if (!(flags & CELLECTOR_MTX_HEADER_ZERO)) {
            count = n;
            if (mode != CELLECTOR_WRITE_ALIGNED) {
                count = 0;
                for (uint64_t at = 0; at < n; at += W) {
                    uint64_t b, l, z;
                    CHK(mw_window(c, &s, mw_slice(c, at, n - at < W ? n - at : W), which, mode, sep, nullptr, &b, &l, &z));
                    count += l;
                }
            }
        }
        uint64_t zeros = 0, nw = 0;
        const cellector_status st = mtx_write_file(c, &s, &p, gz ? &z : nullptr, which ? second_path : first_path, which, mode, sep, count,
                                                   which ? &out.bytes_second : &out.bytes_first, which ? &out.lines_second : &out.lines_first,
                                                   &zeros, &nw, timing ? phase : nullptr);
        out.n_windows = nw;
        out.n_dropped_keys = zeros;  // (the entries with alt = ref = 0, whichever file counted them; ALIGNED writes them)
        (which ? zout.file_bytes_second : zout.file_bytes_first) = z.file_bytes;
        (which ? zout.blocks_second : zout.blocks_first) = z.blocks;
        zout.stored_blocks += z.stored;
        if (st != CELLECTOR_OK) return st;
    }
    if (timing)
        fprintf(stderr, "[timing]   write_mtx: %llu entries, %llu windows per file: format %.4f s (length kernels %.3f ms, format kernels %.3f ms), "
                        "waiting for copies %.4f s, for writes %.4f s\n",
                (unsigned long long)n, (unsigned long long)out.n_windows, phase[0], s.ms_length, s.ms_format, phase[1], phase[2]);
    if (timing && gz)
        fprintf(stderr, "[timing]   write_mtx_bgzf: %llu + %llu bytes of text in %llu + %llu blocks (%llu stored) -> %llu + %llu bytes: "
                        "block kernels %.3f ms, compaction kernels %.3f ms\n",
                (unsigned long long)out.bytes_first, (unsigned long long)out.bytes_second, (unsigned long long)zout.blocks_first,
                (unsigned long long)zout.blocks_second, (unsigned long long)zout.stored_blocks, (unsigned long long)zout.file_bytes_first,
                (unsigned long long)zout.file_bytes_second, z.scratch.ms_block, z.scratch.ms_compact);
    if (sum) *sum = out;
    if (gz) {
        zout.text = out;
        *gz = zout;
    }
    return CELLECTOR_OK;
}
