// Device-side parse of the vartrix alt.mtx / ref.mtx text (rows A1 and f2 of the scope table).
//
// The host only brings bytes (mmap for plain files, zlib inflate for ".gz", multi-member) and reads the three header
// lines (mtx_bytes.cpp); the data lines are tokenised and converted on the GPU:
//   k_nl_count               newlines per 128-byte segment, scanned: the index of the first line that starts in a segment;
//   k_parse_lines            a thread per segment, for every line that starts there: split_whitespace + parse::<usize>() of the tokens the reference reads
//                            (load_data.rs:190-204): alt file tokens 0,1,2 (locus, cell, alt count), ref file token 2 only
//                            (its indices are never read); any failure records the smallest offending line;
//   k_pair_check / k_pair_fill   zip the two files (shorter one wins, like izip!), range checks, this shard's cell range,
//                            ordered compaction into the staged COO (locus u32, cell_local u32, alt u16, ref u16).
// The text contract is the reference's; errors come back as CELLECTOR_EPARSE / CELLECTOR_EINVAL with the line number.
#include <condition_variable>
#include <mutex>
#include <thread>

#include "ctx.h"
#include "device_math.h"
#include "mtx_bytes.h"

#define PB 256

__device__ __forceinline__ bool is_ws(uint8_t ch)
{
    return ch == ' ' || ch == '\t' || ch == '\r' || ch == '\n' || ch == '\f' || ch == '\v';
}

// ---- line starts ----------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t newline_mask16(const uint8_t *__restrict__ text, uint64_t n, uint64_t base)
{
    uint32_t m = 0;
    if (base + 16 <= n) {
        const uint4 v = *reinterpret_cast<const uint4 *>(text + base);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int b = 0; b < 4; b++)
                if (((w[q] >> (8 * b)) & 0xffu) == '\n') m |= 1u << (4 * q + b);
    } else {
        for (uint64_t i = base; i < n; i++)
            if (text[i] == '\n') m |= 1u << (uint32_t)(i - base);
    }
    return m;
}

// (a thread takes NL_SEG bytes = 8 units of 16: the count array is 1/16 of the text instead of 1/2 — at 30 GB of text per
// file that is 15 GB of VRAM less to map)
#define NL_SEG 128
__global__ __launch_bounds__(PB) void k_nl_count(const uint8_t *__restrict__ text, uint64_t n, uint64_t *__restrict__ cnt)
{
    const uint64_t t = (uint64_t)blockIdx.x * PB + threadIdx.x;
    const uint64_t base = t * NL_SEG;
    if (base >= n) return;
    uint32_t k = 0;
#pragma unroll
    for (int u = 0; u < NL_SEG / 16; u++)
        if (base + 16 * u < n) k += __popc(newline_mask16(text, n, base + 16 * u));
    cnt[t] = k;
}

// ---- tokens ---------------------------------------------------------------------------------------------------
// parse token `idx` of [p, e) as an unsigned integer (optional leading '+'); false on missing / malformed / > 2^32-1
// parse tokens first_idx .. first_idx + n_tok - 1 of the LINE that starts at p (it ends at the next '\n'; e bounds the text)
// as unsigned integers (optional leading '+'); false on a missing / malformed token or a value above 2^32-1
__device__ bool token_u32(const uint8_t *__restrict__ p, const uint8_t *__restrict__ e, int first_idx, int n_tok,
                          uint32_t *out)
{
    int t = 0;
    while (true) {
        while (p < e && *p != '\n' && is_ws(*p)) p++;
        if (p >= e || *p == '\n') return false;
        const uint8_t *s = p;
        while (p < e && !is_ws(*p)) p++;
        if (t >= first_idx) {
            if (*s == '+') s++;
            if (s == p) return false;
            uint64_t v = 0;
            for (; s < p; s++) {
                if (*s < '0' || *s > '9') return false;
                v = v * 10 + (uint64_t)(*s - '0');
                if (v > 0xffffffffull) return false;
            }
            out[t - first_idx] = (uint32_t)v;
            if (t - first_idx + 1 == n_tok) return true;
        }
        t++;
    }
}

// ALT file: tokens 0,1,2 -> (locus1, cell1, count); REF file: token 2 -> count.  A thread takes the lines that START in its
// NL_SEG bytes (line 0 at byte 0, line k after the k-th newline; off[t] = newlines before the segment, from the scan of
// k_nl_count) — no array of line starts is ever materialised (at 2e9 lines per file that array was 16 GB of VRAM each).
#define PARSE_TAIL 64  // bytes staged beyond the block's segments: a line that starts near the end finishes in there
// Windowed use (big files, parse_windowed below): `text` is one window of the data section plus look-ahead bytes, n_count
// the bytes whose newlines belong to this window, line_base the number of newlines before the window, first = the window
// starts at the first data byte (line 0 has no newline before it), more = the file goes on beyond the n bytes given.
template <bool ALT>
__global__ __launch_bounds__(PB) void k_parse_lines(const uint8_t *__restrict__ text, uint64_t n, uint64_t n_count, uint64_t n_lines,
                                                    uint64_t line_base, bool first, bool more,
                                                    const uint64_t *__restrict__ off, uint32_t *__restrict__ o0,
                                                    uint32_t *__restrict__ o1, uint32_t *__restrict__ o2,
                                                    unsigned long long *__restrict__ first_bad)
{
    // the block's PB segments (+ a tail) go through LDS: coalesced 16-byte loads instead of byte-wise global reads
    __shared__ __attribute__((aligned(16))) uint8_t s_text[PB * NL_SEG + PARSE_TAIL];
    const uint64_t blk = (uint64_t)blockIdx.x * PB * NL_SEG;
    const uint64_t avail = blk < n ? min((uint64_t)(PB * NL_SEG + PARSE_TAIL), n - blk) : 0;  // text has 16 bytes of padding
    for (uint32_t i = threadIdx.x * 16; i < avail; i += PB * 16)
        *reinterpret_cast<uint4 *>(s_text + i) = *reinterpret_cast<const uint4 *>(text + blk + i);
    __syncthreads();
    const uint64_t t = (uint64_t)blockIdx.x * PB + threadIdx.x;
    const uint64_t base = t * NL_SEG;
    if (base >= n_count) return;
    auto line = [&](uint64_t i, uint64_t start) {
        if (i >= n_lines || start >= n) return;
        uint32_t v[3] = {0, 0, 0};
        // inside the staged window (a line is far shorter than the tail) parse from LDS, else from the text itself
        const uint64_t rel = start - blk;
        const uint8_t *p = text + start, *e = text + n;
        bool closed = false;
        if (rel + PARSE_TAIL <= avail) {
            const uint8_t *q = s_text + rel, *qe = q + PARSE_TAIL;
            for (const uint8_t *z = q; z < qe; z++)
                if (*z == '\n') { closed = true; break; }
            if (closed) { p = q; e = qe; }
        }
        if (!closed && more) {  // a line that runs out of the window's look-ahead: not supported (PW_LOOK bytes)
            for (const uint8_t *z = p; z < e; z++)
                if (*z == '\n') { closed = true; break; }
            if (!closed) {
                atomicMin(first_bad, (unsigned long long)i);
                return;
            }
        }
        const bool ok = ALT ? token_u32(p, e, 0, 3, v) : token_u32(p, e, 2, 1, v);
        if (!ok) {
            atomicMin(first_bad, (unsigned long long)i);
            return;
        }
        if (ALT) { o0[i] = v[0]; o1[i] = v[1]; o2[i] = v[2]; } else o2[i] = v[0];
    };
    if (t == 0 && first) line(line_base, 0);
    uint64_t k = line_base + off[t];
    for (int u = 0; u < NL_SEG / 16; u++) {
        const uint64_t ub = base + 16 * u;
        if (ub >= n_count) break;
        uint32_t m = newline_mask16(text, n_count, ub);
        while (m) {
            const int b = __ffs((int)m) - 1;
            m &= m - 1;
            line(++k, ub + b + 1);
        }
    }
}

// ---- zip, validate, shard filter ------------------------------------------------------------------------------
enum { PE_NONE = 0, PE_INDEX0 = 1, PE_LOCUS = 2, PE_CELL = 3, PE_COUNT = 4 };
#define PE_KIND_BITS 3  // k_pair_check reports (entry << PE_KIND_BITS) | kind: the minimum is the smallest entry, with ITS kind
static const char *const pe_what[] = {"", "index 0 (indices are 1-based)", "locus index out of range", "cell index out of range",
                                      "count above 65535 not supported"};
inline const char *pe_kind_text(unsigned long long packed)
{
    const unsigned kind = (unsigned)(packed & ((1u << PE_KIND_BITS) - 1));
    return pe_what[kind <= PE_COUNT ? kind : 0];
}

__global__ __launch_bounds__(PB) void k_pair_check(uint64_t n, const uint32_t *__restrict__ l1, const uint32_t *__restrict__ c1,
                                                   const uint32_t *__restrict__ a, const uint32_t *__restrict__ r,
                                                   uint64_t total_loci, uint64_t total_cells, uint64_t cb, uint64_t ce,
                                                   uint64_t *__restrict__ keep, unsigned long long *__restrict__ first_bad,
                                                   uint32_t *__restrict__ unsorted)
{
    const uint64_t i = (uint64_t)blockIdx.x * PB + threadIdx.x;
    if (i > n) return;
    if (i == n) { if (keep) keep[i] = 0; return; }
    uint32_t kind = PE_NONE;
    if (l1[i] == 0 || c1[i] == 0) kind = PE_INDEX0;          // `tok - 1` underflows in the reference
    else if (l1[i] > total_loci) kind = PE_LOCUS;
    else if (c1[i] > total_cells) kind = PE_CELL;
    else if (a[i] > CELLECTOR_MAX_COUNT || r[i] > CELLECTOR_MAX_COUNT) kind = PE_COUNT;
    if (kind != PE_NONE) {
        atomicMin(first_bad, ((unsigned long long)i << PE_KIND_BITS) | kind);  // entry and kind in one word: the smallest entry's own kind
        if (keep) keep[i] = 0;
        return;
    }
    const uint64_t c0 = c1[i] - 1;
    const bool mine = c0 >= cb && c0 < ce;
    if (keep) keep[i] = mine ? 1 : 0;  // (null: the shard holds every cell, every valid entry stays where it is)
    if (i + 1 < n && l1[i + 1] < l1[i]) *unsorted = 1;  // file order not locus-major (all entries, a superset check)
}

__global__ __launch_bounds__(PB) void k_pair_fill(uint64_t n, const uint32_t *__restrict__ l1, const uint32_t *__restrict__ c1,
                                                  const uint32_t *__restrict__ a, const uint32_t *__restrict__ r, uint64_t cb,
                                                  uint64_t ce, const uint64_t *__restrict__ pos, uint32_t *__restrict__ o_locus,
                                                  uint32_t *__restrict__ o_cell, uint16_t *__restrict__ o_alt,
                                                  uint16_t *__restrict__ o_ref)
{
    const uint64_t i = (uint64_t)blockIdx.x * PB + threadIdx.x;
    if (i >= n) return;
    const uint64_t c0 = (uint64_t)c1[i] - 1;
    if (c1[i] == 0 || c0 < cb || c0 >= ce) return;
    const uint64_t p = pos[i];
    o_locus[p] = l1[i] - 1;
    o_cell[p] = (uint32_t)(c0 - cb);
    o_alt[p] = (uint16_t)a[i];
    o_ref[p] = (uint16_t)r[i];
}

// a shard that holds every cell: the token arrays BECOME the staged COO (indices made 0-based in place, counts narrowed
// into two new u16 arrays) — no keep flags, no scan, no second copy of the indices: 32 GB less fresh VRAM at 2e9 entries
__global__ __launch_bounds__(PB) void k_pair_take(uint64_t n, uint32_t *__restrict__ l1, uint32_t *__restrict__ c1,
                                                  const uint32_t *__restrict__ a, const uint32_t *__restrict__ r,
                                                  uint16_t *__restrict__ o_alt, uint16_t *__restrict__ o_ref)
{
    const uint64_t i = (uint64_t)blockIdx.x * PB + threadIdx.x;
    if (i >= n) return;
    l1[i] -= 1;
    c1[i] -= 1;
    o_alt[i] = (uint16_t)a[i];
    o_ref[i] = (uint16_t)r[i];
}

// ===============================================================================================================
namespace {

struct DevText {
    DevBuf<uint8_t> text;
    uint64_t lead = 0;  // the data section starts this far into `text` (a multiple of 16; not 0 only for a file inflated on the device)
    uint8_t *at() const { return text.get() + lead; }
    uint64_t n = 0, n_lines = 0;
    DevBuf<uint64_t> seg_off;  // newlines before each NL_SEG-byte segment (exclusive scan of k_nl_count)
    uint64_t n_seg = 0;
};

inline unsigned pgrid(uint64_t n) { return (unsigned)((n + PB - 1) / PB ? (n + PB - 1) / PB : 1); }

// bytes of the data section -> device.  A plain hipMemcpy out of the mapped file is staged by ONE runtime thread and
// swings between 8 and 25 GB/s from box to box (where the page cache sits relative to the GPU); here UP_THREADS host
// threads copy each piece into one of two pinned buffers while the previous piece is on its way over PCIe.
#define UP_PIECE (256ull << 20)
#define UP_THREADS 8
#define UP_MIN (4ull << 30)
// one timing line of a file inflated on the device (CELLECTOR_TIMING=1)
void inf_report(const InfScratch &s, const FileBytes &fb)
{
    if (s.timed)
        fprintf(stderr, "[timing]     inflate on the device: %s: %llu members, %llu -> %llu bytes, inflate kernel %.3f ms\n", fb.path.c_str(),
                (unsigned long long)s.n_members, (unsigned long long)s.bytes_in, (unsigned long long)s.bytes_out, s.ms_kernel);
}

// ... of a BGZF file left compressed (option gz_device): the compressed bytes from the first member that holds data-section text to
// the end go up in pieces of inf_chunk_members() members, and k_bgzf_inflate writes their text straight into dt->text, at the offset
// that puts the data section's first byte at dt->at()[0] (the header's tail in that first member lands in the `lead` bytes before).
// *refused: a member the device does not accept (the caller hands the file to the host reader).
cellector_status upload_text_gz(cellector_ctx *c, const FileBytes &fb, size_t data_off, DevText *dt, bool *refused)
{
    HIPCHK(c, hipSetDevice(c->device));
    dt->n = fb.size - data_off;
    const uint64_t nb = fb.blocks.size(), k_first = dt->n ? fb.member_at(data_off) : nb;
    const uint64_t before = dt->n ? data_off - fb.blocks[k_first].out : 0;  // text of that member in front of the data section
    dt->lead = (before + 15) & ~15ull;
    CHK(dev_alloc(c, &dt->text, dt->lead + dt->n + 16));
    HIPCHK(c, hipMemsetAsync(dt->at() + dt->n, '\n', 16, c->stream));
    if (!dt->n) return CELLECTOR_OK;
    const uint64_t chunk = inf_chunk_members(), out_first = fb.blocks[k_first].out;
    uint64_t max_in = 0;
    for (uint64_t k0 = k_first; k0 < nb; k0 += chunk) {
        const uint64_t k1 = std::min(nb, k0 + chunk);
        max_in = std::max<uint64_t>(max_in, fb.blocks[k1 - 1].off + fb.blocks[k1 - 1].clen - fb.blocks[k0].off);
    }
    InfScratch s;
    DevBuf<uint8_t> d_in;
    CHK(inf_scratch(c, &s, std::min(chunk, nb - k_first)));
    CHK(dev_alloc(c, &d_in, max_in));
    std::vector<InfMember> table(s.cap_members);
    for (uint64_t k0 = k_first; k0 < nb; k0 += chunk) {
        const uint64_t k1 = std::min(nb, k0 + chunk);
        const uint64_t in_first = fb.blocks[k0].off, n_in = fb.blocks[k1 - 1].off + fb.blocks[k1 - 1].clen - in_first;
        HIPCHK(c, hipMemcpyAsync(d_in, fb.gz + in_first, n_in, hipMemcpyHostToDevice, c->stream));
        // (every member's place is relative to the first member's text; the kernel checks it against the bytes behind that)
        CHK(inf_launch(c, &s, c->stream, fb.blocks, k0, k1, table.data(), fb.gz, d_in, in_first, n_in, dt->at() - before, out_first,
                       fb.size - out_first, false));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        inf_launch_timed(&s);
        if (*s.h_status != ~0ull) {
            *refused = true;
            return inf_refused(c, fb.path.c_str(), *s.h_status);
        }
    }
    s.bytes_out = fb.size - out_first;
    inf_report(s, fb);
    return CELLECTOR_OK;
}

cellector_status upload_text(cellector_ctx *c, const FileBytes &fb, size_t data_off, DevText *dt)
{
    HIPCHK(c, hipSetDevice(c->device));
    dt->n = fb.size - data_off;
    // a final line without '\n' still counts (BufRead::lines); normalise by treating the end of data as a terminator
    CHK(dev_alloc(c, &dt->text, dt->n + 16));
    // (everything below is ordered on the ctx's stream, which may be a non-blocking one: no null-stream calls)
    HIPCHK(c, hipMemsetAsync(dt->text + dt->n, '\n', 16, c->stream));
    if (dt->n < UP_MIN) {  // pinning the two buffers costs ~0.1 s: only worth it for multi-GB files
        const size_t piece = 1ull << 30;
        for (size_t o = 0; o < dt->n; o += piece)
            HIPCHK(c, hipMemcpyAsync(dt->text + o, fb.data + data_off + o, std::min(piece, (size_t)dt->n - o), hipMemcpyHostToDevice,
                                     c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return CELLECTOR_OK;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (the padding is in place before the upload stream's copies are consumed)
    uint8_t *pin[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipStream_t up = nullptr;
    hipError_t e = hipStreamCreateWithFlags(&up, hipStreamNonBlocking);
    for (int b = 0; b < 2 && e == hipSuccess; b++) {
        e = hipHostMalloc((void **)&pin[b], UP_PIECE);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ev[b], hipEventDisableTiming);
    }
    const uint8_t *src = fb.data + data_off;
    uint64_t piece = 0;
    for (size_t o = 0; o < dt->n && e == hipSuccess; o += UP_PIECE, piece++) {
        const int b = (int)(piece & 1);
        const size_t len = std::min((size_t)UP_PIECE, (size_t)dt->n - o);
        if (piece >= 2) e = hipEventSynchronize(ev[b]);  // the copy that last read this buffer is done
        if (e != hipSuccess) break;
        std::thread th[UP_THREADS];
        const size_t slice = (len + UP_THREADS - 1) / UP_THREADS;
        for (int t = 0; t < UP_THREADS; t++)
            th[t] = std::thread([=] {
                const size_t b0 = std::min(len, (size_t)t * slice), b1 = std::min(len, b0 + slice);
                if (b1 > b0) memcpy(pin[b] + b0, src + o + b0, b1 - b0);
            });
        for (int t = 0; t < UP_THREADS; t++) th[t].join();
        e = hipMemcpyAsync(dt->text + o, pin[b], len, hipMemcpyHostToDevice, up);
        if (e == hipSuccess) e = hipEventRecord(ev[b], up);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(up);
    for (int b = 0; b < 2; b++) {
        if (ev[b]) (void)hipEventDestroy(ev[b]);
        if (pin[b]) (void)hipHostFree(pin[b]);
    }
    if (up) (void)hipStreamDestroy(up);
    if (e != hipSuccess) return ctx_fail(c, CELLECTOR_EDEVICE, "text upload: %s", hipGetErrorString(e));
    return CELLECTOR_OK;
}

// the file's last byte; of a file left compressed through the host decoder, whose refusal of that member counts like the device's
cellector_status read_last_byte(cellector_ctx *c, const FileBytes &fb, uint8_t *byte, bool *refused)
{
    if (fb.read(fb.size - 1, 1, byte)) return CELLECTOR_OK;
    if (!fb.gz) return ctx_fail(c, CELLECTOR_EIO, "cannot read the input file");
    *refused = true;
    return ctx_fail(c, CELLECTOR_EIO, "%s: member %llu is refused: the host decoder does not accept it", fb.path.c_str(),
                    (unsigned long long)fb.member_at(fb.size - 1));
}

cellector_status split_lines(cellector_ctx *c, const FileBytes &fb, DevText *dt, bool *refused)
{
    uint8_t last_byte = '\n';
    if (dt->n > 0) CHK(read_last_byte(c, fb, &last_byte, refused));
    const bool unterminated = last_byte != '\n';
    const uint64_t n_scan = dt->n + (unterminated ? 1 : 0);  // include one padding '\n' as the terminator
    const uint64_t nthreads = (n_scan + NL_SEG - 1) / NL_SEG;
    CHK(dev_alloc(c, &dt->seg_off, nthreads + 1));
    HIPCHK(c, hipMemsetAsync(dt->seg_off, 0, (nthreads + 1) * 8, c->stream));
    if (nthreads) hipLaunchKernelGGL(k_nl_count, dim3(pgrid(nthreads)), dim3(PB), 0, c->stream, dt->at(), n_scan, dt->seg_off);
    HIPCHK(c, hipGetLastError());
    uint64_t n_nl = 0;
    CHK(dev_exclusive_scan_u64(c, dt->seg_off, nthreads + 1, &n_nl));
    dt->n_lines = n_nl;  // every line is terminated now
    dt->n_seg = nthreads;
    dt->n = n_scan;
    return CELLECTOR_OK;
}

// ---- windowed parse of one file -------------------------------------------------------------------------------
// A multi-GB data section never resides on the device as a whole: a producer thread copies windows of it (plus PW_LOOK
// bytes of look-ahead: a line that starts in a window may end behind it) through pinned buffers into one of PW_NB device
// buffers, the caller's thread counts the window's newlines, scans them and tokenises the lines that start there straight
// into the token arrays, at the running line count.  The text of BASELINE configs[4] is 2 x 31 GB: as one allocation per
// file it cost 65 GB of fresh VRAM (30-50 ms per GB to map) before the first line was parsed.
#define PW_LOOK (1ull << 20)  // the longest line a windowed file may hold
#define PW_NB 3
#define PW_WINDOW (256ull << 20)
#define PW_SPLIT_WINDOW (32ull << 20)  // largest window of the split ingest of a multi-device ctx (every shard has its own ring)
#define PW_MIN (1ull << 30)  // data sections from this size on go through the windows
#define PW_THREADS 8  // host threads filling a pinned buffer (pread out of the page cache; 16 threads measured no faster)

inline uint64_t pw_windows(uint64_t bytes, uint64_t win) { return (bytes + win - 1) / win; }
// buffers of the ring of a parser that takes n_win windows
inline int pw_ring(uint64_t n_win) { return (int)std::min<uint64_t>(PW_NB, std::max<uint64_t>(1, n_win)); }
// the window: 1/div of the bigger file's data section, lo .. hi bytes; the environment (in MB), then option parse_window override it
uint64_t pw_window(const MtxInput *in, uint64_t div, uint64_t lo, uint64_t hi, const char *env, uint64_t parse_window)
{
    uint64_t win = std::max(in->fa.size - in->off_a, in->fr.size - in->off_r) / div;
    win = std::min<uint64_t>(hi, std::max<uint64_t>(lo, win));
    if (const char *e_mb = getenv(env)) win = (uint64_t)atoll(e_mb) << 20;
    if (parse_window > 0) win = parse_window;
    if (win < 4 * NL_SEG) win = 4 * NL_SEG;
    return win & ~(uint64_t)(NL_SEG - 1);
}

// the status words of a parse on the device and their host copies.  bad[0] alt file, [1] ref file: smallest line that does not
// parse; [2] zip stage: smallest refused entry << PE_KIND_BITS | its kind.  flags[1]: the file order is not locus-major.
struct ParseStatus {
    DevBuf<unsigned long long> bad;
    DevBuf<uint32_t> flags;
    unsigned long long h_bad[3] = {~0ull, ~0ull, ~0ull};
    uint32_t h_flags[4] = {0, 0, 0, 0};
    cellector_status init(cellector_ctx *c, bool with_flags = true)
    {
        CHK(dev_alloc(c, &bad, 3));
        if (with_flags) CHK(dev_alloc(c, &flags, 4));
        return copy(c, bad, h_bad, flags, h_flags, with_flags, hipMemcpyHostToDevice);
    }
    // (read BEHIND the kernels on the ctx's stream: a caller-supplied non-blocking stream does not order against null-stream copies)
    cellector_status read(cellector_ctx *c, bool with_flags) { return copy(c, h_bad, bad, h_flags, flags, with_flags, hipMemcpyDeviceToHost); }
    cellector_status copy(cellector_ctx *c, void *dbad, const void *sbad, void *dflags, const void *sflags, bool with_flags, hipMemcpyKind kind)
    {
        hipError_t e = hipMemcpyAsync(dbad, sbad, sizeof h_bad, kind, c->stream);
        if (e == hipSuccess && with_flags) e = hipMemcpyAsync(dflags, sflags, sizeof h_flags, kind, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        return e == hipSuccess ? CELLECTOR_OK : ctx_fail(c, CELLECTOR_EDEVICE, "parse: %s", hipGetErrorString(e));
    }
};

// the windows' buffers, shared by the two files of a pair (pinning 3 x 257 MB takes ~0.05 s)
struct PwBuffers {
    uint8_t *pin[PW_NB] = {};
    DevBuf<uint8_t> dev[PW_NB];
    hipEvent_t ev_up[PW_NB] = {}, ev_free[PW_NB] = {};
    hipStream_t up = nullptr;
    DevBuf<uint64_t> seg;
    uint64_t window = 0;
    int n = 0;
    cellector_status make(cellector_ctx *c, uint64_t win, int count)
    {
        window = win;
        const size_t buf_bytes = window + PW_LOOK + 64;
        hipError_t e = hipStreamCreateWithFlags(&up, hipStreamNonBlocking);
        for (int b = 0; b < count && e == hipSuccess; b++) {
            e = hipHostMalloc((void **)&pin[b], buf_bytes);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&ev_up[b], hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&ev_free[b], hipEventDisableTiming);
            if (e == hipSuccess && dev_alloc(c, &dev[b], buf_bytes) != CELLECTOR_OK) e = hipErrorOutOfMemory;
            if (e == hipSuccess) n = b + 1;
        }
        if (e == hipSuccess && dev_alloc(c, &seg, window / NL_SEG + 2) != CELLECTOR_OK) e = hipErrorOutOfMemory;
        return e == hipSuccess ? CELLECTOR_OK : ctx_fail(c, CELLECTOR_EDEVICE, "parse buffers: %s", hipGetErrorString(e));
    }
    ~PwBuffers()
    {
        if (up) (void)hipStreamSynchronize(up);
        for (int b = 0; b < PW_NB; b++) {
            if (ev_up[b]) (void)hipEventDestroy(ev_up[b]);
            if (ev_free[b]) (void)hipEventDestroy(ev_free[b]);
            if (pin[b]) (void)hipHostFree(pin[b]);
            dev[b].reset();
        }
        seg.reset();
        if (up) (void)hipStreamDestroy(up);
    }
};

// what the windowed parser needs beside PwBuffers for a file left compressed (option gz_device): per ring slot a pinned buffer
// for a window's compressed bytes and one for its member table; one device buffer for the compressed bytes and one for the
// inflated members (the upload stream orders their reuse).  Sized from the member index: the largest window of this call.
struct GzWindows {
    InfScratch s;
    uint8_t *pin_in[PW_NB] = {};
    InfMember *pin_members[PW_NB] = {};
    DevBuf<uint8_t> d_in, d_text;
    uint64_t cap_in = 0, cap_text = 0;
    uint64_t have_a = 1, have_b = 0;  // the members d_text holds (none yet): a window they cover needs no launch
    cellector_status make(cellector_ctx *c, const FileBytes &fb, size_t data_off, uint64_t window, uint64_t nb, uint64_t w_begin, uint64_t w_end,
                          int n_ring, hipStream_t up)
    {
        uint64_t cap_members = 0;
        for (uint64_t w = w_begin; w < w_end; w++) {
            const uint64_t o = w * window, len = std::min<uint64_t>(window + PW_LOOK, nb - o);
            const uint64_t ka = fb.member_at(data_off + o), kb = fb.member_at(data_off + o + len - 1);
            cap_in = std::max<uint64_t>(cap_in, fb.blocks[kb].off + fb.blocks[kb].clen - fb.blocks[ka].off);
            cap_text = std::max<uint64_t>(cap_text, fb.blocks[kb].out + fb.blocks[kb].isize - fb.blocks[ka].out);
            cap_members = std::max(cap_members, kb + 1 - ka);
        }
        CHK(inf_scratch(c, &s, cap_members));
        CHK(dev_alloc(c, &d_in, cap_in));
        CHK(dev_alloc(c, &d_text, cap_text));
        for (int b = 0; b < n_ring; b++) {
            HIPCHK(c, hipHostMalloc((void **)&pin_in[b], cap_in ? cap_in : 1));
            HIPCHK(c, hipHostMalloc((void **)&pin_members[b], cap_members * sizeof(InfMember)));
        }
        HIPCHK(c, hipMemsetAsync(s.status, 0xff, sizeof(unsigned long long), up));  // (one status word for the file's launches)
        return CELLECTOR_OK;
    }
    ~GzWindows()
    {
        for (int b = 0; b < PW_NB; b++) {
            if (pin_in[b]) (void)hipHostFree(pin_in[b]);
            if (pin_members[b]) (void)hipHostFree(pin_members[b]);
        }
    }
};

template <typename T>
cellector_status grow_tokens(cellector_ctx *c, DevBuf<T> *arr, uint64_t used, uint64_t new_cap)
{
    DevBuf<T> bigger;
    CHK(dev_alloc(c, &bigger, new_cap));
    hipError_t e = hipSuccess;
    if (used) e = hipMemcpyAsync(bigger, *arr, used * sizeof(T), hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return ctx_fail(c, CELLECTOR_EDEVICE, "parse: %s", hipGetErrorString(e));
    *arr = std::move(bigger);
    return CELLECTOR_OK;
}

// tokens of every line of the data section: ALT -> o0, o1, o2 (locus, cell, count), else o2 only (count); arrays are
// allocated here (capacity from the header's entry count, grown if the file holds more lines)
template <bool ALT>
cellector_status parse_windowed(cellector_ctx *c, const FileBytes &fb, size_t data_off, PwBuffers &B, uint64_t cap_hint,
                                DevBuf<uint32_t> *o0, DevBuf<uint32_t> *o1, DevBuf<uint32_t> *o2, uint64_t *n_lines,
                                unsigned long long *bad, bool *refused, uint64_t w_begin = 0, uint64_t w_end = ~0ull)
{
    // [w_begin, w_end): the windows this call takes (a multi-device ingest gives every GPU a range of them).  Line indices
    // are then LOCAL: the number of newlines before the line inside the range; the line that starts right behind the range's
    // last newline — in the next range's bytes — is still this call's (look-ahead).  *n_lines = newlines in the range.
    const uint64_t window = B.window;
    uint8_t *const *pin = B.pin;
    const DevBuf<uint8_t> *dev = B.dev;
    hipEvent_t *ev_up = B.ev_up, *ev_free = B.ev_free;
    hipStream_t up = B.up;
    uint64_t *seg = B.seg;
    const uint64_t n_ring = (uint64_t)B.n;  // buffers in the ring
    const uint64_t nb = fb.size - data_off;
    *n_lines = 0;
    uint64_t cap = (cap_hint ? cap_hint : nb / 12) + 16;
    if (ALT) { CHK(dev_alloc(c, o0, cap)); CHK(dev_alloc(c, o1, cap)); }
    CHK(dev_alloc(c, o2, cap));
    if (nb == 0) return CELLECTOR_OK;
    uint8_t last_byte = '\n';
    CHK(read_last_byte(c, fb, &last_byte, refused));
    const bool unterminated = last_byte != '\n';
    const uint64_t n_win = (nb + window - 1) / window;
    if (w_end > n_win) w_end = n_win;
    if (w_begin >= w_end) return CELLECTOR_OK;
    GzWindows G;  // (a file left compressed: the producer inflates every window on the device)
    if (fb.gz) CHK(G.make(c, fb, data_off, window, nb, w_begin, w_end, (int)n_ring, up));
    hipError_t e = hipSuccess;
    std::mutex mu;
    std::condition_variable cv;
    uint64_t produced = 0, consumed = 0;
    bool stop = false;
    hipError_t perr = hipSuccess;
    cellector_status st = CELLECTOR_OK;
    {
        std::thread producer([&] {
            hipError_t pe = hipSetDevice(c->device);
            for (uint64_t w = w_begin; w < w_end && pe == hipSuccess; w++) {
                const uint64_t wi = w - w_begin;
                const int b = (int)(wi % n_ring);
                if (wi >= n_ring) {  // the buffer's previous window has been tokenised
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return consumed + n_ring > wi || stop; });
                    if (stop) return;
                    lk.unlock();
                    pe = hipEventSynchronize(ev_free[b]);
                    if (pe != hipSuccess) break;
                }
                const uint64_t o = w * window;
                const size_t len = (size_t)std::min<uint64_t>(window + PW_LOOK, nb - o);
                if (fb.gz) {
                    // the members that cover the window's text: their compressed bytes through the slot's pinned buffer to the
                    // device, inflated there into a scratch whose origin is the first member's text, the window's slice of that
                    // into dev[b], the padding newlines behind it; ev_up[b] last.  (Consecutive windows inflate the look-ahead's
                    // members twice: at most PW_LOOK of text a window, not worth a carry.)
                    const uint64_t t0 = data_off + o, ka = fb.member_at(t0), kb = fb.member_at(t0 + len - 1);
                    const uint64_t in_first = fb.blocks[ka].off, n_in = fb.blocks[kb].off + fb.blocks[kb].clen - in_first;
                    const uint64_t out_first = fb.blocks[ka].out, n_text = fb.blocks[kb].out + fb.blocks[kb].isize - out_first;
                    if (n_in > G.cap_in || n_text > G.cap_text || kb + 1 - ka > G.s.cap_members) { pe = hipErrorInvalidValue; break; }
                    // (the scratch still holds the members of the last launch; a window they cover — every one after the first of
                    //  a file shorter than the look-ahead — is only sliced out of it: the stream orders the copies)
                    const bool launch = !(ka >= G.have_a && kb <= G.have_b);
                    if (launch) {
                        G.have_a = ka;
                        G.have_b = kb;
                        std::thread th[PW_THREADS];
                        const size_t slice = ((size_t)n_in + PW_THREADS - 1) / PW_THREADS;
                        for (int t = 0; t < PW_THREADS; t++)
                            th[t] = std::thread([&, t] {
                                const size_t b0 = std::min((size_t)n_in, (size_t)t * slice), b1 = std::min((size_t)n_in, b0 + slice);
                                if (b1 > b0) memcpy(G.pin_in[b] + b0, fb.gz + in_first + b0, b1 - b0);
                            });
                        for (int t = 0; t < PW_THREADS; t++) th[t].join();
                        pe = hipMemcpyAsync(G.d_in, G.pin_in[b], n_in, hipMemcpyHostToDevice, up);
                        if (pe == hipSuccess && inf_launch(c, &G.s, up, fb.blocks, ka, kb + 1, G.pin_members[b], fb.gz, G.d_in, in_first, n_in,
                                                           G.d_text, out_first, n_text, false) != CELLECTOR_OK)
                            pe = hipErrorLaunchFailure;
                    }
                    if (pe == hipSuccess)
                        pe = hipMemcpyAsync(dev[b], G.d_text + (t0 - fb.blocks[G.have_a].out), len, hipMemcpyDeviceToDevice, up);
                    if (pe == hipSuccess) pe = hipMemsetAsync(dev[b] + len, '\n', 32, up);
                    if (pe == hipSuccess) pe = hipEventRecord(ev_up[b], up);
                    if (pe == hipSuccess && launch && G.s.timed) {  // (the kernel's time is read before its events are recorded again)
                        pe = hipStreamSynchronize(up);
                        inf_launch_timed(&G.s);
                    }
                    if (pe != hipSuccess) break;
                    {
                        std::lock_guard<std::mutex> lk(mu);
                        produced = wi + 1;
                    }
                    cv.notify_all();
                    continue;
                }
                std::thread th[PW_THREADS];
                bool got[PW_THREADS];
                const size_t slice = (len + PW_THREADS - 1) / PW_THREADS;
                for (int t = 0; t < PW_THREADS; t++)
                    th[t] = std::thread([&, t] {
                        const size_t b0 = std::min(len, (size_t)t * slice), b1 = std::min(len, b0 + slice);
                        got[t] = b1 <= b0 || fb.read(data_off + o + b0, b1 - b0, pin[b] + b0);
                    });
                for (int t = 0; t < PW_THREADS; t++) th[t].join();
                for (int t = 0; t < PW_THREADS; t++)
                    if (!got[t]) pe = hipErrorFileNotFound;  // (reported as the upload's failure)
                if (pe != hipSuccess) break;
                memset(pin[b] + len, '\n', 32);  // the end of the data terminates a last line without '\n' (BufRead::lines)
                pe = hipMemcpyAsync(dev[b], pin[b], len + 32, hipMemcpyHostToDevice, up);
                if (pe == hipSuccess) pe = hipEventRecord(ev_up[b], up);
                if (pe != hipSuccess) break;
                {
                    std::lock_guard<std::mutex> lk(mu);
                    produced = wi + 1;
                }
                cv.notify_all();
            }
            if (pe != hipSuccess) {
                std::lock_guard<std::mutex> lk(mu);
                perr = pe;
                stop = true;
            }
            cv.notify_all();
        });
        uint64_t line_base = 0;
        for (uint64_t w = w_begin; w < w_end && st == CELLECTOR_OK; w++) {
            const uint64_t wi = w - w_begin;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return produced > wi || stop; });
                if (produced <= wi) {
                    st = ctx_fail(c, CELLECTOR_EDEVICE, "text upload: %s", hipGetErrorString(perr));
                    break;
                }
            }
            const int b = (int)(wi % n_ring);
            const uint64_t o = w * window, in_win = std::min<uint64_t>(window, nb - o);
            const uint64_t len = std::min<uint64_t>(window + PW_LOOK, nb - o);
            const bool last = w + 1 == n_win, more = o + len < nb;
            const uint64_t n_count = in_win + (last && unterminated ? 1 : 0);  // (the padding newline closes the last line)
            const uint64_t n_buf = len + (last && unterminated ? 1 : 0);
            const uint64_t nseg = (n_count + NL_SEG - 1) / NL_SEG;
            e = hipStreamWaitEvent(c->stream, ev_up[b], 0);
            if (e == hipSuccess) e = hipMemsetAsync(seg, 0, (nseg + 1) * 8, c->stream);
            if (e != hipSuccess) { st = ctx_fail(c, CELLECTOR_EDEVICE, "parse: %s", hipGetErrorString(e)); break; }
            hipLaunchKernelGGL(k_nl_count, dim3(pgrid(nseg)), dim3(PB), 0, c->stream, dev[b], n_count, seg);
            uint64_t n_nl = 0;
            st = dev_exclusive_scan_u64(c, seg, nseg + 1, &n_nl);
            if (st != CELLECTOR_OK) break;
            if (line_base + n_nl + 1 > cap) {
                const uint64_t want = std::max(line_base + n_nl + 16, cap + cap / 2);
                if (ALT) { st = grow_tokens(c, o0, line_base + 1, want); if (st == CELLECTOR_OK) st = grow_tokens(c, o1, line_base + 1, want); }
                if (st == CELLECTOR_OK) st = grow_tokens(c, o2, line_base + 1, want);
                if (st != CELLECTOR_OK) break;
                cap = want;
            }
            hipLaunchKernelGGL(k_parse_lines<ALT>, dim3(pgrid(nseg)), dim3(PB), 0, c->stream, dev[b], n_buf, n_count, cap, line_base,
                               w == 0, more, seg, ALT ? *o0 : (uint32_t *)nullptr, ALT ? *o1 : (uint32_t *)nullptr, *o2, bad);
            e = hipEventRecord(ev_free[b], c->stream);
            if (e != hipSuccess) { st = ctx_fail(c, CELLECTOR_EDEVICE, "parse: %s", hipGetErrorString(e)); break; }
            {
                std::lock_guard<std::mutex> lk(mu);
                consumed = wi + 1;
            }
            cv.notify_all();
            line_base += n_nl;
        }
        {
            std::lock_guard<std::mutex> lk(mu);
            if (st != CELLECTOR_OK) stop = true;
        }
        cv.notify_all();
        producer.join();
        e = hipStreamSynchronize(c->stream);
        if (st == CELLECTOR_OK && e != hipSuccess) st = ctx_fail(c, CELLECTOR_EDEVICE, "parse: %s", hipGetErrorString(e));
        if (st == CELLECTOR_OK) *n_lines = line_base;
    }
    if (up) (void)hipStreamSynchronize(up);  // (the buffers go on to the pair's other file)
    if (fb.gz) {  // the status word of the file's launches arrived behind the last one; a refusal goes before whatever else failed
        if (*G.s.h_status != ~0ull) {
            *refused = true;
            *n_lines = 0;
            return inf_refused(c, fb.path.c_str(), *G.s.h_status);
        }
        if (st == CELLECTOR_OK) inf_report(G.s, fb);
    }
    return st;
}

}  // namespace

// a file small enough to sit on the device whole: one upload, one scan of its newlines, one tokeniser launch
template <bool ALT>
static cellector_status parse_whole(cellector_ctx *c, const FileBytes &fb, size_t data_off, DevBuf<uint32_t> *o0, DevBuf<uint32_t> *o1,
                                    DevBuf<uint32_t> *o2, uint64_t *n_lines, unsigned long long *bad, bool *refused)
{
    DevText t;
    cellector_status st = fb.gz ? upload_text_gz(c, fb, data_off, &t, refused) : upload_text(c, fb, data_off, &t);
    if (st == CELLECTOR_OK) st = split_lines(c, fb, &t, refused);
    const uint64_t n = t.n_lines;
    if (st == CELLECTOR_OK && ALT) { st = dev_alloc(c, o0, n); if (st == CELLECTOR_OK) st = dev_alloc(c, o1, n); }
    if (st == CELLECTOR_OK) st = dev_alloc(c, o2, n);
    if (st == CELLECTOR_OK && n) {
        hipLaunchKernelGGL(k_parse_lines<ALT>, dim3(pgrid(t.n_seg)), dim3(PB), 0, c->stream, t.at(), t.n, t.n, n, 0ull, true, false,
                           t.seg_off, ALT ? *o0 : (uint32_t *)nullptr, ALT ? *o1 : (uint32_t *)nullptr, *o2, bad);
        const hipError_t e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) st = ctx_fail(c, CELLECTOR_EDEVICE, "parse: %s", hipGetErrorString(e));
    }
    *n_lines = n;
    return st;
}

// one file's tokens, through B's windows (made by the caller; [w_begin, w_end): see parse_windowed) or whole
template <bool ALT>
static cellector_status parse_file(cellector_ctx *c, FileBytes &fb, size_t data_off, bool windowed, PwBuffers &B, uint64_t cap_hint,
                                   DevBuf<uint32_t> *o0, DevBuf<uint32_t> *o1, DevBuf<uint32_t> *o2, uint64_t *n_lines,
                                   unsigned long long *bad, uint64_t w_begin = 0, uint64_t w_end = ~0ull)
{
    for (int attempt = 0;; attempt++) {
        bool refused = false;
        const cellector_status st = windowed ? parse_windowed<ALT>(c, fb, data_off, B, cap_hint, o0, o1, o2, n_lines, bad, &refused, w_begin, w_end)
                                             : parse_whole<ALT>(c, fb, data_off, o0, o1, o2, n_lines, bad, &refused);
        if (!refused || attempt) return st;
        // The device refused a member of a file left compressed (option gz_device).  The host reader decides what the file is, as
        // it does for a damaged block without the option: the outcome is then the one of gz_device 0.  What the tokeniser made of
        // the member's bytes meanwhile is forgotten.
        // Neither case is silent: the failure keeps the device's words (file, member, why), and a file the host accepts where
        // the device did not is reported on stderr — the decoder then disagrees with zlib's reader, and the load paid for both.
        const std::string why = c->err;
        if (!file_bytes_to_host(&fb)) return ctx_fail(c, CELLECTOR_EIO, "couldn't open file %s (%s)", fb.path.c_str(), why.c_str());
        fprintf(stderr, "cellector: gz_device: %s; the host reader accepts the file: it is read on the host\n", why.c_str());
        HIPCHK(c, hipMemsetAsync(bad, 0xff, sizeof(unsigned long long), c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
}

// ---- split ingest of a multi-device ctx -------------------------------------------------------------------------------------
// Every shard tokenises a RANGE OF WINDOWS of both files on its own GPU (its own PCIe link, its own reader threads), then the
// shards line the two files up and route every entry to the shard that owns its cell:
//   1. parse: alt windows [k n_win / n, (k+1) n_win / n) -> (locus, cell, count) tokens, ref windows likewise -> counts; a
//      line's LOCAL index is the number of newlines before it inside the range, so its global index (= its position in the
//      zip, load_data.rs:190-204) is known once every shard's newline count is: exclusive sums over the ranks;
//   2. the two files' byte ranges do not cut at the same lines (their lines differ in length): every shard fetches the ref
//      counts of ITS alt lines from whichever shards tokenised them (contiguous pieces, peer copies);
//   3. zip + validation of its lines (same kernels as the single-device path), in place -> all-cells COO of those lines;
//   4. cut by owning cell range (order kept), one piece per destination shard;
//   5. every shard concatenates the pieces meant for it IN RANK ORDER = file order, which is what load_cell_data's per-cell
//      lists need (load_data.rs:151-174).
// The threads meet at a barrier between the steps; a failing shard releases the others (LocalGroup::fail).
struct MtxSplit {
    int n = 0;
    LocalGroup *bar = nullptr;
    uint64_t ma[CELLECTOR_MAX_SHARDS] = {}, mr[CELLECTOR_MAX_SHARDS] = {};
    unsigned long long bad_a[CELLECTOR_MAX_SHARDS] = {}, bad_r[CELLECTOR_MAX_SHARDS] = {}, bad_z[CELLECTOR_MAX_SHARDS] = {};
    uint32_t bad_kind[CELLECTOR_MAX_SHARDS] = {}, unsorted[CELLECTOR_MAX_SHARDS] = {};
    uint32_t first_locus[CELLECTOR_MAX_SHARDS] = {}, last_locus[CELLECTOR_MAX_SHARDS] = {};
    uint64_t lines[CELLECTOR_MAX_SHARDS] = {};
    uint32_t *r_dev[CELLECTOR_MAX_SHARDS] = {};  // (each shard's ref counts, owned by the shard)
    int device[CELLECTOR_MAX_SHARDS] = {};
    StagedCoo piece[CELLECTOR_MAX_SHARDS][CELLECTOR_MAX_SHARDS];  // [from][to]: shard `from`'s lines meant for shard `to`, on `from`'s device
    bool balance = false;                             // cut the cells so that every shard gets about the same number of entries
    std::vector<uint32_t> hist[CELLECTOR_MAX_SHARDS];  // ... from every parser's entries per cell
};
MtxSplit *mtx_split_new(int n, LocalGroup *bar, bool balance)
{
    MtxSplit *S = new (std::nothrow) MtxSplit();
    if (S) { S->n = n; S->bar = bar; S->balance = balance; }
    return S;
}
void mtx_split_delete(MtxSplit *S) { delete S; }
cellector_status ctx_mtx_open(const cellector_ctx *c, const char *alt_path, const char *ref_path, MtxInput **out, uint64_t *total_loci,
                              uint64_t *total_cells, bool single_device)
{
    std::string msg;
    const cellector_status st = mtx_input_open(alt_path, ref_path, out, &msg, single_device && c->gz_device);
    if (st != CELLECTOR_OK) return ctx_fail(c, st, "%s", msg.c_str());
    *total_loci = (*out)->total_loci;
    *total_cells = (*out)->total_cells;
    return CELLECTOR_OK;
}
// both files go through the windowed parser (big, or the parse_window option forces it): the split ingest needs that
bool mtx_input_windowed(const MtxInput *in, int64_t parse_window_opt)
{
    const uint64_t na = in->fa.size - in->off_a, nr = in->fr.size - in->off_r;
    return na > 0 && nr > 0 && (parse_window_opt > 0 || (na >= PW_MIN && nr >= PW_MIN));
}

cellector_status ingest_stage_mtx_split(cellector_ctx *c, MtxInput *in, MtxSplit *S, int rank, uint64_t parse_window, StagedCoo *out)
{
    const int n = S->n;
    const uint64_t TL = in->total_loci, TC = in->total_cells;
    DevBuf<uint32_t> l1, c1, a, r, rk;
    DevBuf<uint16_t> alt16, ref16;
    ParseStatus ps;
    DevBuf<uint64_t> keep;
    // (on a failure the pieces this shard cut for the others stay until the MtxSplit goes: a peer may still be reading them)
#define SCHK(expr)                     \
    do {                               \
        cellector_status s__ = (expr); \
        if (s__ != CELLECTOR_OK) {     \
            S->bar->fail();            \
            return s__;                \
        }                              \
    } while (0)
#define SBARRIER()                                                                                                         \
    do {                                                                                                                   \
        if (!S->bar->barrier()) return ctx_fail(c, CELLECTOR_ECOMM, "another shard of this ctx failed during the ingest"); \
    } while (0)
    if (hipSetDevice(c->device) != hipSuccess) {  // (through the barrier group like every other failure: the peers must not wait)
        S->bar->fail();
        return ctx_fail(c, CELLECTOR_EDEVICE, "hipSetDevice(%d) failed", c->device);
    }
    S->device[rank] = c->device;
    const bool timing = rank == 0 && getenv("CELLECTOR_TIMING") != nullptr;  // phase wall times of shard 0 on stderr
    LapTimer t;
    auto lap = [&](const char *what) {
        if (timing) fprintf(stderr, "[timing]     split: %-26s %8.3f s\n", what, t.lap());
    };
    SCHK(ps.init(c));
    unsigned long long *const bad = ps.bad, *const h_bad = ps.h_bad;
    hipError_t e = hipSuccess;
    // ---- 1. this shard's windows of both files
    // (n shards pin their upload buffers at the same time and the driver pins them one after the other: 4 x 3 x 256 MB took
    //  0.2-0.5 s per shard on one box — 4 logical shards, 2 x 2.9 GB: 1.1 s with 256 MB windows, 0.32 s with 16 MB)
    const uint64_t win = pw_window(in, (uint64_t)n * 32, 16ull << 20, PW_SPLIT_WINDOW, "CELLECTOR_SPLIT_WINDOW_MB" /*tools/split_check.sh*/,
                                   parse_window);
    uint64_t ma = 0, mr = 0;
    {
        const uint64_t nb_a = in->fa.size - in->off_a, nb_r = in->fr.size - in->off_r;
        const uint64_t nw_a = pw_windows(nb_a, win), nw_r = pw_windows(nb_r, win);
        const uint64_t hint = in->nnz_hint ? in->nnz_hint / (uint64_t)n + in->nnz_hint / (uint64_t)(8 * n) + 1024 : 0;
        PwBuffers B;
        SCHK(B.make(c, win, pw_ring(std::max(nw_a, nw_r) / (uint64_t)n + 1)));
        lap("upload buffers");
        // ranges of ceil(n_win / n) windows: rank 0 always holds window 0 (= line 0); late ranks of a short file may hold none
        const uint64_t pa = (nw_a + n - 1) / n, pr = (nw_r + n - 1) / n;
        SCHK((parse_file<true>(c, in->fa, in->off_a, true, B, hint ? hint : nb_a / (12 * (uint64_t)n) + 1024, &l1, &c1, &a, &ma, bad,
                               std::min(nw_a, pa * rank), std::min(nw_a, pa * (rank + 1)))));
        lap("alt range (upload + tokens)");
        SCHK((parse_file<false>(c, in->fr, in->off_r, true, B, hint ? hint : nb_r / (12 * (uint64_t)n) + 1024, nullptr, nullptr, &r, &mr,
                                bad + 1, std::min(nw_r, pr * rank), std::min(nw_r, pr * (rank + 1)))));
        lap("ref range (upload + tokens)");
    }
    SCHK(ps.read(c, false));
    S->ma[rank] = ma; S->mr[rank] = mr; S->bad_a[rank] = h_bad[0]; S->bad_r[rank] = h_bad[1]; S->r_dev[rank] = r;
    lap("release buffers");
    SBARRIER();
    lap("wait for the other shards");
    // ---- 2. global line numbers; the ref counts of this shard's alt lines
    uint64_t abase[CELLECTOR_MAX_SHARDS + 1] = {0}, rbase[CELLECTOR_MAX_SHARDS + 1] = {0};
    for (int k = 0; k < n; k++) { abase[k + 1] = abase[k] + S->ma[k]; rbase[k + 1] = rbase[k] + S->mr[k]; }
    const uint64_t nlines = std::min(abase[n], rbase[n]);  // izip!: stops at the shorter file
    {
        unsigned long long first = ~0ull;  // (a line beyond the shorter file is never read by the reference)
        for (int k = 0; k < n; k++) {
            if (S->bad_a[k] != ~0ull) first = std::min<unsigned long long>(first, abase[k] + S->bad_a[k]);
            if (S->bad_r[k] != ~0ull) first = std::min<unsigned long long>(first, rbase[k] + S->bad_r[k]);
        }
        if (first < nlines) {
            (void)S->bar->barrier();  // (every shard sees the same numbers and leaves here: nobody is left waiting)
            return ctx_fail(c, CELLECTOR_EPARSE, "cannot parse mtx entry %llu (line %llu of the data section)", first, first + 1);
        }
    }
    // lines held by rank k of a file with bases b: global (b[k], b[k] + m[k]] and, for rank 0, line 0; local index = global - b[k]
    auto g_lo = [&](const uint64_t *b, int k) -> uint64_t { return k == 0 ? (uint64_t)0 : b[k] + 1; };
    auto g_hi = [&](const uint64_t *b, int k) -> uint64_t { return std::min<uint64_t>(nlines, b[k + 1] + 1); };  // exclusive
    const uint64_t glo = std::min(g_lo(abase, rank), nlines), ghi = std::max(glo, g_hi(abase, rank));
    const uint64_t count = ghi - glo, lo = count ? glo - abase[rank] : 0;  // (a rank whose alt range lies beyond a shorter ref file holds nothing)
    SCHK(dev_alloc(c, &rk, ma + 2));
    for (int k = 0; k < n; k++) {
        const uint64_t s0 = std::max(glo, g_lo(rbase, k)), s1 = std::min(ghi, g_hi(rbase, k));
        if (s0 >= s1) continue;
        e = dev_copy_sync(c->stream, rk + (s0 - abase[rank]), c->device, S->r_dev[k] + (s0 - rbase[k]), S->device[k], (s1 - s0) * sizeof(uint32_t));
        if (e != hipSuccess) SCHK(ctx_fail(c, CELLECTOR_EDEVICE, "copy between shards failed: %s", hipGetErrorString(e)));
    }
    SBARRIER();  // (every shard has fetched what it needs out of the others' ref counts)
    lap("fetch ref counts");
    r.reset();
    S->r_dev[rank] = nullptr;
    // ---- 3. zip + validation of this shard's lines, in place
    hipLaunchKernelGGL(k_pair_check, dim3(pgrid(count + 1)), dim3(PB), 0, c->stream, count, l1 + lo, c1 + lo, a + lo, rk + lo, TL, TC,
                       (uint64_t)0, TC, (uint64_t *)nullptr, bad + 2, ps.flags + 1);
    uint32_t edge[2] = {0, 0};  // (the first and the last locus token, queued in front of the status words' copy and its synchronise)
    if (count) e = hipMemcpyAsync(&edge[0], l1 + lo, 4, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && count) e = hipMemcpyAsync(&edge[1], l1 + lo + count - 1, 4, hipMemcpyDeviceToHost, c->stream);
    if (e != hipSuccess) SCHK(ctx_fail(c, CELLECTOR_EDEVICE, "parse: %s", hipGetErrorString(e)));
    SCHK(ps.read(c, true));
    S->bad_z[rank] = h_bad[2] == ~0ull ? ~0ull : glo + (h_bad[2] >> PE_KIND_BITS);  // (local entry -> global, the kind beside it)
    S->bad_kind[rank] = (uint32_t)(h_bad[2] & ((1u << PE_KIND_BITS) - 1)); S->unsorted[rank] = ps.h_flags[1];
    S->first_locus[rank] = edge[0]; S->last_locus[rank] = edge[1]; S->lines[rank] = count;
    SBARRIER();
    {
        int worst = -1;
        for (int k = 0; k < n; k++)
            if (S->bad_z[k] != ~0ull && (worst < 0 || S->bad_z[k] < S->bad_z[worst])) worst = k;
        if (worst >= 0) {
            (void)S->bar->barrier();
            return ctx_fail(c, CELLECTOR_EINVAL, "mtx entry %llu: %s", S->bad_z[worst], pe_kind_text(S->bad_kind[worst]));
        }
        bool sorted = true;
        uint32_t prev_last = 0;
        bool have_prev = false;
        for (int k = 0; k < n; k++) {
            if (S->unsorted[k]) sorted = false;
            if (!S->lines[k]) continue;
            if (have_prev && S->first_locus[k] < prev_last) sorted = false;  // (1-based tokens on both sides)
            prev_last = S->last_locus[k];
            have_prev = true;
        }
        out->sorted = sorted;
    }
    SCHK(dev_alloc(c, &alt16, count)); SCHK(dev_alloc(c, &ref16, count));
    if (count) hipLaunchKernelGGL(k_pair_take, dim3(pgrid(count)), dim3(PB), 0, c->stream, count, l1 + lo, c1 + lo, a + lo, rk + lo, alt16, ref16);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) SCHK(ctx_fail(c, CELLECTOR_EDEVICE, "parse: %s", hipGetErrorString(e)));
    // ---- 4. one piece per destination shard (cells of its range, order kept, cell index local to it)
    SCHK(dev_alloc(c, &keep, count + 1));
    if (S->balance) {
        // nnz-balanced ranges: every parser counts its entries per cell, all of them add the n histograms up (the same
        // integers on every shard) and cut the cells where the running sum crosses k / n of the entries
        SCHK(ingest_cell_histogram(c, c1 + lo, count, TC, &S->hist[rank]));
        SBARRIER();
        std::vector<uint32_t> epc(TC, 0u);
        for (int k = 0; k < n; k++)
            for (uint64_t i = 0; i < TC; i++) epc[i] += S->hist[k][i];
        comm_balanced_bounds(epc.data(), TC, n, c->comm.bounds);
        c->comm.has_bounds = true;
    }
    for (int d = 0; d < n; d++) {
        uint64_t cb, ce;
        comm_range(c->comm, TC, d, &cb, &ce);
        SCHK(ingest_split_coo(c, CooView{l1 + lo, c1 + lo, alt16, ref16, count}, cb, ce, keep, &S->piece[rank][d]));
    }
    lap("zip + cut by owner");
    SBARRIER();
    // ---- 5. this shard's entries = the pieces meant for it, in rank order (= file order)
    uint64_t total = 0;
    for (int k = 0; k < n; k++) total += S->piece[k][rank].n;
    SCHK(out->alloc(c, total));
    uint64_t at = 0;
    for (int k = 0; k < n; k++) {
        const uint64_t m = S->piece[k][rank].n;
        e = out->copy_from(c, at, S->piece[k][rank], S->device[k], m);
        if (e != hipSuccess) SCHK(ctx_fail(c, CELLECTOR_EDEVICE, "copy between shards failed: %s", hipGetErrorString(e)));
        at += m;
    }
    SBARRIER();  // (the pieces this shard made have been fetched by their destinations)
    for (int d = 0; d < n; d++) S->piece[rank][d].reset();
    l1.reset(); c1.reset(); a.reset(); rk.reset(); ps.flags.reset(); ps.bad.reset(); keep.reset(); alt16.reset(); ref16.reset();
    lap("gather own pieces");
#undef SCHK
#undef SBARRIER
    return CELLECTOR_OK;
}

// Stage this shard's entries of the alt/ref pair on the device; dims / shard range must already be set on the ctx.
// The ref file's count tokens parsed on ANOTHER ctx's device and stream (multi-device ingest: the two files are independent
// byte streams until they are zipped, so a second GPU takes the second file over its own PCIe link while the first one
// tokenises the alt file; two files together also read faster from the page cache than one: 76 vs 43 GB/s measured).
static cellector_status parse_ref_on(cellector_ctx *h, FileBytes &fr, size_t off_r, uint64_t win, bool windowed, uint64_t nnz_hint,
                                     DevBuf<uint32_t> *r_out, uint64_t *n_r, unsigned long long *bad_host)
{
    HIPCHK(h, hipSetDevice(h->device));
    ParseStatus ps;  // (the helper uses word 0 for its file)
    CHK(ps.init(h, false));
    {
        PwBuffers B;
        if (windowed) CHK(B.make(h, win, pw_ring(pw_windows(fr.size - off_r, win))));
        CHK((parse_file<false>(h, fr, off_r, windowed, B, nnz_hint, nullptr, nullptr, r_out, n_r, ps.bad)));
    }
    CHK(ps.read(h, false));
    *bad_host = ps.h_bad[0];
    return CELLECTOR_OK;
}

// the window of a single-device ingest of the pair, and whether a file goes through the windows at all
static uint64_t pair_window(const cellector_ctx *c, const MtxInput *in)
{
    return pw_window(in, 96, 32ull << 20, PW_WINDOW, "CELLECTOR_WINDOW_MB" /*the sweep*/, c->parse_window_opt > 0 ? (uint64_t)c->parse_window_opt : 0);
}
static bool file_windowed(const cellector_ctx *c, const FileBytes &f, size_t data_off)
{
    return c->parse_window_opt > 0 || (!f.data && !f.gz) || f.size - data_off >= PW_MIN;  // (a compressed file is not an unmapped one)
}

cellector_status ingest_stage_mtx_device(cellector_ctx *c, MtxInput *in, cellector_ctx *helper)
{
    FileBytes &fa = in->fa, &fr = in->fr;
    const size_t off_a = in->off_a, off_r = in->off_r;
    const bool timing = getenv("CELLECTOR_TIMING") != nullptr;  // phase wall times on stderr
    LapTimer t;
    auto lap = [&](const char *what) {
        if (!timing) return;
        (void)hipDeviceSynchronize();
        fprintf(stderr, "[timing]     %-22s %8.3f s\n", what, t.lap());
    };
    DevBuf<uint32_t> l1, c1, a, r;
    ParseStatus ps;
    DevBuf<uint64_t> keep;
    HIPCHK(c, hipSetDevice(c->device));
    CHK(ps.init(c));
    unsigned long long *const bad = ps.bad, *const h_bad = ps.h_bad;
    // a multi-GB file goes through the device in windows (option parse_window forces a window size: tests); the token
    // arrays' capacity comes from the size line's entry count (a hint only: the reference never reads it)
    uint64_t n_a = 0, n_r = 0;
    // window: 1/96 of the bigger file, 32 MB .. PW_WINDOW.  (Pinning and releasing 3 x 256 MB of upload buffers is 0.1-0.15 s
    // of a 0.39 s ingest of 2 x 2.9 GB: 32 MB windows take 0.245 s there; at 2 x 31 GB the window size makes no difference,
    // 256 MB stays.  tools/window_sweep.sh)
    const uint64_t win = pair_window(c, in);
    const bool win_a = file_windowed(c, fa, off_a), win_r = file_windowed(c, fr, off_r);
    if (helper) {  // the ref file on the helper's device, concurrently (its own ring of window buffers, its own stream)
        DevBuf<uint32_t> r_h;
        unsigned long long bad_r = ~0ull;
        cellector_status st_r = CELLECTOR_OK;
        std::thread th([&] { st_r = parse_ref_on(helper, fr, off_r, win, win_r, in->nnz_hint, &r_h, &n_r, &bad_r); });
        cellector_status st_a = CELLECTOR_OK;
        {
            PwBuffers B;
            if (win_a) st_a = B.make(c, win, pw_ring(pw_windows(fa.size - off_a, win)));
            if (st_a == CELLECTOR_OK) st_a = parse_file<true>(c, fa, off_a, win_a, B, in->nnz_hint, &l1, &c1, &a, &n_a, bad);
        }
        th.join();
        (void)hipSetDevice(c->device);
        if (st_a == CELLECTOR_OK && st_r != CELLECTOR_OK) st_a = ctx_fail(c, st_r, "%s", helper->err.c_str());
        if (st_a == CELLECTOR_OK) st_a = dev_alloc(c, &r, n_r);
        if (st_a == CELLECTOR_OK && n_r && dev_copy_sync(c->stream, r, c->device, r_h, helper->device, n_r * sizeof(uint32_t)) != hipSuccess)
            st_a = ctx_fail(c, CELLECTOR_EDEVICE, "peer copy of the ref counts failed: %s", hipGetErrorString(hipGetLastError()));
        if (st_a == CELLECTOR_OK &&
            (hipMemcpyAsync(bad + 1, &bad_r, sizeof bad_r, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
             hipStreamSynchronize(c->stream) != hipSuccess))
            st_a = ctx_fail(c, CELLECTOR_EDEVICE, "parse: copy failed");
        r_h.reset();
        CHK(st_a);
        lap("alt + ref files (two devices)");
    } else {
        // While the host reads and the device tokenises (host-bound: ~1.5 s for 2 x 31 GB), a helper thread maps the VRAM the
        // CSC / CSR build will ask for right afterwards — three arrays of 8 bytes per entry, sized from the header's entry
        // count — and parks the blocks in the caching layer: mapping fresh VRAM costs 10-60 ms per GB at this footprint and
        // would otherwise be paid serially behind the parse (0.5-1.5 s of the 1M x 200k ingest).  Unused blocks go back at the
        // end of the ingest (dev_cache_trim).
        std::thread premap;
        struct Joiner { std::thread &t; ~Joiner() { if (t.joinable()) t.join(); } } premap_joiner{premap};
        {
            const char *env = getenv("CELLECTOR_PREMAP");
            const bool all = c->cell_begin == 0 && c->cell_end >= c->total_cells;
            const uint64_t hint = in->nnz_hint <= (fa.size - off_a) / 6 ? in->nnz_hint : 0;  // (a line has at least 6 bytes: else the header lies)
            if (win_a && all && !c->ingest_all_cells && hint >= (1ull << 26) && (!env || atoi(env) != 0)) {  // (not for a multi-device ctx's parser: its shards build smaller matrices)
                const int dev = c->device;
                premap = std::thread([dev, hint] {
                    if (hipSetDevice(dev) != hipSuccess) return;
                    // (a little more than 8 bytes per entry: the 4-byte token arrays, asked for meanwhile, must not match
                    //  these blocks — the caching layer hands out blocks of up to twice the request)
                    // in the order they are asked for: the ref file's count tokens (4 B per entry, as parse_windowed sizes
                    // them), the two 16-bit count arrays of the staged entries, then the CSC / CSR build's three arrays
                    const size_t sizes[6] = {((size_t)hint + 16) * 4, (size_t)hint * 2 + 4096, (size_t)hint * 2 + 4096,
                                             (size_t)hint * 8 + (1u << 16), (size_t)hint * 8 + (1u << 16), (size_t)hint * 8 + (1u << 16)};
                    for (size_t bytes : sizes) {
                        void *p = nullptr;
                        if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); return; }
                        dev_cache_park(p, bytes, dev);
                    }
                });
            }
        }
        PwBuffers B;  // one ring of window buffers for both files
        if (win_a || win_r) {
            const uint64_t longest = std::max(win_a ? fa.size - off_a : 0, win_r ? fr.size - off_r : 0);
            CHK(B.make(c, win, pw_ring(pw_windows(longest, win))));
        }
        CHK((parse_file<true>(c, fa, off_a, win_a, B, in->nnz_hint, &l1, &c1, &a, &n_a, bad)));
        lap("alt file (upload + tokens)");
        CHK((parse_file<false>(c, fr, off_r, win_r, B, in->nnz_hint, nullptr, nullptr, &r, &n_r, bad + 1)));
        lap("ref file (upload + tokens)");
        if (premap.joinable()) premap.join();
        lap("wait for the pre-mapped blocks");
    }
    const uint64_t n = std::min(n_a, n_r);  // izip!: stops at the shorter file
    CHK(ps.read(c, false));
    {   // (a line beyond the shorter file is never read by the reference: only failures among the first n count)
        const unsigned long long first = std::min(h_bad[0], h_bad[1]);
        if (first < n)
            return ctx_fail(c, CELLECTOR_EPARSE, "cannot parse mtx entry %llu (line %llu of the data section)", first, first + 1);
    }
    const bool all_cells = c->cell_begin == 0 && c->cell_end >= c->total_cells;
    if (!all_cells) CHK(dev_alloc(c, &keep, n + 1));
    hipLaunchKernelGGL(k_pair_check, dim3(pgrid(n + 1)), dim3(PB), 0, c->stream, n, l1, c1, a, r, c->total_loci, c->total_cells,
                       c->cell_begin, c->cell_end, keep, bad + 2, ps.flags + 1);
    CHK(ps.read(c, true));  // (the range check's result)
    if (h_bad[2] != ~0ull) {
        return ctx_fail(c, CELLECTOR_EINVAL, "mtx entry %llu: %s", h_bad[2] >> PE_KIND_BITS, pe_kind_text(h_bad[2]));
    }
    c->coo.sorted = ps.h_flags[1] == 0;
    if (all_cells) {
        c->coo.n = n;
        CHK(dev_alloc(c, &c->coo.alt, n)); CHK(dev_alloc(c, &c->coo.ref, n));
        if (n) hipLaunchKernelGGL(k_pair_take, dim3(pgrid(n)), dim3(PB), 0, c->stream, n, l1, c1, a, r, c->coo.alt, c->coo.ref);
        c->coo.locus = std::move(l1);  // (the token arrays are the staged COO)
        c->coo.cell = std::move(c1);
    } else {
        uint64_t kept = 0;
        CHK(dev_exclusive_scan_u64(c, keep, n + 1, &kept));
        CHK(c->coo.alloc(c, kept));
        if (n)
            hipLaunchKernelGGL(k_pair_fill, dim3(pgrid(n)), dim3(PB), 0, c->stream, n, l1, c1, a, r, c->cell_begin, c->cell_end,
                               keep, c->coo.locus, c->coo.cell, c->coo.alt, c->coo.ref);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    lap("tokenise + zip + filter");
    if (e != hipSuccess) return ctx_fail(c, CELLECTOR_EDEVICE, "parse: %s", hipGetErrorString(e));
    return CELLECTOR_OK;
}

// ---- the joined ingest's tokens (kernels_join.hip joins them) -------------------------------------------------------------------
cellector_status join_size_lines(const cellector_ctx *c, const MtxInput *in, uint64_t *first_hint)
{
    std::string third;
    uint64_t tl = 0, tc = 0;
    const size_t off = skip_header(in->fa, &third);
    if (!host_tok_u64(third, 0, &tl) || !host_tok_u64(third, 1, &tc))
        return ctx_fail(c, CELLECTOR_EPARSE, "FIRST file: cannot parse the matrix market size line");
    if (tl != in->total_loci || tc != in->total_cells)
        return ctx_fail(c, CELLECTOR_EINVAL, "join: the size lines disagree: FIRST has %llu loci x %llu cells, SECOND %llu x %llu",
                        (unsigned long long)tl, (unsigned long long)tc, (unsigned long long)in->total_loci, (unsigned long long)in->total_cells);
    if (!host_tok_u64(third, 2, first_hint) || *first_hint > (in->fa.size - off) / 4) *first_hint = 0;  // (as mtx_input_open treats SECOND's)
    return CELLECTOR_OK;
}

// (No pre-mapping thread here: the aligned ingest's is sized for token arrays that BECOME the staged COO; this route's COO is
// allocated by the join, once the number of distinct keys is known, and the token arrays go back to the cache before the build.)
cellector_status join_parse_pair(cellector_ctx *c, MtxInput *in, uint64_t first_hint, JoinTokens *first, JoinTokens *second, JoinPhases *ph)
{
    HIPCHK(c, hipSetDevice(c->device));
    LapTimer t;
    ParseStatus ps;
    CHK(ps.init(c, false));
    const uint64_t win = pair_window(c, in);
    const bool win_a = file_windowed(c, in->fa, in->off_a), win_r = file_windowed(c, in->fr, in->off_r);
    {
        PwBuffers B;  // one ring of window buffers for both files
        if (win_a || win_r) {
            const uint64_t longest = std::max(win_a ? in->fa.size - in->off_a : 0, win_r ? in->fr.size - in->off_r : 0);
            CHK(B.make(c, win, pw_ring(pw_windows(longest, win))));
        }
        CHK((parse_file<true>(c, in->fa, in->off_a, win_a, B, first_hint, &first->locus, &first->cell, &first->count, &first->n, ps.bad)));
        ph->tokens_first = t.lap();
        CHK((parse_file<true>(c, in->fr, in->off_r, win_r, B, in->nnz_hint, &second->locus, &second->cell, &second->count, &second->n, ps.bad + 1)));
    }
    CHK(ps.read(c, false));
    ph->tokens_second = t.lap();
    for (int s = 0; s < 2; s++)  // (every line of a file counts here: no file is cut at the other one's length)
        if (ps.h_bad[s] != ~0ull)
            return ctx_fail(c, CELLECTOR_EPARSE, "%s file: cannot parse mtx entry %llu (line %llu of the data section)", s ? "SECOND" : "FIRST",
                            ps.h_bad[s], ps.h_bad[s] + 1);
    return CELLECTOR_OK;
}
