// See mtx_bytes.h.
#include "mtx_bytes.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // (the library builds this file as HIP: the format headers' host/device qualifiers)
#endif
#include "inflate_format.h"

#include <fcntl.h>
#include <sys/stat.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <new>
#include <thread>

// A ".gz" whose members all carry the BGZF extra field (bgzip: blocks of at most 64 KB, each a gzip member with its own
// compressed size in a 'B','C' subfield — the reference's MultiGzDecoder reads such a file like any multi-member gzip,
// load_data.rs:246) is inflated block-parallel: the member boundaries are found by hopping over the size fields, the
// output offsets are the prefix sums of the members' ISIZE trailers, and host threads inflate ranges of blocks straight
// into place (raw deflate, CRC-32 and length of every block checked like gzread does).  A single zlib stream inflates at
// ~0.35 GB/s of text; a plain gzip file has no such index and keeps the serial path below.
bool bgzf_index(const uint8_t *f, size_t n, std::vector<BgzfBlock> *blocks, size_t *total)
{
    size_t pos = 0, out = 0;
    while (pos < n) {
        if (n - pos < 18 || f[pos] != 0x1f || f[pos + 1] != 0x8b || f[pos + 2] != 8 || !(f[pos + 3] & 4)) return false;
        if (f[pos + 3] & ~4u) return false;  // (name / comment / header CRC: not what bgzip writes — leave it to zlib)
        const uint32_t xlen = f[pos + 10] | ((uint32_t)f[pos + 11] << 8);
        if (n - pos < 12 + (size_t)xlen + 8) return false;
        uint32_t bsize = 0;
        bool have = false;
        for (size_t q = pos + 12, e = pos + 12 + xlen; q + 4 <= e;) {
            const uint32_t slen = f[q + 2] | ((uint32_t)f[q + 3] << 8);
            if (f[q] == 'B' && f[q + 1] == 'C' && slen == 2 && q + 6 <= e) { bsize = f[q + 4] | ((uint32_t)f[q + 5] << 8); have = true; }
            q += 4 + slen;
        }
        const size_t clen = (size_t)bsize + 1;
        if (!have || clen < 12 + (size_t)xlen + 8 || n - pos < clen) return false;
        const uint8_t *tr = f + pos + clen - 4;
        const uint32_t isize = tr[0] | ((uint32_t)tr[1] << 8) | ((uint32_t)tr[2] << 16) | ((uint32_t)tr[3] << 24);
        if (isize > 65536u) return false;  // (bgzip never puts more than 64 KB into a block: not BGZF, leave it to zlib)
        blocks->push_back({pos, clen, xlen, isize, out});
        out += isize;
        pos += clen;
    }
    *total = out;
    return !blocks->empty();
}
bool bgzf_inflate(const uint8_t *f, const std::vector<BgzfBlock> &blocks, uint8_t *dst)
{
    unsigned nt = std::thread::hardware_concurrency();
    if (nt < 1) nt = 1;
    if (nt > 32) nt = 32;
    if ((size_t)nt > blocks.size()) nt = (unsigned)blocks.size();
    std::atomic<bool> ok(true);
    auto work = [&](size_t b0, size_t b1) {
        z_stream z;
        memset(&z, 0, sizeof z);
        if (inflateInit2(&z, -15) != Z_OK) { ok = false; return; }
        for (size_t b = b0; b < b1 && ok; b++) {
            const BgzfBlock &k = blocks[b];
            z.next_in = const_cast<Bytef *>(f + k.off + 12 + k.xlen);
            z.avail_in = (uInt)(k.clen - 12 - k.xlen - 8);
            z.next_out = dst + k.out;
            z.avail_out = k.isize;
            const int r = k.isize || z.avail_in ? inflate(&z, Z_FINISH) : Z_STREAM_END;
            const uint8_t *tr = f + k.off + k.clen - 8;
            const uint32_t crc = tr[0] | ((uint32_t)tr[1] << 8) | ((uint32_t)tr[2] << 16) | ((uint32_t)tr[3] << 24);
            if (r != Z_STREAM_END || z.avail_out != 0 || (uint32_t)crc32(crc32(0L, Z_NULL, 0), dst + k.out, k.isize) != crc) ok = false;
            inflateReset(&z);
        }
        inflateEnd(&z);
    };
    std::vector<std::thread> th;
    const size_t per = (blocks.size() + nt - 1) / nt;
    for (unsigned t = 1; t < nt; t++) th.emplace_back(work, std::min(blocks.size(), t * per), std::min(blocks.size(), (t + 1) * per));
    work(0, std::min(blocks.size(), per));
    for (auto &t : th) t.join();
    return ok;
}

// ---- the compressed kind ------------------------------------------------------------------------------------------------------------
size_t FileBytes::member_at(size_t text_off) const
{
    size_t lo = 0, hi = blocks.size();  // the last member with out <= text_off: the empty ones before it share its `out` and come first
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        if (blocks[mid].out <= text_off) lo = mid; else hi = mid;
    }
    return lo;
}
// text [off, off + len) through the serial decoder of inflate_format.h, member by member (CRC-32 and length checked like the device does)
bool FileBytes::read_gz(size_t off, size_t len, uint8_t *dst) const
{
    if (off > size || len > size - off) return false;
    if (!len) return true;
    std::vector<uint8_t> text(INF_MAX_OUT);
    for (size_t k = member_at(off); len; k++) {
        if (k >= blocks.size()) return false;
        const BgzfBlock &b = blocks[k];
        const uint8_t *body = gz + b.off + 12 + b.xlen, *tr = gz + b.off + b.clen - 8;
        const uint32_t crc = tr[0] | ((uint32_t)tr[1] << 8) | ((uint32_t)tr[2] << 16) | ((uint32_t)tr[3] << 24);
        int err = INF_OK;
        inflate_member_host(body, (uint32_t)(b.clen - 12 - b.xlen - 8), text.data(), b.isize, &err);
        if (err != INF_OK || (uint32_t)crc32(crc32(0L, Z_NULL, 0), text.data(), b.isize) != crc) return false;
        const size_t from = off - b.out, take = std::min<size_t>(len, b.isize - from);  // (off >= b.out; an empty member gives nothing)
        memcpy(dst, text.data() + from, take);
        dst += take; off += take; len -= take;
    }
    return true;
}
static void file_bytes_drop_gz(FileBytes *fb)
{
    if (fb->map) munmap(fb->map, fb->map_len);
    if (fb->fd >= 0) close(fb->fd);
    fb->map = nullptr; fb->map_len = 0; fb->fd = -1;
    fb->gz = nullptr; fb->gz_len = 0; fb->blocks.clear(); fb->owned.clear(); fb->head_len = 0; fb->size = 0;
}
bool file_bytes_to_host(FileBytes *fb)
{
    const std::string path = fb->path;
    file_bytes_drop_gz(fb);
    return load_bytes(path.c_str(), fb, false);
}

// reader (load_data.rs:240-251): ".gz" by extension (multi-member), plain otherwise
bool load_bytes(const char *path, FileBytes *fb, bool gz_device)
{
    const size_t n = strlen(path);
    fb->path = path;
    if (n >= 3 && strcmp(path + n - 3, ".gz") == 0) {
        {   // block-compressed (bgzip)?  then in parallel
            const int fd = open(path, O_RDONLY);
            struct stat st;
            if (fd >= 0 && fstat(fd, &st) == 0 && st.st_size > 0 && !getenv("CELLECTOR_NO_BGZF")) {
                void *m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
                if (m != MAP_FAILED) {
                    std::vector<BgzfBlock> blocks;
                    size_t total = 0;
                    bool done = false;
                    try {
                        if (gz_device && bgzf_index((const uint8_t *)m, (size_t)st.st_size, &blocks, &total)) {
                            // left compressed: the device inflates it (option gz_device); only the head's members here
                            fb->map = m; fb->map_len = (size_t)st.st_size; fb->fd = fd;
                            fb->gz = (const uint8_t *)m; fb->gz_len = (size_t)st.st_size;
                            fb->blocks = std::move(blocks);
                            fb->size = total;
                            fb->head_len = std::min<size_t>(total, FB_HEAD);
                            fb->owned.resize(fb->head_len ? fb->head_len : 1);
                            if (fb->read_gz(0, fb->head_len, fb->owned.data())) return true;
                            // (a damaged member among the first: the host reader below decides, as it does without the option)
                            fb->map = nullptr; fb->map_len = 0; fb->fd = -1;
                            fb->gz = nullptr; fb->gz_len = 0; fb->blocks.clear(); fb->owned.clear(); fb->head_len = 0; fb->size = 0;
                            blocks.clear();
                            total = 0;
                        }
                        if (bgzf_index((const uint8_t *)m, (size_t)st.st_size, &blocks, &total)) {
                            fb->owned.resize(total ? total : 1);
                            done = bgzf_inflate((const uint8_t *)m, blocks, fb->owned.data());
                            if (done) { fb->data = fb->owned.data(); fb->size = total; }
                        }
                    } catch (const std::exception &) {  // (no room for the index or the text: the serial reader decides)
                        done = false;
                    }
                    munmap(m, (size_t)st.st_size);
                    if (done) { close(fd); return true; }
                    fb->owned.clear();  // (a damaged block: the serial reader below reports what zlib makes of the file)
                }
            }
            if (fd >= 0) close(fd);
        }
        gzFile gz = gzopen(path, "rb");
        if (!gz) return false;
        gzbuffer(gz, 1 << 20);
        size_t cap = 1 << 24, len = 0;
        fb->owned.resize(cap);
        for (;;) {
            if (len == cap) fb->owned.resize(cap *= 2);
            const int got = gzread(gz, fb->owned.data() + len, (unsigned)std::min<size_t>(cap - len, 1u << 30));
            if (got < 0) {  // a damaged stream (CRC, truncated member): the reference's decoder fails the read as well
                gzclose(gz);
                return false;
            }
            if (got == 0) break;
            len += (size_t)got;
        }
        if (gzclose(gz) != Z_OK) return false;  // (a file that ends inside a member: gzread hands out what came before, only the close says so)
        fb->data = fb->owned.data();
        fb->size = len;
        return true;
    }
    fb->fd = open(path, O_RDONLY);
    if (fb->fd < 0) return false;
    struct stat st;
    if (fstat(fb->fd, &st) != 0) return false;
    fb->size = (size_t)st.st_size;
    const char *um = getenv("CELLECTOR_UNMAPPED_MIN");  // (tests: the unmapped path on small files)
    if (fb->size >= (um ? (size_t)strtoull(um, nullptr, 10) : (size_t)FB_UNMAPPED) && fb->size > 0) {
        fb->head_len = std::min<size_t>(fb->size, FB_HEAD);
        fb->owned.resize(fb->head_len);
        return fb->read(0, fb->head_len, fb->owned.data());
    }
    if (fb->size) {
        fb->map = mmap(nullptr, fb->size, PROT_READ, MAP_PRIVATE, fb->fd, 0);
        if (fb->map == MAP_FAILED) { fb->map = nullptr; return false; }
        fb->map_len = fb->size;
        madvise(fb->map, fb->size, MADV_SEQUENTIAL);
        fb->data = (const uint8_t *)fb->map;
    }
    return true;
}

// consume_mtx_header (load_data.rs:206-223): exactly three lines; returns the offset of the first data byte
size_t skip_header(const FileBytes &fb, std::string *third)
{
    size_t pos = 0;
    for (int x = 0; x < 3; x++) {
        // (an unmapped file: the three lines are looked for in its first FB_HEAD bytes)
        const uint8_t *hd = fb.head();
        const size_t hn = fb.head_size();
        const void *nl = pos < hn ? memchr(hd + pos, '\n', hn - pos) : nullptr;
        const size_t end = nl ? (size_t)((const uint8_t *)nl - hd) : hn;
        if (x == 2 && third) third->assign((const char *)hd + pos, end - pos);
        pos = nl ? end + 1 : hn;
    }
    return pos;
}

bool host_tok_u64(const std::string &s, int idx, uint64_t *out)
{
    size_t p = 0;
    for (int t = 0;; t++) {
        while (p < s.size() && isspace((unsigned char)s[p])) p++;
        if (p >= s.size()) return false;
        size_t b = p;
        while (p < s.size() && !isspace((unsigned char)s[p])) p++;
        if (t == idx) {
            if (s[b] == '+') b++;
            if (b == p) return false;
            uint64_t v = 0;
            for (; b < p; b++) {
                if (s[b] < '0' || s[b] > '9') return false;
                v = v * 10 + (uint64_t)(s[b] - '0');
            }
            *out = v;
            return true;
        }
    }
}

cellector_status mtx_input_open(const char *alt_path, const char *ref_path, MtxInput **out, std::string *msg, bool gz_device)
{
    MtxInput *in = new (std::nothrow) MtxInput();
    if (!in) { *msg = "out of host memory"; return CELLECTOR_ENOMEM; }
    cellector_status st = CELLECTOR_OK;
    std::string third;
    bool ok_a = false, ok_r = false;
    {   // the two files are independent byte streams: inflate / map them concurrently
        std::thread ta([&] { ok_a = load_bytes(alt_path, &in->fa, gz_device); });
        ok_r = load_bytes(ref_path, &in->fr, gz_device);
        ta.join();
    }
    if (!ok_a || !ok_r) {
        st = CELLECTOR_EIO;
        *msg = std::string("couldn't open file ") + (!ok_a ? alt_path : ref_path);
    } else {
        in->off_a = skip_header(in->fa, nullptr);
        in->off_r = skip_header(in->fr, &third);
        if (!host_tok_u64(third, 0, &in->total_loci) || !host_tok_u64(third, 1, &in->total_cells)) {
            st = CELLECTOR_EPARSE;
            *msg = std::string("cannot parse the matrix market size line of ") + ref_path;
        } else if (!host_tok_u64(third, 2, &in->nnz_hint) || in->nnz_hint > (in->fr.size - in->off_r) / 4)
            in->nnz_hint = 0;  // (a line holds at least "1 1 1": a hint beyond the bytes there are is nonsense)
    }
    if (st != CELLECTOR_OK) {
        delete in;
        return st;
    }
    *out = in;
    return CELLECTOR_OK;
}

void mtx_input_close(MtxInput *in) { delete in; }
