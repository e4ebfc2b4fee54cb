// The bytes of an alt.mtx / ref.mtx pair on the host: plain (mapped or pread) or ".gz" (block-parallel BGZF, serial zlib; or BGZF
// left compressed for the device), and
// the three header lines.  Plain C++: no device code, no ctx (tools/mtx_bytes_check.cpp drives it on a CPU).
#pragma once
#include <sys/mman.h>
#include <unistd.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/cellector_ffi.h"

struct BgzfBlock { size_t off, clen; uint32_t xlen, isize; size_t out; };

// the bytes of one input file: inflated into `owned` (.gz), mapped (plain, below FB_UNMAPPED), or — a plain file of
// FB_UNMAPPED bytes and more — not mapped at all: its windows are pread() straight into the pinned upload buffers.  (Mapping 2 x 31 GB meant
// 15 M page-table entries to fault in and to tear down again: the munmap alone took 0.7 s, during which the runtime's
// own allocations queue for the address-space lock.)  A third kind (load_bytes with gz_device, option "gz_device"): a BGZF ".gz"
// left COMPRESSED, the file mapped (`gz`) with its member index (`blocks`); size is the inflated size, data is null, owned holds
// the first FB_HEAD bytes of TEXT, and read() inflates the members that cover a range on the host (small ranges only: the
// device inflates the rest, kernels_inflate.hip).
#define FB_UNMAPPED (1ull << 30)
struct FileBytes {
    const uint8_t *data = nullptr;  // null: unmapped or compressed, use read()
    size_t size = 0;
    void *map = nullptr;
    size_t map_len = 0;
    int fd = -1;
    std::vector<uint8_t> owned;  // .gz: the inflated file; unmapped, compressed: its first FB_HEAD bytes of text (the header lines)
    size_t head_len = 0;
    const uint8_t *gz = nullptr;  // compressed kind: the mapped file
    size_t gz_len = 0;
    std::vector<BgzfBlock> blocks;
    std::string path;
    bool read_gz(size_t off, size_t len, uint8_t *dst) const;  // (mtx_bytes.cpp)
    size_t member_at(size_t text_off) const;                   // the member that holds text byte text_off < size
    ~FileBytes()
    {
        if (map) munmap(map, map_len);
        if (fd >= 0) close(fd);
    }
    const uint8_t *head() const { return data ? data : owned.data(); }
    size_t head_size() const { return data ? size : head_len; }
    bool read(size_t off, size_t len, uint8_t *dst) const
    {
        if (gz) return read_gz(off, len, dst);
        if (data) {
            memcpy(dst, data + off, len);
            return true;
        }
        while (len) {
            const ssize_t got = pread(fd, dst, len, (off_t)off);
            if (got <= 0) return false;
            dst += got; off += (size_t)got; len -= (size_t)got;
        }
        return true;
    }
};
#define FB_HEAD (1u << 20)

bool bgzf_index(const uint8_t *f, size_t n, std::vector<BgzfBlock> *blocks, size_t *total);
bool bgzf_inflate(const uint8_t *f, const std::vector<BgzfBlock> &blocks, uint8_t *dst);
bool load_bytes(const char *path, FileBytes *fb, bool gz_device = false);
// a compressed FileBytes becomes an inflated one by the host reader's rules (what load_bytes without gz_device makes of the path);
// false: the host reader refuses the file too
bool file_bytes_to_host(FileBytes *fb);
size_t skip_header(const FileBytes &fb, std::string *third);
bool host_tok_u64(const std::string &s, int idx, uint64_t *out);

struct MtxInput {
    FileBytes fa, fr;
    size_t off_a = 0, off_r = 0;
    uint64_t total_loci = 0, total_cells = 0;
    uint64_t nnz_hint = 0;  // third number of the size line (0: absent); a capacity hint, never trusted
};
// open both files (bytes only) and read the dims from the REF file's third header line (load_data.rs:216-220); a failure
// leaves its words in *msg
cellector_status mtx_input_open(const char *alt_path, const char *ref_path, MtxInput **out, std::string *msg, bool gz_device = false);
void mtx_input_close(MtxInput *in);
