// Drives the compressed kind of the host byte reader (cellector_amd/csrc/mtx_bytes.cpp, load_bytes with gz_device) without a GPU:
//   gz_bytes_check ALT REF SEED N_RANGES
// opens the pair the way option gz_device does and prints, per file: "kind" (1: left compressed with its member index, 0: the host
// reader took it), the inflated size, the members, the head (hex of its first 64 bytes), the last byte, and N_RANGES lines
// "off len fnv" of ranges drawn from SEED (an LCG), each read back through FileBytes::read (fnv: FNV-1a of the bytes), then the
// dims and both data offsets.  A failed open: exit 1, "status N: message" on stderr.  (tests/test_inflate_api.py)
#include <cstdio>
#include <cstdlib>

#include "../cellector_amd/csrc/mtx_bytes.h"

static uint64_t fnv(const uint8_t *p, size_t n)
{
    uint64_t h = 1469598103934665603ull;
    for (size_t k = 0; k < n; k++) h = (h ^ p[k]) * 1099511628211ull;
    return h;
}

static bool report(const FileBytes &fb, uint64_t seed, int n_ranges)
{
    printf("kind %d\nsize %zu\nmembers %zu\nhead ", fb.gz ? 1 : 0, fb.size, fb.blocks.size());
    for (size_t k = 0; k < fb.head_size() && k < 64; k++) printf("%02x", fb.head()[k]);
    printf("\n");
    uint8_t last = 0;
    if (fb.size && !fb.read(fb.size - 1, 1, &last)) return false;
    printf("last %d\n", fb.size ? (int)last : -1);
    std::vector<uint8_t> buf;
    for (int r = 0; r < n_ranges; r++) {
        seed = seed * 6364136223846793005ull + 1442695040888963407ull;
        const size_t off = fb.size ? (size_t)((seed >> 33) % fb.size) : 0;
        seed = seed * 6364136223846793005ull + 1442695040888963407ull;
        const size_t len = (size_t)((seed >> 33) % (r % 4 == 0 ? 200000 : 3000)) % (fb.size - off + 1);
        buf.resize(len ? len : 1);
        if (!fb.read(off, len, buf.data())) return false;
        printf("range %zu %zu %llu\n", off, len, (unsigned long long)fnv(buf.data(), len));
    }
    return true;
}

int main(int argc, char **argv)
{
    if (argc != 5) {
        fprintf(stderr, "usage: %s ALT REF SEED N_RANGES\n", argv[0]);
        return 2;
    }
    MtxInput *in = nullptr;
    std::string msg;
    const cellector_status st = mtx_input_open(argv[1], argv[2], &in, &msg, true);
    if (st != CELLECTOR_OK) {
        fprintf(stderr, "status %d: %s\n", (int)st, msg.c_str());
        return 1;
    }
    const uint64_t seed = strtoull(argv[3], nullptr, 10);
    const bool ok = report(in->fa, seed, atoi(argv[4])) && report(in->fr, seed + 1, atoi(argv[4]));
    printf("loci %llu\ncells %llu\noff_alt %zu\noff_ref %zu\n", (unsigned long long)in->total_loci, (unsigned long long)in->total_cells,
           in->off_a, in->off_r);
    mtx_input_close(in);
    if (!ok) fprintf(stderr, "cannot read the files back\n");
    return ok ? 0 : 3;
}
