// Drives the host byte reader of the mtx ingest (cellector_amd/csrc/mtx_bytes.cpp) without a GPU:
//   mtx_bytes_check ALT REF OUT_ALT OUT_REF
// opens the pair, prints the dims, the entry-count hint and both data offsets, and writes both data sections, read back through
// FileBytes::read in pieces of a prime length.  A failed open: exit 1, "status N: message" on stderr.  (tests/test_host_mtx_bytes.py)
#include <cstdio>

#include "../cellector_amd/csrc/mtx_bytes.h"

static bool dump(const FileBytes &fb, size_t off, const char *path)
{
    FILE *f = fopen(path, "wb");
    if (!f) return false;
    uint8_t piece[251];
    bool ok = true;
    for (size_t at = off; ok && at < fb.size; at += sizeof piece) {
        const size_t len = fb.size - at < sizeof piece ? fb.size - at : sizeof piece;
        ok = fb.read(at, len, piece) && fwrite(piece, 1, len, f) == len;
    }
    return fclose(f) == 0 && ok;
}

int main(int argc, char **argv)
{
    if (argc != 5) {
        fprintf(stderr, "usage: %s ALT REF OUT_ALT OUT_REF\n", argv[0]);
        return 2;
    }
    MtxInput *in = nullptr;
    std::string msg;
    const cellector_status st = mtx_input_open(argv[1], argv[2], &in, &msg);
    if (st != CELLECTOR_OK) {
        fprintf(stderr, "status %d: %s\n", (int)st, msg.c_str());
        return 1;
    }
    printf("loci %llu\ncells %llu\nnnz_hint %llu\noff_alt %zu\noff_ref %zu\n", (unsigned long long)in->total_loci,
           (unsigned long long)in->total_cells, (unsigned long long)in->nnz_hint, in->off_a, in->off_r);
    const bool ok = dump(in->fa, in->off_a, argv[3]) && dump(in->fr, in->off_r, argv[4]);
    mtx_input_close(in);
    if (!ok) fprintf(stderr, "cannot read back the data sections\n");
    return ok ? 0 : 3;
}
