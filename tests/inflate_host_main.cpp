// A stand-alone program around inflate_member_host (csrc/inflate_format.h) for tests/test_inflate_reference.py, which builds it with
// the address and undefined-behaviour sanitizers.  Usage: inflate_host_main IN OUT.  IN holds records {u32 n_in, u32 isize, u32 crc,
// n_in bytes of raw deflate}; for each one a line "status produced" goes to stdout (status: the INF_E_ kind, 0 = accepted) and, when
// accepted, the text to OUT.  Every body and every text lives in a heap block of exactly its size, so that a read or a write
// beyond either is a sanitizer report.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../cellector_amd/csrc/inflate_format.h"

static uint32_t u32(const uint8_t *p) { return p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::vector<uint8_t> all;
    uint8_t buf[1 << 16];
    for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) all.insert(all.end(), buf, buf + got);
    fclose(f);
    FILE *o = fopen(argv[2], "wb");
    if (!o) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    for (size_t at = 0; at < all.size();) {
        if (all.size() - at < 12) { fprintf(stderr, "a record is cut short\n"); return 2; }
        const uint32_t n_in = u32(&all[at]), isize = u32(&all[at + 4]), crc = u32(&all[at + 8]);
        at += 12;
        if (all.size() - at < n_in || isize > INF_MAX_OUT) { fprintf(stderr, "a record is cut short or its isize too large\n"); return 2; }
        uint8_t *in = (uint8_t *)malloc(n_in ? n_in : 1), *out = (uint8_t *)malloc(isize ? isize : 1);
        if (n_in) memcpy(in, &all[at], n_in);
        at += n_in;
        int err = 0;
        const uint32_t produced = inflate_member_host(n_in ? in : nullptr, n_in, isize ? out : nullptr, isize, &err);
        if (err == INF_OK && inf_crc32_plain(out, isize) != crc) err = INF_E_CRC;
        printf("%d %u\n", err, produced);
        if (err == INF_OK && isize) fwrite(out, 1, isize, o);
        free(in);
        free(out);
    }
    fclose(o);
    return 0;
}
