// Drives the line renderer of the mtx writer (cellector_amd/csrc/mtx_format.h, the code the kernels run) without a GPU:
//   mtx_format_check WHICH MODE SEP < entries > lines
// WHICH 0 / 1, MODE 0 aligned / 1 sparse / 2 depth, SEP t / s.  stdin: one `locus0 cell0 alt ref` per line; stdout: the body
// lines of the file for those entries.  Every line is rendered into the middle of a canary-filled buffer: a length that is not
// mtxf_line_len, a byte outside it or a line above MTXF_MAX_LINE is exit 3.  (tests/test_host_mtx_format.py)
#include <cstdio>
#include <cstring>

#include "../cellector_amd/csrc/mtx_format.h"

int main(int argc, char **argv)
{
    if (argc != 4 || (argv[3][0] != 't' && argv[3][0] != 's')) {
        fprintf(stderr, "usage: %s WHICH MODE t|s < entries > lines\n", argv[0]);
        return 2;
    }
    const int which = argv[1][0] - '0', mode = argv[2][0] - '0';
    const uint8_t sep = argv[3][0] == 't' ? '\t' : ' ';
    unsigned long long l0, c0, a, r;
    while (scanf("%llu %llu %llu %llu", &l0, &c0, &a, &r) == 4) {
        uint32_t value;
        if (!mtxf_value((uint32_t)a, (uint32_t)r, which, mode, &value)) continue;
        uint8_t buf[16 + MTXF_MAX_LINE + 16];
        memset(buf, 0xA5, sizeof buf);
        const uint32_t want = mtxf_line_len((uint32_t)l0, (uint32_t)c0, value);
        const uint32_t len = mtxf_render(buf + 16, (uint32_t)l0, (uint32_t)c0, value, sep);
        bool ok = len == want && len <= MTXF_MAX_LINE;
        for (size_t i = 0; i < sizeof buf; i++)
            if ((i < 16 || i >= 16 + (size_t)len) && buf[i] != 0xA5) ok = false;
        if (!ok) {
            fprintf(stderr, "entry %llu %llu %llu %llu: rendered %u bytes, mtxf_line_len %u, or a byte outside the line\n", l0, c0, a, r, len, want);
            return 3;
        }
        fwrite(buf + 16, 1, len, stdout);
    }
    return 0;
}
