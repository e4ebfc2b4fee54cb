// Stand-alone driver of csrc/bgzf_format.h on a CPU (tests/test_bgzf_host.py builds it with the address and undefined-behaviour
// sanitizers and runs it as a program):
//   bgzf_host_main compress IN OUT   IN as a BGZF stream, block by block through bgzf_encode_block_host, then the EOF member
//   bgzf_host_main preset            the preset's code lengths, the table's bit count and bits, one line each
#include <cstdio>
#include <cstring>
#include <vector>

#include "../cellector_amd/csrc/bgzf_format.h"

static int compress(const char *in_path, const char *out_path)
{
    FILE *f = fopen(in_path, "rb");
    if (!f) { perror(in_path); return 2; }
    std::vector<uint8_t> in;
    uint8_t buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) in.insert(in.end(), buf, buf + k);
    fclose(f);
    BgzfTables *t = new BgzfTables;
    bgzf_tables_build(t);
    std::vector<uint8_t> out, member(BGZF_MAX_MEMBER + 8);
    unsigned long long blocks = 0, stored_blocks = 0;
    for (size_t at = 0; at < in.size(); at += BGZF_PAYLOAD) {
        const uint32_t n = (uint32_t)(in.size() - at < BGZF_PAYLOAD ? in.size() - at : BGZF_PAYLOAD);
        // an exact copy of the block: a read outside it is a read outside an allocation
        std::vector<uint8_t> block(in.begin() + at, in.begin() + at + n);
        bool stored = false;
        const uint32_t size = bgzf_encode_block_host(t, block.data(), n, member.data(), &stored);
        if (size > BGZF_MAX_MEMBER) { fprintf(stderr, "member of %u bytes\n", size); return 3; }
        out.insert(out.end(), member.begin(), member.begin() + size);
        blocks++;
        stored_blocks += stored;
    }
    delete t;
    out.insert(out.end(), BGZF_EOF, BGZF_EOF + BGZF_EOF_BYTES);
    f = fopen(out_path, "wb");
    if (!f) { perror(out_path); return 2; }
    const bool ok = fwrite(out.data(), 1, out.size(), f) == out.size();
    if (fclose(f) != 0 || !ok) { perror(out_path); return 2; }
    printf("blocks %llu stored_blocks %llu\n", blocks, stored_blocks);
    return 0;
}

static int preset()
{
    printf("litlen");
    for (int k = 0; k < 286; k++) printf(" %d", BGZF_LITLEN_LENGTHS[k]);
    printf("\ndist");
    for (int k = 0; k < 30; k++) printf(" %d", BGZF_DIST_LENGTHS[k]);
    printf("\nheader_bits %u\nheader ", BGZF_HEADER_BITS);
    for (uint32_t k = 0; k < (BGZF_HEADER_BITS + 7u) / 8u; k++) printf("%02x", (BGZF_HEADER[k >> 2] >> (8 * (k & 3u))) & 0xffu);
    printf("\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 4 && !strcmp(argv[1], "compress")) return compress(argv[2], argv[3]);
    if (argc == 2 && !strcmp(argv[1], "preset")) return preset();
    fprintf(stderr, "usage: %s compress IN OUT | preset\n", argv[0]);
    return 1;
}
