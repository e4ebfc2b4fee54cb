// One body line of a MatrixMarket coordinate file, `locus0+1 SEP cell0+1 SEP value\n`, rendered from a staged entry: which value
// a (file, mode) writes, how long its line is, and its bytes.  Plain decimal, no sign, padding or exponent.  The same code runs
// on the device (kernels_mtx_write.hip) and on the host (tools/mtx_format_check.cpp drives it on a CPU); cellector_amd/mtx_write.py
// is the byte-identical numpy twin.  No division by a variable: digit counts come from compares, digits from a multiply-high by
// the constant of 1 / 10.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MTXF_HD __host__ __device__ __forceinline__
#else
#define MTXF_HD inline
#endif

// (= CELLECTOR_WRITE_* of include/cellector_ffi.h; tools/mtx_format_check.cpp includes this header alone)
#define MTXF_ALIGNED 0
#define MTXF_SPARSE 1
#define MTXF_DEPTH 2
// the longest line: two indices of 2^32 (10 digits each), a value of 131070 (6 digits), two separators, the newline
#define MTXF_MAX_LINE 29

// The third token of the entry's line in file `which` (0 / 1) under `mode`, and whether the file has a line for the entry at all:
// ALIGNED writes every entry with its alt (file 0) or ref (file 1); SPARSE the same two values where they are above 0; DEPTH alt
// where alt > 0 and alt + ref where alt + ref > 0 (at most 131070).
MTXF_HD bool mtxf_value(uint32_t alt, uint32_t ref, int which, int mode, uint32_t *value)
{
    const uint32_t v = which == 0 ? alt : (mode == MTXF_DEPTH ? alt + ref : ref);
    *value = v;
    return mode == MTXF_ALIGNED || v > 0;
}

// decimal digits of v <= 2^32 (a 1-based index, formed in 64 bits) or of a count
MTXF_HD uint32_t mtxf_digits(uint64_t v)
{
    return 1u + (v >= 10ull) + (v >= 100ull) + (v >= 1000ull) + (v >= 10000ull) + (v >= 100000ull) + (v >= 1000000ull) + (v >= 10000000ull) +
           (v >= 100000000ull) + (v >= 1000000000ull);
}

MTXF_HD uint32_t mtxf_line_len(uint32_t locus0, uint32_t cell0, uint32_t value)
{
    return mtxf_digits((uint64_t)locus0 + 1) + mtxf_digits((uint64_t)cell0 + 1) + mtxf_digits(value) + 3u;
}

// v / 10 for any 32-bit v: the high part of v * ceil(2^35 / 10)
MTXF_HD uint32_t mtxf_div10(uint32_t v) { return (uint32_t)(((uint64_t)v * 0xCCCCCCCDull) >> 35); }

// the d = mtxf_digits(v) digits of v <= 2^32 at p; returns p + d.  A tenth digit is 1..4 and comes from compares; the rest fits
// 32 bits.
MTXF_HD uint8_t *mtxf_put(uint8_t *p, uint64_t v, uint32_t d)
{
    uint32_t lo = (uint32_t)v, n = d;
    if (d == 10u) {
        const uint32_t top = 1u + (v >= 2000000000ull) + (v >= 3000000000ull) + (v >= 4000000000ull);
        *p++ = (uint8_t)('0' + top);
        lo = (uint32_t)(v - (uint64_t)top * 1000000000ull);
        n = 9u;
    }
    for (uint32_t k = n; k-- > 0;) {
        const uint32_t q = mtxf_div10(lo);
        p[k] = (uint8_t)('0' + (lo - q * 10u));
        lo = q;
    }
    return p + n;
}

// the line of (locus0, cell0, value) at p, `sep` between its tokens; returns its length = mtxf_line_len of the three
MTXF_HD uint32_t mtxf_render(uint8_t *p, uint32_t locus0, uint32_t cell0, uint32_t value, uint8_t sep)
{
    uint8_t *q = p;
    const uint64_t a = (uint64_t)locus0 + 1, b = (uint64_t)cell0 + 1;
    q = mtxf_put(q, a, mtxf_digits(a)); *q++ = sep;
    q = mtxf_put(q, b, mtxf_digits(b)); *q++ = sep;
    q = mtxf_put(q, value, mtxf_digits(value)); *q++ = (uint8_t)'\n';
    return (uint32_t)(q - p);
}
