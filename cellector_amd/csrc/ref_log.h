// The C library's natural log, operation for operation, for host and device; the reference's log_beta_binomial_pmf on it.
//
// Option resolve_ties (kernels_resolve.hip) re-evaluates the cells next to an order statistic or the threshold with the
// reference's own arithmetic (stats.rs:41-53, statrs' Lanczos ln_gamma) and promises the reference's bits.  The reference
// (Rust f64::ln) and the CPU oracle call the C library's log; the device maths library's log can differ from it in the
// last place, and so can a correctly rounded one: glibc's log (2.28 and later) is accurate to 0.52 ulp, not correctly
// rounded — a correctly rounded log differed from it on 7 in 10^6 random arguments and on 5 in 10^5 of the arguments the
// Lanczos sum passes to it (measured).  So ref_log repeats that log itself: its constants
// (ref_log_table.h, read out of the C library by tools/gen_ref_log_table.py) and its operations, with the fused
// multiply-adds of its x86-64 FMA build (the variant the C library selects on every CPU with FMA) written out.
//
//   x next to 1 (1 - 2^-4 <= x < 1 + 0x1.09p-4): r = x - 1, log1p(r) by a degree-11 polynomial, r + r^2 B0 in extra precision;
//   else x = 2^k z, z in [0x1.6p-1, 0x1.6p+0); i = 7 bits of z; r = z / c_i - 1 (one fma);
//   log x = k ln2_hi + log c_i + r  +  (k ln2_lo + rounding terms)  +  r^2 (A0 + r A1 + r^2 A2 + r^3 A3 + r^4 A4).
//
// Origin: the algorithm and its constants are glibc's log (sysdeps/ieee754/dbl-64/e_log.c, e_log_data.c, LGPL-2.1+), which
// glibc took from Arm's optimized-routines (math/log.c, log_data.c; MIT OR Apache-2.0 WITH LLVM-exception).  api_options.cpp
// compares ref_log with the host's log on a few arguments before it accepts option resolve_ties (ref_log_matches_host).
//
// Positive finite normal arguments only (the Lanczos sums and arguments of ln_gamma at alpha, beta >= 1 are).  Explicit fma
// only: the file is compiled without contraction (the library and the test build use -ffp-contract=off; clang also gets the
// pragma).  Builds under hipcc (__host__ __device__) and as plain C++ without hip_runtime.h (tests/test_ref_log.py).
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define REF_HD __host__ __device__
#else
#define REF_HD
#endif
#define REF_LOG_TABLE_ATTR static constexpr  // (clang emits a device copy of a constexpr table that device code reads)
#include "ref_log_table.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

REF_HD inline double ref_log(double x)
{
    uint64_t ix;
    memcpy(&ix, &x, sizeof ix);
    const uint64_t LO = 0x3fee000000000000ull;  // 1 - 2^-4
    const uint64_t HI = 0x3ff1090000000000ull;  // 1 + 0x1.09p-4
    if (ix - LO < HI - LO) {
        if (ix == 0x3ff0000000000000ull) return 0.0;
        const double *B = ref_log_b;
        const double r = x - 1.0;
        const double r2 = r * r;
        const double r3 = r * r2;
        const double p3 = __builtin_fma(r3, B[10], __builtin_fma(r2, B[9], __builtin_fma(r, B[8], B[7])));
        const double p2 = __builtin_fma(r3, p3, __builtin_fma(r2, B[6], __builtin_fma(r, B[5], B[4])));
        const double p1 = __builtin_fma(r3, p2, __builtin_fma(r2, B[3], __builtin_fma(r, B[2], B[1])));
        double w = r * 0x1p27;
        const double rhi = r + w - w;
        const double rlo = r - rhi;
        const double rr = rhi * rhi;  // exact (rhi has 26 bits); times B0 = -1/2 exact
        const double hi = __builtin_fma(rr, B[0], r);
        double lo = __builtin_fma(rr, B[0], r - hi);
        lo = __builtin_fma(B[0] * rlo, rhi + r, lo);
        double y = __builtin_fma(r3, p1, lo);
        y += hi;
        return y;
    }
    const uint64_t OFF = 0x3fe6000000000000ull;
    const uint64_t tmp = ix - OFF;
    const int i = (int)((tmp >> 45) % 128);
    const int k = (int)((int64_t)tmp >> 52);
    const uint64_t iz = ix - (tmp & (0xfffull << 52));
    const double invc = ref_log_tab[i][0], logc = ref_log_tab[i][1];
    double z;
    memcpy(&z, &iz, sizeof z);
    const double r = __builtin_fma(z, invc, -1.0);
    const double kd = (double)k;
    const double w = __builtin_fma(kd, REF_LOG_LN2HI, logc);
    const double hi = w + r;
    const double lo = __builtin_fma(kd, REF_LOG_LN2LO, w - hi + r);
    const double *A = ref_log_a;
    const double r2 = r * r;
    const double q = __builtin_fma(r2, __builtin_fma(r, A[4], A[3]), __builtin_fma(r, A[2], A[1]));
    const double y = __builtin_fma(r * r2, q, __builtin_fma(r2, A[0], lo)) + hi;
    return y;
}

// ---- the reference's log_beta_binomial_pmf with ref_log --------------------------------------------------------------
// Operation for operation as dm_ln_gamma / dm_log_bb_pmf_ref (device_math.h) and the CPU oracle: statrs' Lanczos sum
// (x >= 0.5 branch), ln C from the ln-factorial table lf = ln(FCACHE[0..170]) (built with the host's log), ln_gamma(x + 1)
// beyond; (lnGamma(a) + lnGamma(b)) - lnGamma(a + b); (lnC + numerator) - denominator.
REF_HD inline double ref_ln_gamma(double x)
{
    const double dk[11] = {2.48574089138753565546e-5,  1.05142378581721974210,    -3.45687097222016235469,
                           4.51227709466894823700,     -2.98285225323576655721,   1.05639711577126713077,
                           -1.95428773191645869583e-1, 1.70970543404441224307e-2, -5.71926117404305781283e-4,
                           4.63399473359905636708e-6,  -2.71994908488607703910e-9};
    double s = dk[0];
    for (int i = 1; i <= 10; i++) s += dk[i] / (x + (double)i - 1.0);
    return ref_log(s) + 0.6207822376352452223455184457816472122518527279025978 +
           (x - 0.5) * ref_log((x - 0.5 + 10.900511) / 2.71828182845904523536028747135266250);
}
REF_HD inline double ref_ln_factorial(const double *lf, uint32_t x) { return x <= 170u ? lf[x] : ref_ln_gamma((double)x + 1.0); }
REF_HD inline double ref_log_beta_calc(double a, double b)
{
    const double lga = ref_ln_gamma(a);
    const double lgb = ref_ln_gamma(b);
    const double lgab = ref_ln_gamma(a + b);
    return lga + lgb - lgab;
}
REF_HD inline double ref_log_bb_pmf(const double *lf, double alpha, double beta, uint32_t a, uint32_t r)
{
    const double lnc = ref_ln_factorial(lf, a + r) - ref_ln_factorial(lf, a) - ref_ln_factorial(lf, r);
    const double num = ref_log_beta_calc((double)a + alpha, (double)r + beta);
    const double den = ref_log_beta_calc(alpha, beta);
    return lnc + num - den;
}
