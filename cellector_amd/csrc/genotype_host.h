// The genotype rule of output_final_vcf (main.rs:79-124) on the host, stated for one (class, locus), and the statrs pieces under it
// (SURVEY Appendix B.1, B.2, B.4): ln_gamma, ln_factorial and Binomial::pmf.  The reference (Rust f64::exp / ln) and the CPU oracle
// (orc_vcf_genotype) call the C library's exp and log, so does this file: with ambient = 0.03 and threshold = 0.99 the result for
// (a, r, A, R) is bit for bit the oracle's minority output for orc_vcf_genotype(a, r, A - a, R - r).
//
// No HIP in this file: api_classes.cpp (cellector_class_genotypes) and host/cellector.cpp (the two VCF writers) include it, and
// tests/test_genotype_reference.py builds it as plain C++.  Scalar code and explicit expression order only; compile without
// contraction (-ffp-contract=off; clang also gets the pragma).
//
// The reference's quirk is kept: at deep tallies all three pmfs can underflow to 0; then den is 0, every q is 0 / 0 = NaN, gp is
// NaN (fmax of NaNs) and gt is 0 ("./."), since no comparison with a NaN holds.  A log-space variant would change the reference's
// output and is not offered.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// statrs gamma::ln_gamma for x >= 0.5 (Appendix B.1): the Lanczos sum with g = 10.900511, n = 11
static inline double genotype_ln_gamma(double x)
{
    static const double dk[11] = {2.48574089138753565546e-5,  1.05142378581721974210,    -3.45687097222016235469,
                                  4.51227709466894823700,     -2.98285225323576655721,   1.05639711577126713077,
                                  -1.95428773191645869583e-1, 1.70970543404441224307e-2, -5.71926117404305781283e-4,
                                  4.63399473359905636708e-6,  -2.71994908488607703910e-9};
    double s = dk[0];
    for (int i = 1; i <= 10; i++) s += dk[i] / (x + (double)i - 1.0);
    return std::log(s) + 0.6207822376352452223455184457816472122518527279025978 +
           (x - 0.5) * std::log((x - 0.5 + 10.900511) / 2.71828182845904523536028747135266250);
}

// statrs factorial::ln_factorial (Appendix B.2): the log of the cached running product up to 170!, ln_gamma(x + 1) above
static inline double genotype_ln_factorial(uint64_t x)
{
    struct Cache {  // statrs FCACHE: running f64 product (built once; thread-safe initialisation)
        double v[171];
        Cache()
        {
            v[0] = 1.0;
            for (int i = 1; i <= 170; i++) v[i] = v[i - 1] * (double)i;
        }
    };
    static const Cache cache;
    return x <= 170 ? std::log(cache.v[x]) : genotype_ln_gamma((double)x + 1.0);
}

// statrs Binomial::pmf (Appendix B.4)
static inline double genotype_binomial_pmf(double p, uint64_t n, uint64_t k)
{
    if (k > n) return 0.0;
    if (p == 0.0) return k == 0 ? 1.0 : 0.0;
    if (std::fabs(p - 1.0) <= 4 * 2.220446049250313e-16) return k == n ? 1.0 : 0.0;
    const double lnb = genotype_ln_factorial(n) - genotype_ln_factorial(k) - genotype_ln_factorial(n - k);
    return std::exp(lnb + (double)k * std::log(p) + (double)(n - k) * std::log(1.0 - p));
}

// main.rs:79-92 for one locus: the ambient ("soup") alt fraction from the locus' totals over ALL cells, and the alt probability of
// a read under each genotype with `ambient` of the reads coming from the soup.  p = {hom-alt, het, hom-ref}.
struct GenotypeLocus { double p[3]; };
static inline GenotypeLocus genotype_locus(uint64_t total_alt, uint64_t total_ref, double ambient)
{
    const double soup = total_alt + total_ref > 0 ? (double)total_alt / (double)(total_alt + total_ref) : 0.5;
    GenotypeLocus g;
    g.p[0] = (1.0 - ambient) * 0.99 + ambient * soup;
    g.p[1] = (1.0 - ambient) * 0.5 + ambient * soup;
    g.p[2] = (1.0 - ambient) * 0.01 + ambient * soup;
    return g;
}

// main.rs:93-124 for one class at that locus: the three posteriors under a flat prior (q = {alt, het, ref}), their maximum, and the
// call: 1 = "1/1", 2 = "0/1", 3 = "0/0", 0 = "./." (the oracle's codes)
struct GenotypeCall { double q[3], gp; uint8_t gt; };
static inline GenotypeCall genotype_call(const GenotypeLocus &g, uint64_t alt, uint64_t ref, double threshold)
{
    const double l_alt = genotype_binomial_pmf(g.p[0], alt + ref, alt), l_het = genotype_binomial_pmf(g.p[1], alt + ref, alt),
                 l_ref = genotype_binomial_pmf(g.p[2], alt + ref, alt);
    const double den = 1.0 / 3.0 * l_alt + 1.0 / 3.0 * l_het + 1.0 / 3.0 * l_ref;
    GenotypeCall c;
    c.q[0] = l_alt * 1.0 / 3.0 / den;
    c.q[1] = l_het * 1.0 / 3.0 / den;
    c.q[2] = l_ref * 1.0 / 3.0 / den;
    c.gp = std::fmax(std::fmax(c.q[0], c.q[1]), c.q[2]);
    c.gt = c.q[0] > threshold ? 1 : c.q[1] > threshold ? 2 : c.q[2] > threshold ? 3 : 0;
    return c;
}

static inline const char *genotype_string(uint8_t gt)
{
    static const char *const s[4] = {"./.", "1/1", "0/1", "0/0"};
    return s[gt & 3];
}
