// The last steps of calculate_posteriors (main.rs:266-278) and the rule of output_final_assignments (main.rs:145-169) on the
// host, with the C library: the reference (Rust f64::exp / ln / log10) and the CPU oracle call these very functions, so the
// cells option resolve_posteriors evaluates get their posterior, label and qual from here and not from the device's exp / log.
//
// No HIP in this file: api_posteriors.cpp includes it, and tests/test_ref_log_posterior.py builds it as plain C++.  Scalar code
// and explicit expression order only; compile without contraction (-ffp-contract=off; clang also gets the pragma).
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// stats.rs:35-39
static inline double assign_logsumexp(double a, double b)
{
    const double m = std::fmax(a, b);
    const double sum = std::exp(a - m) + std::exp(b - m);
    return m + std::log(sum);
}

// main.rs:266-278 for one cell: the three per-cell LLs and the three log priors in, posterior and doublet posterior out
static inline void assign_posterior(double ll_min, double ll_maj, double ll_dbl, double lp_min, double lp_maj, double lp_dbl,
                                    double *posterior, double *doublet)
{
    const double log_num = lp_min + ll_min;
    double log_den = assign_logsumexp(log_num, lp_maj + ll_maj);
    const double log_dbl = lp_dbl + ll_dbl;
    log_den = assign_logsumexp(log_den, log_dbl);
    *posterior = std::exp(log_num - log_den);
    *doublet = std::exp(log_dbl - log_den);
}

// main.rs:145-157: 0 "0", 1 "1", 2 "doublet", 3 "unassigned"
static inline uint8_t assign_label(double posterior, double doublet, uint64_t n_entries, double threshold, uint64_t min_loci_used)
{
    uint8_t a = 3;
    if (posterior > threshold) a = 0;
    else if (1.0 - posterior > threshold) a = 1;
    if (doublet > 0.5) a = 2;
    if (n_entries < min_loci_used) a = 3;
    return a;
}

// main.rs:165-167: min(-10 log10(1 - max(p, 1 - p)), 255) as usize (f64::min ignores a NaN, the cast saturates)
static inline uint64_t assign_qual(double posterior)
{
    const double post = std::fmax(posterior, 1.0 - posterior);
    const double q = std::fmin(-10.0 * std::log10(1.0 - post), 255.0);
    return (q != q || q < 0.0) ? 0 : (uint64_t)q;
}
