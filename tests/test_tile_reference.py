"""The cell pass' high-precision reference (tests/tile_reference.py) checked on the CPU: against mpmath, against the oracle,
and the ln C part of the device's bound against the device's own table arithmetic (which is host arithmetic: exact here)."""
import math

import numpy as np
import pytest

import tile_reference as tr


def _random_keys(rng, K):
    """alpha, beta log-uniform in [1, 1e9] (half of them whole numbers like the EM phase's, half not, like the posterior
    phase's), totals 0..200"""
    alpha = 10.0 ** rng.uniform(0, 9, K)
    beta = 10.0 ** rng.uniform(0, 9, K)
    whole = rng.random(K) < 0.5
    alpha = np.where(whole, np.round(alpha), alpha)
    beta = np.where(whole, np.round(beta), beta)
    n = rng.integers(0, 201, K)
    n[: K // 4] = rng.integers(0, 9, K // 4)  # the totals the tiles hold, well represented
    a = (rng.random(K) * (n + 1)).astype(np.int64)
    return alpha, beta, a, n - a


def _ref_tolerance(n, t, partial):
    """module docstring of tile_reference: REF_OPS(n) roundings of 2^-64 at the size of the largest value met, plus the final
    conversion to double (half an ulp)"""
    big = np.maximum(1.0, np.maximum(np.abs(t), partial))
    return tr.ref_ops(n) * 2.0 ** -64 * big + 0.5 * np.spacing(np.abs(t))


def test_longdouble_is_the_x87_format_or_mpmath_takes_over():
    import mpmath  # noqa: F401  (the reference needs it either way: ln C)
    assert tr.HAVE_X87 == (np.finfo(np.longdouble).nmant == 63)


def test_terms_against_mpmath_loggamma_form():
    """2 400 random keys: the product form in longdouble against ln C + lnB(a + alpha, r + beta) - lnB(alpha, beta) with
    mpmath's loggamma at 50 digits.  The claim is about the ABSOLUTE error of a term (a term near zero is far off in ulps of
    itself and still right to 1e-18)."""
    import mpmath as mp
    mp.mp.dps = 50
    rng = np.random.default_rng(20240611)
    alpha, beta, a, r = _random_keys(rng, 2400)
    t, _, partial = tr.term_values(alpha, beta, a, r)
    td = t.astype(np.float64)
    worst = 0.0
    for i in range(len(a)):
        al, be, ai, ri = mp.mpf(float(alpha[i])), mp.mpf(float(beta[i])), int(a[i]), int(r[i])
        want = (mp.log(mp.binomial(ai + ri, ai)) + mp.loggamma(ai + al) + mp.loggamma(ri + be) - mp.loggamma(ai + ri + al + be)
                - mp.loggamma(al) - mp.loggamma(be) + mp.loggamma(al + be))
        tol = float(_ref_tolerance(ai + ri, float(want), partial[i]))
        # the longdouble value itself (hi + lo), then the double it rounds to
        hi = float(t[i])
        lo = float(t[i] - np.longdouble(hi))
        err_ld = abs(float(mp.mpf(hi) + mp.mpf(lo) - want))
        err_d = abs(float(mp.mpf(float(td[i])) - want))
        assert err_ld <= tol - 0.5 * np.spacing(abs(float(want))) + 1e-300, (i, ai, ri, alpha[i], beta[i], err_ld, tol)
        assert err_d <= tol, (i, ai, ri, alpha[i], beta[i], err_d, tol)
        worst = max(worst, err_ld / max(tol, 1e-300))
    print(f"longdouble terms vs mpmath: worst error / allowed = {worst:.3f}")


def test_expected_terms_against_mpmath():
    """ln sum pmf(k)^2 from the same products against mpmath, 300 keys (totals up to 60: the sum has n + 1 terms of n factors)"""
    rng = np.random.default_rng(7)
    alpha, beta, a, r = _random_keys(rng, 300)
    n = np.minimum(a + r, 60)
    e = tr.expected_values(alpha, beta, n)
    for i in range(len(n)):
        want = tr.expected_mp(alpha[i], beta[i], n[i])
        # n + 1 pmfs of 3 n + 3 roundings each, squared (x 2, + 1), summed (+ n), one log: (7 n + 8) units of 2^-64 relative
        tol = (7 * int(n[i]) + 8) * 2.0 ** -64 * max(1.0, abs(float(want))) + 0.5 * np.spacing(abs(float(want)))
        assert abs(float(want) - float(e[i])) <= tol, (i, n[i], alpha[i], beta[i])


def test_oracle_within_its_depth_tolerance_of_the_reference(oracle_lib):
    """Ties the two checkers together: the oracle's ln_gamma-difference form lies within 8 eps lnGamma(alpha + beta + n) of the
    reference (the per-entry depth tolerance tests/test_gpu_deep.py states), on 500 keys."""
    L_ = oracle_lib.lib()
    rng = np.random.default_rng(99)
    alpha, beta, a, r = _random_keys(rng, 500)
    t = tr.term_values(alpha, beta, a, r)[0].astype(np.float64)
    eps = 2.220446049250313e-16
    worst = 0.0
    for i in range(500):
        n = int(a[i] + r[i])
        got = L_.orc_log_beta_binomial_pmf(float(a[i]), float(r[i]), float(alpha[i]), float(beta[i]), L_.orc_ln_binomial(n, int(a[i])))
        tol = 8 * eps * max(1.0, math.lgamma(alpha[i] + beta[i] + n))
        assert abs(got - t[i]) <= tol, (i, a[i], r[i], alpha[i], beta[i], got, t[i], tol)
        worst = max(worst, abs(got - t[i]) / tol)
    print(f"oracle vs reference: worst |diff| / depth tolerance = {worst:.3f}")


def test_zero_total_entries_and_masked_loci():
    """Q14 and the mask: an alt = ref = 0 entry adds exactly 0.0 and counts; entries at masked loci do neither."""
    lo = np.array([0, 1, 2, 2, 1]); ce = np.array([0, 0, 0, 1, 1])
    al = np.array([0, 2, 1, 0, 3]); re = np.array([0, 1, 0, 0, 0])
    alpha = np.array([3.5, 2.25, 7.0]); beta = np.array([1.5, 9.0, 2.0])
    full = tr.cell_reference(3, lo, ce, al, re, alpha, beta)
    assert full["loci_used"].tolist() == [3.0, 2.0, 0.0]
    assert full["ll"][2] == 0.0 and full["expected_ll"][2] == 0.0
    want0 = float(tr.term_mp(2.25, 9.0, 2, 1) + tr.term_mp(7.0, 2.0, 1, 0))
    assert abs(full["ll"][0] - want0) < 1e-15
    assert full["term"][0] == 0.0 and full["eterm"][0] == 0.0 and full["term"][3] == 0.0
    masked = tr.cell_reference(3, lo, ce, al, re, alpha, beta, mask=np.array([1, 0, 1]))
    assert masked["loci_used"].tolist() == [2.0, 1.0, 0.0]
    assert abs(masked["ll"][0] - float(tr.term_mp(7.0, 2.0, 1, 0))) < 1e-16 and masked["ll"][1] == 0.0
    assert masked["abs_ll"][0] == abs(masked["ll"][0]) and masked["count"].tolist() == [2, 1, 0]


def test_ln_choose_bound_against_the_factorial_table_arithmetic():
    """The device's ln C(n, a) = lf[n] - lf[a] - lf[n - a] is host arithmetic (lf = log of the running f64 product 1 * 2 * ... * x,
    cellector_create; two IEEE subtractions on the device), so its error against the exact ln C(n, a) is measured here for
    every n <= 170 and every a.

    The sweep's figure for it is half an ulp of ln(n!) per table value, 1.5 ulp in all (tile_reference.ln_choose_bound).  That
    figure leaves out the two subtractions (half an ulp of ln(n!) each at most) and the roundings of the running product
    (x - 22 of them in x!, the products up to 22! being exact): the complete count is asserted for every (n, a), the sweep's
    figure for every total the sweep draws (n <= 64 and the probes' 171 and 240 take their a, r <= 170 from the table).
    Measured: the 1.5 ulp figure holds for every n <= 170 but 125 (C(125, 40): 1.03 of it); worst below 65 is 0.93 at n = 40."""
    import mpmath as mp
    mp.mp.dps = 50
    f, lf = 1.0, [0.0]
    for i in range(1, 171):
        f *= float(i)
        lf.append(math.log(f))
    lnf = [mp.log(mp.factorial(x)) for x in range(171)]
    worst, over = (0.0, 0, 0), []
    for n in range(171):
        ulp_n = float(np.spacing(math.lgamma(n + 1.0)))
        for a in range(n + 1):
            got = lf[n] - lf[a] - lf[n - a]
            err = abs(float(mp.mpf(got) - (lnf[n] - lnf[a] - lnf[n - a])))
            bound = tr.ln_choose_bound(n, a)
            full = bound + (ulp_n if n >= 2 else 0.0) + sum(max(0, x - 22) for x in (n, a, n - a)) * tr.U53
            assert err <= full, (n, a, err, full)
            if n <= 64:
                assert err <= bound, (n, a, err, bound)
            elif err > bound:
                over.append((n, a, err / bound))
            if bound > 0 and err / bound > worst[0]:
                worst = (err / bound, n, a)
    print(f"ln C table arithmetic: worst error / (1.5 ulp of ln n!) = {worst[0]:.3f} at C({worst[1]}, {worst[2]}); "
          f"beyond it above n = 64: {[(n, a, round(q, 3)) for n, a, q in over]}")
