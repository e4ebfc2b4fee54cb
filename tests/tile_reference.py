"""High-precision reference of the cell pass (get_cell_log_likelihoods, main.rs:541-591) and the device's error bound.

A plain helper for the tests (no fixtures, no GPU): give it the COO arrays in load order, the per-locus alpha / beta and an
optional locus mask; it returns every cell's log-likelihood, expected log-likelihood and loci_used together with what a
bound on a double-precision evaluation needs (sum of |term|, entry count, sum of the per-term bounds).

Per-term values, for the distinct (locus, alt, ref) keys of the matrix (n = alt + ref):

    t = ln C(n, alt) + ln[ prod_{i<alt}(alpha+i) prod_{j<ref}(beta+j) / prod_{k<n}(alpha+beta+k) ]
    e = ln sum_{k=0..n} pmf(k)^2,   pmf(k) = C(n, k) prod_{i<k}(alpha+i) prod_{j<n-k}(beta+j) / prod_{k<n}(alpha+beta+k)

in 80-bit np.longdouble (64-bit mantissa), vectorised over the keys; ln C(n, alt) and C(n, k) come from mpmath at 50 digits
(a few hundred distinct values).  Where np.longdouble is not the x87 format (nmant != 63) everything is evaluated with mpmath
at 50 digits instead.  The products are taken in chunks of eight factors with one log per chunk — the same split as
csrc/device_math.h, so that the magnitude of every log the device takes is known for its bound — which also keeps every
product far inside the longdouble range.

Masked loci (mask[l] == 0) contribute nothing and are not counted in loci_used.  Quirk Q14: an entry with alt + ref == 0
is a used locus like any other (main.rs:556-575 adds its log-pmf and counts it; nothing there looks at the total): its
log-pmf is ln C(0, 0) + ln(1 / 1) = 0 and its expected term ln(pmf(0)^2) = 0, so it adds exactly 0.0 to both sums and 1 to
loci_used.  The oracle (oracle/cellector_oracle.c) does the same.

Accuracy of the reference itself (tests/test_tile_reference.py holds it to this against mpmath): a term is the sum of
ceil(n / 8) chunk logs and ln C.  A chunk ratio carries at most 3 * 8 + 1 roundings of 2^-64 relative, its log one more unit
of 2^-64 * max(1, |log|), and the additions one each: REF_OPS(n) * 2^-64 * max(1, |t|, largest partial) in all, with
REF_OPS(n) = 4 n + 3 ceil(n / 8) + 4; the conversion to double adds half an ulp of the double.
"""
import math

import numpy as np

LD = np.longdouble
HAVE_X87 = np.finfo(LD).nmant == 63
U53 = 2.0 ** -53  # unit roundoff of a double operation
DM_CHUNK = 8      # csrc/device_math.h: factors multiplied between logs

_LNC = {}    # (n, a) -> (hi, lo) doubles of ln C(n, a)
_BINOM = {}  # n -> longdouble array C(n, 0..n)


def _mp():
    import mpmath as mp
    mp.mp.dps = 50
    return mp


def _split(x):
    """an mpmath value as two doubles (hi + lo carries 106 bits)"""
    hi = float(x)
    return hi, float(x - hi)


def ln_choose_ld(n, a):
    """ln C(n, a) as a longdouble, from mpmath"""
    key = (int(n), int(a))
    if key not in _LNC:
        mp = _mp()
        _LNC[key] = _split(mp.log(mp.binomial(key[0], key[1])))
    hi, lo = _LNC[key]
    return LD(hi) + LD(lo)


def _binom_ld(n):
    if n not in _BINOM:
        mp = _mp()
        out = np.empty(n + 1, LD)
        for k in range(n + 1):
            hi, lo = _split(mp.binomial(n, k))
            out[k] = LD(hi) + LD(lo)
        _BINOM[n] = out
    return _BINOM[n]


def ref_ops(n):
    """roundings of 2^-64 in the longdouble evaluation of a term (module docstring)"""
    n = np.asarray(n, np.int64)
    return 4 * n + 3 * ((n + DM_CHUNK - 1) // DM_CHUNK) + 4


def term_mp(alpha, beta, a, r):
    """one term with mpmath at 50 digits, product form (the fallback of term_values, and its own cross-check)"""
    mp = _mp()
    al, be = mp.mpf(float(alpha)), mp.mpf(float(beta))
    num, den = mp.mpf(1), mp.mpf(1)
    for i in range(int(a)):
        num *= al + i
    for j in range(int(r)):
        num *= be + j
    for k in range(int(a + r)):
        den *= al + be + k
    return mp.log(mp.binomial(int(a + r), int(a))) + mp.log(num / den)


def expected_mp(alpha, beta, n):
    mp = _mp()
    al, be = mp.mpf(float(alpha)), mp.mpf(float(beta))
    s = mp.mpf(0)
    for k in range(int(n) + 1):
        s += mp.exp(term_mp(al, be, k, int(n) - k)) ** 2
    return mp.log(s)


def term_values(alpha, beta, alt, ref):
    """Per-key log-pmf: arrays (t longdouble, log_ulps double, partial double).

    log_ulps = sum over the ceil(n / 8) logs of the device's evaluation of one double ulp at that log's magnitude;
    partial = the largest |partial sum| met on the way (for the reference's own error bound)."""
    alpha = np.asarray(alpha, np.float64)
    beta = np.asarray(beta, np.float64)
    a = np.asarray(alt, np.int64)
    r = np.asarray(ref, np.int64)
    n = a + r
    K = len(n)
    if not HAVE_X87:
        t = np.array([LD(float(term_mp(alpha[i], beta[i], a[i], r[i]))) for i in range(K)], LD)
    al, be = alpha.astype(LD), beta.astype(LD)
    ab = al + be
    acc = np.zeros(K, LD)
    log_ulps = np.zeros(K, np.float64)
    partial = np.zeros(K, np.float64)
    num, den = np.ones(K, LD), np.ones(K, LD)
    nmax = int(n.max()) if K else 0
    for k in range(nmax):
        live = k < n
        f = np.where(k < a, al + LD(k), be + (LD(k) - a.astype(LD)))
        num = np.where(live, num * f, num)
        den = np.where(live, den * (ab + LD(k)), den)
        # the device takes a log when a chunk of eight factors is full and more follow, and one at the end
        close = live & (((k + 1) % DM_CHUNK == 0) | (k + 1 == n))
        if close.any():
            lr = np.log(np.where(close, num / den, LD(1)))
            acc = acc + lr
            log_ulps += np.where(close, np.spacing(np.abs(lr).astype(np.float64)), 0.0)
            partial = np.maximum(partial, np.abs(acc).astype(np.float64))
            num = np.where(close, LD(1), num)
            den = np.where(close, LD(1), den)
    # (n == 0: the device returns 0 + log(1 / 1) = 0: one log of magnitude 0; n a multiple of 8 takes no extra log)
    lnc = np.zeros(K, LD)
    for key in set(zip(n.tolist(), a.tolist())):
        if key[0] >= 2:
            lnc[(n == key[0]) & (a == key[1])] = ln_choose_ld(*key)
    partial = np.maximum(partial, np.abs(lnc).astype(np.float64))
    if HAVE_X87:
        t = lnc + acc
    return t, log_ulps, partial


def expected_values(alpha, beta, n):
    """Per-key expected term ln sum_k pmf(k)^2 (longdouble), from the same products."""
    alpha = np.asarray(alpha, np.float64)
    beta = np.asarray(beta, np.float64)
    n = np.asarray(n, np.int64)
    out = np.zeros(len(n), LD)
    if not HAVE_X87:
        return np.array([LD(float(expected_mp(alpha[i], beta[i], n[i]))) for i in range(len(n))], LD)
    for nn in np.unique(n):
        nn = int(nn)
        sel = np.nonzero(n == nn)[0]
        al, be = alpha[sel].astype(LD), beta[sel].astype(LD)
        # A[k] = prod_{i<k}(alpha+i), B[j] = prod_{j'<j}(beta+j'), D = prod_{k<n}(alpha+beta+k): products of at most 240 factors
        # of at most 2e9 stay below 1e2300, far inside the longdouble range (1e4932)
        A = np.ones((nn + 1, len(sel)), LD)
        B = np.ones((nn + 1, len(sel)), LD)
        D = np.ones(len(sel), LD)
        for k in range(nn):
            A[k + 1] = A[k] * (al + LD(k))
            B[k + 1] = B[k] * (be + LD(k))
            D = D * (al + be + LD(k))
        C = _binom_ld(nn)
        s = np.zeros(len(sel), LD)
        for k in range(nn + 1):
            p = C[k] * A[k] * B[nn - k] / D
            s = s + p * p
        out[sel] = np.log(s)
    return out


# ---- the device's bound (csrc/device_math.h; derivation: tests/test_gpu_tile_sweep.py) ---------------------------------------
_DK = [2.48574089138753565546e-5, 1.05142378581721974210, -3.45687097222016235469, 4.51227709466894823700,
       -2.98285225323576655721, 1.05639711577126713077, -1.95428773191645869583e-1, 1.70970543404441224307e-2,
       -5.71926117404305781283e-4, 4.63399473359905636708e-6, -2.71994908488607703910e-9]


def lanczos_bound(x):
    """Absolute error of dm_ln_gamma(x + 1) against ln(x!), x > 170, from its operations:
    s = dk0 + sum dk_i / (X + i - 1), X = x + 1 an integer (the denominators are exact): a division and an addition of half an
    ulp each per term, both at most of the size T = sum |dk_i / (X + i - 1)| -> 11 u T on s, i.e. 11 u T / s on log(s) (the
    alternating terms cancel: T / s is ~1e3 here, the whole of this bound), plus one ulp of log(s);
    (X - 0.5) * log((X - 0.5 + g) / e): the addition, the division and the rounded constant e give 1.5 u relative on the
    argument, the log one ulp of its value, all times (X - 0.5); half an ulp for the product and for each of the two additions;
    the series itself: below 1e-15 relative on Gamma (Pugh, "An Analysis of the Lanczos Gamma Approximation", 2004, the
    n = 10, g = 10.900511 row statrs took its coefficients from), i.e. 1e-15 absolute on the logarithm."""
    X = float(x) + 1.0
    terms = [_DK[i] / (X + i - 1.0) for i in range(1, 11)]
    s = _DK[0] + sum(terms)
    T = sum(abs(v) for v in terms)
    lg = math.log((X - 0.5 + 10.900511) / math.e)
    res = math.lgamma(X)
    return (11 * U53 * T / s + np.spacing(abs(math.log(s))) + (X - 0.5) * (1.5 * U53 + np.spacing(lg))
            + 0.5 * np.spacing((X - 0.5) * lg) + np.spacing(res) + 1e-15)


def ln_choose_bound(n, a):
    """ln C(n, a) = lf(n) - lf(a) - lf(n - a) on the device: half an ulp of ln(n!) for each of the three values taken from the
    ln-factorial table (x <= 170; 0! and 1! are exact), the Lanczos bound for a value beyond the table."""
    n, a = int(n), int(a)
    if n < 2:
        return 0.0
    ulp_n = float(np.spacing(math.lgamma(n + 1.0)))
    out = 0.0
    for x in (n, a, n - a):
        out += lanczos_bound(x) if x > 170 else 0.5 * ulp_n
    return out


def term_bound(n, a, log_ulps):
    """B_term: (2 n + 2 + ceil(n / 8)) roundings of 2^-53 relative on the ratio(s), i.e. absolute on their logs; one ulp of
    each log result; the ln C part."""
    n = np.asarray(n, np.int64)
    a = np.asarray(a, np.int64)
    lnc = np.zeros(len(n), np.float64)
    for key in set(zip(n.tolist(), a.tolist())):
        lnc[(n == key[0]) & (a == key[1])] = ln_choose_bound(*key)
    return (2 * n + 2 + (n + DM_CHUNK - 1) // DM_CHUNK) * U53 + np.asarray(log_ulps, np.float64) + lnc


OV_NE = 17  # csrc/kernels_tiled.hip: the ratio recurrence serves the expected terms up to this total


def expected_bound(alpha, beta, n, e):
    """Bound of the device's expected term against ln sum pmf(k)^2 (u = 2^-53, the largest relative error of one rounded operation).

    n <= 17, the ratio recurrence (dm_expected_log_pmf for the tile tables, ov_expected_rec for the other totals, which multiplies
    by a reciprocal good to an ulp, 2 u, instead of dividing): pmf(0) is n factors of two additions, a reciprocal and two products,
    6 n u; a step of the recurrence two additions, three products and a reciprocal, 8 u, at most n of them; a square doubles the
    relative error and rounds once; the sum of the n + 1 positive squares rounds n times: 2 (6 n + 8 n) + 1 + n = 29 n + 1
    roundings relative on the sum, i.e. absolute on its log, plus one ulp of the log.
    n > 17, the recurrence anchored at the mode k* (ov_expected_mode), ln(sum_k (pmf(k) / pmf(k*))^2) + 2 ln pmf(k*): at most n steps of
    8 u, squared and summed as above, (17 n + 1) u and one ulp of a log of at most ln(n + 1); twice the B_term of ln pmf(k*) (the
    largest over k is taken: k* is the device's rounding); half an ulp of the result for the last addition."""
    alpha = np.asarray(alpha, np.float64)
    beta = np.asarray(beta, np.float64)
    n = np.asarray(n, np.int64)
    e = np.abs(np.asarray(e, np.float64))
    out = (29 * n + 1) * U53 + np.spacing(e)
    for nn in np.unique(n[n > OV_NE]):
        nn = int(nn)
        sel = np.nonzero(n == nn)[0]
        ks = np.tile(np.arange(nn + 1), len(sel))  # every k of every key of this total, in one vectorised call
        _, lu, _ = term_values(np.repeat(alpha[sel], nn + 1), np.repeat(beta[sel], nn + 1), ks, nn - ks)
        bt = term_bound(np.full(len(ks), nn), ks, lu).reshape(len(sel), nn + 1).max(axis=1)
        out[sel] = (17 * nn + 1) * U53 + np.spacing(math.log(nn + 1.0)) + 2 * bt + 0.5 * np.spacing(e[sel])
    return out


def cell_reference(n_cells, locus, cell, alt, ref, alpha, beta, mask=None):
    """The cell pass over COO arrays (load order; a (locus, cell) pair listed twice is two entries).

    Returns a dict of per-cell arrays: ll, expected_ll (double, rounded from the longdouble sums), ll_ld (the longdouble sum of ll
    before it is rounded), loci_used, count (= loci_used as integers), abs_ll / abs_ell (sum of |term|), b_ll / b_ell (sum of the per-term device bounds), and the per-entry arrays
    term / eterm / bterm / ebterm (doubles, for probes) with `keep` (the entries at unmasked loci)."""
    locus = np.asarray(locus, np.int64)
    cell = np.asarray(cell, np.int64)
    alt = np.asarray(alt, np.int64)
    ref = np.asarray(ref, np.int64)
    alpha = np.asarray(alpha, np.float64)
    beta = np.asarray(beta, np.float64)
    keep = np.ones(len(locus), bool) if mask is None else np.asarray(mask)[locus] != 0
    lo, ce, al, re = locus[keep], cell[keep], alt[keep], ref[keep]
    assert (al < 65536).all() and (re < 65536).all()
    key = (lo << 32) | (al << 16) | re
    uk, inv = np.unique(key, return_inverse=True)
    kl, ka, kr = uk >> 32, (uk >> 16) & 0xFFFF, uk & 0xFFFF
    t, log_ulps, _ = term_values(alpha[kl], beta[kl], ka, kr)
    bt = term_bound(ka + kr, ka, log_ulps)
    # expected terms: distinct (locus, n)
    nkey = (kl << 32) | (ka + kr)
    un, ninv = np.unique(nkey, return_inverse=True)
    el, en = un >> 32, un & 0xFFFFFFFF
    e = expected_values(alpha[el], beta[el], en)
    be = expected_bound(alpha[el], beta[el], en, e)
    e, be = e[ninv], be[ninv]

    order = np.argsort(ce, kind="stable")
    cnt = np.bincount(ce, minlength=n_cells)
    starts = np.concatenate([[0], np.cumsum(cnt)[:-1]])

    def per_cell(v):
        v = v[inv][order]
        out = np.zeros(n_cells, v.dtype)
        nz = cnt > 0
        if len(v):
            out[nz] = np.add.reduceat(v, starts[nz])
        return out

    ll_ld = per_cell(t)
    return dict(
        ll=ll_ld.astype(np.float64), ll_ld=ll_ld, expected_ll=per_cell(e).astype(np.float64),
        loci_used=cnt.astype(np.float64), count=cnt,
        abs_ll=per_cell(np.abs(t)).astype(np.float64), abs_ell=per_cell(np.abs(e)).astype(np.float64),
        b_ll=per_cell(bt), b_ell=per_cell(be),
        keep=keep, term=t[inv].astype(np.float64), eterm=e[inv].astype(np.float64), bterm=bt[inv], ebterm=be[inv])


def cell_bound(ref, n_partials):
    """Per-cell bound of the device's sums: sum of the per-term bounds + (m + G) 2^-53 sum |term| for the m additions inside the
    partial sums and the G partial sums added at the end."""
    m = ref["count"].astype(np.float64)
    return (ref["b_ll"] + (m + n_partials) * U53 * ref["abs_ll"], ref["b_ell"] + (m + n_partials) * U53 * ref["abs_ell"])
