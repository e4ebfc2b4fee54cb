"""High-precision reference of the per-entry records of cellector_cell_pmfs (PMFData, main.rs:527-539) and the device's bounds.

A plain helper for the tests (no fixtures, no GPU).  For an entry (alpha, beta, alt, ref), n = alt + ref:

    log_pmf               t = ln pmf(alt)                                     tile_reference.term_values
    expected_log_pmf      E = ln sum_{k=0..n} pmf(k)^2                        stats.rs:19-22
    expected_log_variance V = sum_{k=0..n} pmf(k) (ln pmf(k) - E)^2           stats.rs:23-28, centred on E (quirk Q7)

E and V are formed here from the n + 1 log-pmfs t_k themselves, as the reference does, in log space: exp(2 t_k) and exp(t_k) are
taken relative to the largest, so nothing underflows before it is negligible, and a pmf that is zero even so adds 0.  The t_k
come from tile_reference.term_values (80-bit products, exact ln C) for totals up to LD_MAX; beyond (the products of
tile_reference.expected_values leave the longdouble range, and term_values over all k is O(n^2)) from mpmath at 50 digits by
the log of the ratio recurrence, t_{k+1} = t_k + ln[(n-k)(alpha+k) / ((k+1)(beta+n-k-1))], anchored at t_0 by mpmath's loggamma.
moments_mp is the all-mpmath statement of the same three formulas that tests/test_pmf_reference.py holds this file to.

Accuracy of the reference itself (ref_error): t_k carries rt_k = REF_OPS(n) 2^-64 max(1, |t_k|, largest partial)
(tile_reference); with w_k = pmf(k)^2 / sum pmf^2 the expected term moves by at most 2 sum_k w_k rt_k, and V by
sum_k pmf(k) [rt_k d_k^2 + 2 |d_k| (rt_k + dE)], d_k = t_k - E, plus (n + 3) roundings of 2^-64 on each sum.

The device's bound for V (variance_bound; u = 2^-53; csrc/device_math.h dm_pmf_moments_small / dm_pmf_moments_wave), derived from
its operations the way tile_reference.expected_bound is, nothing fitted:

  n <= 17, the ratio recurrence from pmf(0), run a second time for V:
    pmf(k) as computed: 6 n u for pmf(0) and 8 u a step (expected_bound's count), delta = 14 n u relative at most;
    d_k = log(pmf(k)) - E: delta (a relative error of the argument is absolute on the log), one ulp of the log at |t_k|, the
      bound of E itself, B_E = (29 n + 1) u + ulp(E), and u |d_k| for the subtraction:   dd_k = delta + ulp(t_k) + B_E + u |d_k|;
    the term pmf(k) d_k^2: 2 |d_k| dd_k + dd_k^2 absolute on the square, then delta + 3 u relative (the pmf's own error, the square, the
      product, the addition); the n + 1 additions u V each.
  n > 17, all lanes of a wave, t_k = pmf(k) / pmf(k*) outwards from k* ~ the mode, V = exp(L) (c^2 + sum_k t_k (ln t_k - c)^2),
  L = ln pmf(k*) (dm_log_bb_pmf), c = ln(sum t^2) + L:
    t_k: 8 u a step, at most n steps, and at most 8 more products in the lanes' prefix product: delta = (8 n + 8) u;
    c: expected_bound's count for ln sum t^2, (17 n + 1) u + ulp(ln(n + 1)), the B_term of L (the largest over k: k* is the
      device's rounding) and half an ulp of c:                                            B_c;
    d_k = log(t_k) - c: dd_k = delta + ulp(ln t_k) + B_c + u |d_k|;
    the terms as above; exp(L): the absolute error of L is relative on its exponential, plus one ulp of exp (ROCm device-libs,
      ocml "exp: 1 ulp"), plus the last product; the additions, in the lanes and across them, at most n + 6 of u V each.
Plus half an ulp of the reference's own rounding to double.
"""
import functools
import math

import numpy as np

import tile_reference as tr

LD = np.longdouble
U53 = tr.U53
U64 = 2.0 ** -64
LD_MAX = 300   # totals whose n + 1 log-pmfs come from tile_reference.term_values
SMALL = 17     # csrc/device_math.h DM_MOM_SMALL


def _mp_to_ld(x):
    hi = float(x)
    return LD(hi) + LD(float(x - hi))


@functools.lru_cache(maxsize=8)
def log_pmfs_mp(alpha, beta, n):
    """ln pmf(0..n) with mpmath at 50 digits: loggamma at k = 0, then the log of the ratio recurrence (O(n)); kept per key"""
    mp = tr._mp()
    al, be, n = mp.mpf(float(alpha)), mp.mpf(float(beta)), int(n)
    t = mp.loggamma(be + n) + mp.loggamma(al + be) - mp.loggamma(be) - mp.loggamma(al + be + n)
    out = [t]
    for k in range(n):
        t = t + mp.log((n - k) * (al + k) / ((k + 1) * (be + (n - k - 1))))
        out.append(t)
    return out


def moments_mp(alpha, beta, n):
    """(E, V) straight from the definitions, all in mpmath, every log-pmf by tile_reference.term_mp (O(n^2): small totals)"""
    mp = tr._mp()
    t = [tr.term_mp(alpha, beta, k, int(n) - k) for k in range(int(n) + 1)]
    e = mp.log(sum(mp.exp(2 * x) for x in t))
    v = sum(mp.exp(x) * (x - e) ** 2 for x in t)
    return e, v


def term_bound_upper(alpha, beta, n):
    """An upper bound of tile_reference.term_bound(n, k, .) over every k, for a total whose n + 1 terms cannot all be evaluated:
    a chunk of eight factors is a product of ratios f / (alpha + beta + j) in [min(alpha, beta, 1) / (alpha + beta + n), 1], so each
    of the ceil(n / 8) logs is at most 8 ln((alpha + beta + n) / min(alpha, beta, 1)) in size; ln C takes three values, each at
    most the largest Lanczos bound (or half an ulp of ln n!) over 0..n."""
    n = int(n)
    chunks = (n + tr.DM_CHUNK - 1) // tr.DM_CHUNK
    big = 8.0 * math.log((alpha + beta + n) / min(alpha, beta, 1.0))
    lnc = 0.5 * float(np.spacing(math.lgamma(n + 1.0)))
    if n > 170:
        lnc = max(lnc, max(tr.lanczos_bound(x) for x in range(171, n + 1)))
    return (2 * n + 2 + chunks) * U53 + chunks * float(np.spacing(big)) + 3.0 * lnc


def _table(alpha, beta, nn):
    """the n + 1 log-pmfs of every key of total nn: t (K, nn + 1) longdouble, their reference error rt (double), and bt (K,), the
    largest device B_term over k"""
    K = len(alpha)
    if nn <= LD_MAX:
        ks = np.tile(np.arange(nn + 1), K)
        t, lu, partial = tr.term_values(np.repeat(alpha, nn + 1), np.repeat(beta, nn + 1), ks, nn - ks)
        bt = tr.term_bound(np.full(len(ks), nn), ks, lu).reshape(K, nn + 1).max(axis=1)
        rt = tr.ref_ops(nn) * U64 * np.maximum(1.0, np.maximum(np.abs(t).astype(np.float64), partial))
        return t.reshape(K, nn + 1), rt.reshape(K, nn + 1), bt
    t = np.array([[_mp_to_ld(x) for x in log_pmfs_mp(float(alpha[i]), float(beta[i]), nn)] for i in range(K)], LD)
    rt = 2.0 * U64 * np.maximum(1.0, np.abs(t).astype(np.float64))  # (50 digits: what is left is the conversion to longdouble)
    bt = np.array([term_bound_upper(alpha[i], beta[i], nn) for i in range(K)])
    return t, rt, bt


def _moments_from(t):
    m = t.max(axis=1, keepdims=True)
    e = (2 * m[:, 0]) + np.log(np.exp(2 * (t - m)).sum(axis=1))
    d = t - e[:, None]
    v = (np.exp(t) * d * d).sum(axis=1)
    return e, v, d


def variance_bound(nn, t, e, v, d, bt):
    """the device's bound for V (module docstring), per key of total nn"""
    tf, ef, vf, df = (np.asarray(x, np.float64) for x in (t, e, v, d))
    p = np.exp(tf)
    ad = np.abs(df)
    if nn <= SMALL:
        delta = 14 * nn * U53
        b_e = (29 * nn + 1) * U53 + np.spacing(np.abs(ef))
        dd = delta + np.spacing(np.abs(tf)) + b_e[:, None] + U53 * ad
        tail = (nn + 1) * U53 * vf
    else:
        delta = (8 * nn + 8) * U53
        tmax = tf.max(axis=1)
        b_c = (17 * nn + 1) * U53 + np.spacing(math.log(nn + 1.0)) + bt + 0.5 * np.spacing(np.abs(ef) + np.abs(tmax))
        dd = delta + np.spacing(np.abs(tf - tmax[:, None]) + 1.0) + b_c[:, None] + U53 * ad
        tail = vf * (bt + (nn + 6 + 3) * U53)
    return (p * (2 * ad * dd + dd * dd + df * df * (delta + 3 * U53))).sum(axis=1) + tail + 0.5 * np.spacing(np.abs(vf))


def ref_error(nn, t, rt, e, v, d):
    """what the reference's own E and V may be off by (module docstring): (dE, dV) per key, doubles"""
    tf, df = np.asarray(t, np.float64), np.abs(np.asarray(d, np.float64))
    w = np.exp(2 * (tf - np.asarray(e, np.float64)[:, None]))
    de = 2 * (w * rt).sum(axis=1) + (nn + 3) * U64 * np.maximum(1.0, np.abs(np.asarray(e, np.float64)))
    dv = (np.exp(tf) * (rt * df * df + 2 * df * (rt + de[:, None]))).sum(axis=1) + (nn + 3) * U64 * np.asarray(v, np.float64)
    return de, dv


def moments(alpha, beta, n):
    """Per key (alpha, beta, n): dict of arrays e, v (longdouble), v_bound (the device's bound for V), bt (largest B_term over k:
    expected_bound's ingredient), de, dv (the reference's own error)."""
    alpha = np.asarray(alpha, np.float64)
    beta = np.asarray(beta, np.float64)
    n = np.asarray(n, np.int64)
    K = len(n)
    out = dict(e=np.zeros(K, LD), v=np.zeros(K, LD), v_bound=np.zeros(K), bt=np.zeros(K), de=np.zeros(K), dv=np.zeros(K))
    for nn in np.unique(n):
        nn = int(nn)
        sel = np.nonzero(n == nn)[0]
        t, rt, bt = _table(alpha[sel], beta[sel], nn)
        e, v, d = _moments_from(t)
        out["e"][sel], out["v"][sel], out["bt"][sel] = e, v, bt
        out["v_bound"][sel] = variance_bound(nn, t, e, v, d, bt)
        out["de"][sel], out["dv"][sel] = ref_error(nn, t, rt, e, v, d)
    return out


def expected_bound(alpha, beta, n, e, bt):
    """tile_reference.expected_bound, with the largest B_term over k handed in (moments()'s bt): the same formula for every total, also
    where that maximum is term_bound_upper's."""
    n = np.asarray(n, np.int64)
    e = np.abs(np.asarray(e, np.float64))
    small = (29 * n + 1) * U53 + np.spacing(e)
    big = (17 * n + 1) * U53 + np.spacing(np.log(n + 1.0)) + 2 * np.asarray(bt) + 0.5 * np.spacing(e)
    return np.where(n > tr.OV_NE, big, small)


def records(alpha, beta, locus, alt, ref):
    """The three values and their device bounds for entries (locus, alt, ref) under per-locus alpha / beta: a dict of per-entry
    arrays log_pmf, expected, variance (doubles, rounded from the reference), b_log_pmf, b_expected, b_variance."""
    locus = np.asarray(locus, np.int64)
    a = np.asarray(alt, np.int64)
    r = np.asarray(ref, np.int64)
    alpha = np.asarray(alpha, np.float64)
    beta = np.asarray(beta, np.float64)
    key = (locus << 34) | (a << 17) | r
    uk, inv = np.unique(key, return_inverse=True)
    kl, ka, kr = uk >> 34, (uk >> 17) & 0x1FFFF, uk & 0x1FFFF
    t = np.zeros(len(uk), LD)
    bt = np.zeros(len(uk))
    cls = ka + kr <= LD_MAX
    if cls.any():
        tv, lu, _ = tr.term_values(alpha[kl[cls]], beta[kl[cls]], ka[cls], kr[cls])
        t[cls], bt[cls] = tv, tr.term_bound((ka + kr)[cls], ka[cls], lu)
    for i in np.nonzero(~cls)[0]:  # (term_values loops up to the largest total of its keys: these come from the mpmath table)
        al, be, nn = float(alpha[kl[i]]), float(beta[kl[i]]), int(ka[i] + kr[i])
        t[i], bt[i] = _mp_to_ld(log_pmfs_mp(al, be, nn)[int(ka[i])]), term_bound_upper(al, be, nn)
    nkey = (kl << 34) | (ka + kr)
    un, ninv = np.unique(nkey, return_inverse=True)
    m = moments(alpha[un >> 34], beta[un >> 34], un & 0x3FFFFFFFF)
    be = expected_bound(alpha[un >> 34], beta[un >> 34], un & 0x3FFFFFFFF, m["e"], m["bt"])
    e64, v64 = m["e"].astype(np.float64), m["v"].astype(np.float64)
    half = lambda x: 0.5 * np.spacing(np.abs(x))
    t64 = t.astype(np.float64)
    return dict(log_pmf=t64[inv], expected=e64[ninv][inv], variance=v64[ninv][inv],
                b_log_pmf=(bt + half(t64))[inv], b_expected=(be + half(e64))[ninv][inv], b_variance=m["v_bound"][ninv][inv])
