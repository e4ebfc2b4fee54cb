"""80-bit reference of the donor calls from genotype probabilities (cellector_donor_weights / cellector_donor_posteriors_gp /
cellector_match_donors_gp; csrc/kernels_donors.hip), the device's error bounds, and the cases the CPU and the GPU tests share.

A plain helper for the tests (no fixtures, no GPU), built on donor_reference (dr) and independent of cellector_amd/donors.py: it
shares no code with the twin.  The model of include/cellector_ffi.h is stated once more here in np.longdouble (2^-64).

The weights are IEEE operations on doubles made of floats (two adds, one division): the device's w IS the double formed here, and the
reference takes w and the tables as the doubles they are.

Bounds (u = 2^-53; nothing here is fitted to observed errors).  An entry's term under a row of kind < 4 is the hard call's:
two rounded products and their rounded sum, E = 2 u (|a la| + |r lb|).  Under a soft row with the set P of n_P genotypes (pairs: of
n_P products g, h) of positive weight:

  t_g    as the hard term: E_g = 2 u (|a la_g| + |r lb_g|).
  shift  m is the largest of the device's own t_g.  m + log(sum w_g exp(t_g - m)) is the same real number for EVERY shift m, so the
         device's choice of m carries no error of its own, whichever genotype it picks among near-equal ones.
  d_g    = t_g - m rounds once: the argument of exp is off by eta_g = E_g + u |d_g| (the error of t_g, and the rounding).
  z      exp is good to C_EXP u relative, w_g exp rounds once (pairs: w_g w_h rounds once more), and the n_P - 1 adds round once
         each (0.0 + x is exact); every term is positive, so the relative errors do not amplify:
         |log(z_dev) - log(z)| <= max_g eta_g - log1p(-(C_EXP + pw + n_P) u) + sub / z, pw = 1 for pairs and 0 for singlets.
         sub = 2 n_P 2^-1074: an exp or a product that underflows (t_g - m below -745: exp returns 0) is off by at most the smallest
         denormal, absolutely; z is at least the weight of the genotype at the maximum.
  log    C_LOG u |log z|, and m + log z rounds once: u |term|.
  term   B_t = max_g eta_g - log1p(-(C_EXP + pw + n_P) u) + sub / z + C_LOG u |log z| + u |term|.
  sum    n terms added in order: B = sum_i B_t[i] + n u sum_i |term_i|.

exp(eta) amplifies nothing further: eta enters log z at most once (a weighted mean of the eta_g, bounded by the largest).  The chain
behind the sums and its bounds are donor_reference's, operation for operation.  The reference repeats the operations at 2^-64:
every bound is widened by dr.F.
"""
import math

import numpy as np

import donor_reference as dr

LD = np.longdouble
U = dr.U
C_EXP, C_LOG = dr.C_EXP, dr.C_LOG
SOFT = 4
TINY = 2.0 ** -1074


# ---- weights -----------------------------------------------------------------------------------------------------------------------
def weights_reference(gp_used):
    """(w [L, D, 3] double, kind [L, D]) from gp_used [D, L, 3] float32, row by row"""
    D, L, _ = gp_used.shape
    w, kind = np.zeros((L, D, 3)), np.zeros((L, D), np.uint8)
    for d in range(D):
        for l in range(L):
            x = [float(v) for v in gp_used[d, l]]
            if all(math.isnan(v) for v in x):
                kind[l, d] = 3
                continue
            assert all(math.isfinite(v) and v >= 0 for v in x) and max(x) > 0, (d, l, x)
            tot = (x[0] + x[1]) + x[2]
            w[l, d] = [v / tot for v in x]
            pos = [g for g in range(3) if x[g] > 0]
            kind[l, d] = pos[0] if len(pos) == 1 else SOFT
    return w, kind


def hard_reference(gp):
    """the argmax of every row, the smallest g on ties, 3 for a no-call"""
    out = np.full(gp.shape[:-1], 3, np.uint8)
    for idx in np.ndindex(*gp.shape[:-1]):
        x = gp[idx]
        if not np.isnan(x).all():
            out[idx] = [g for g in range(3) if x[g] == x.max()][0]
    return out


# ---- terms -------------------------------------------------------------------------------------------------------------------------
def _terms(a, r, t, ww, soft, pw):
    """(term [m, D] longdouble, bound [m, D]) of m entries.  a, r [m] counts; t [m, G, 2] the locus' table rows (doubles); ww
    [m, D, G] the weights over those rows (a row of kind < 4: 1.0 on its own row); soft [m, D]: the mixture, else the lookup."""
    aL, rL = a.astype(LD)[:, None], r.astype(LD)[:, None]
    tL = t.astype(LD)
    pa, pb = aL * tL[:, :, 0], rL * tL[:, :, 1]  # [m, G]
    tg = (pa + pb)[:, None, :]                   # [m, 1, G]
    E = (2.0 * U * (np.abs(pa) + np.abs(pb)).astype(np.float64))[:, None, :]
    P = ww > 0
    n_P = P.sum(axis=2)
    m = np.where(P, tg, -np.inf).max(axis=2)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.where(P, tg - m[:, :, None], 0)
        z = np.where(P, ww.astype(LD) * np.exp(d), 0).sum(axis=2)
    lz = np.log(z)
    term = m + lz
    eta = np.where(P, E + U * np.abs(d).astype(np.float64), 0.0).max(axis=2)
    zf = z.astype(np.float64)
    B_soft = (eta - np.log1p(-(C_EXP + pw + n_P) * U) + 2.0 * n_P * TINY / np.where(zf > 0, zf, 1.0)
              + C_LOG * U * np.abs(lz).astype(np.float64) + U * np.abs(term).astype(np.float64))
    # the lookup: the one row of weight 1.0
    hard_t = np.where(P, tg, 0).sum(axis=2)
    hard_B = np.where(P, E, 0.0).sum(axis=2)
    return np.where(soft, term, hard_t), np.where(soft, B_soft, hard_B)


def _four(w, kind):
    out = np.zeros(kind.shape + (4,))
    for g in range(4):
        out[..., g] = np.where(kind == g, 1.0, np.where((kind == SOFT) & (g < 3), w[..., min(g, 2)], 0.0))
    return out


def _sum_terms(ce, term, B_t, N):
    s, cnt = dr._seg_sum(ce, term, N)
    mag, _ = dr._seg_sum(ce, np.abs(term), N)
    Bs, _ = dr._seg_sum(ce, B_t.astype(LD), N)
    return s, Bs.astype(np.float64) + cnt[:, None] * U * mag.astype(np.float64), cnt


def _same_rows(ce, lo, w, kind, N):
    """code [N, D]: the smallest donor whose rows (weights and kind) equal donor d's at every entry of the cell: equal codes are
    structural ties (the same bits on every side)"""
    D = kind.shape[1]
    wl, kl = w[lo], kind[lo]
    eq = (wl[:, :, None, :] == wl[:, None, :, :]).all(axis=3) & (kl[:, :, None] == kl[:, None, :])
    same = np.ones((N, D, D), bool)
    cnt = np.bincount(ce, minlength=N)
    if len(ce):
        starts = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        nz = cnt > 0
        same[nz] = np.logical_and.reduceat(eq, starts[nz], axis=0)
    return np.argmax(same, axis=2).astype(np.uint64)


def reference(L, N, coo, w, kind, tab1, tab2, log_prior=None, anchor=None, mask=None, **kw):
    """donor_reference.reference with the rows (w [L, D, 3], kind [L, D]) in place of the hard calls: the same dict"""
    prm = dr.params(**kw)
    w, kind = np.asarray(w, np.float64), np.asarray(kind, np.int64)
    D = kind.shape[1]
    lo, ce, al, re = dr._rows(coo, mask)
    t1, t2 = np.asarray(tab1, np.float64), np.asarray(tab2, np.float64)
    w4 = _four(w, kind)
    term, B_t = _terms(al, re, t1[lo], w4[lo], kind[lo] == SOFT, 0)
    s, B_s, cnt = _sum_terms(ce, term, B_t, N)
    lp = np.zeros(D) if log_prior is None else np.asarray(log_prior, np.float64)
    u = s + lp.astype(LD)[None, :]
    B_u = B_s + U * np.abs(np.where(np.isfinite(u), u, 0)).astype(np.float64)
    code = _same_rows(ce, lo, w, kind, N)
    F = dr.F
    best, best_ok = dr._decide(u, B_u * F, code, lp)
    if D > 1:
        second, second_ok = dr._decide(u, B_u * F, code, lp, best)
    else:
        second, second_ok = np.full(N, dr.NONE), np.ones(N, bool)
    second_ok &= best_ok
    a = best if anchor is None else np.asarray(anchor, np.int64)
    wa, ka = w4[lo, a[ce]], kind[lo, a[ce]]
    ww = (wa[:, None, :, None] * w4[lo][:, :, None, :]).reshape(len(lo), D, 16)
    term2, B_t2 = _terms(al, re, t2[lo], ww, (ka == SOFT)[:, None] | (kind[lo] == SOFT), 1)
    p, B_p, _ = _sum_terms(ce, term2, B_t2, N)
    r = np.arange(N)
    p[r, a], B_p[r, a] = s[r, a], B_s[r, a]
    # the chain: donor_reference.reference, operation for operation
    rate = float(prm["doublet_rate"])
    ls = math.log(1.0 - rate)
    lpair = (math.log(rate / float(D - 1)) if rate > 0 else -math.inf) if D > 1 else 0.0
    x = u + LD(ls)
    y = p + LD(lpair)
    y[r, a] = -np.inf
    fin = lambda v: np.abs(np.where(np.isfinite(v), v, 0)).astype(np.float64)
    B_x, B_y = B_u + U * fin(x), B_p + U * fin(y)
    t = np.concatenate([x, y], axis=1)
    B_c = np.concatenate([B_x, B_y], axis=1)
    m = t.max(axis=1)
    d = t - m[:, None]
    ex = np.exp(d)
    den = ex.sum(axis=1)
    wt = ex / den[:, None]
    err = B_c + np.where(np.isfinite(t), B_c, 0).max(axis=1)[:, None] + U * fin(d)
    rel_k = np.expm1(err) + C_EXP * U
    rel_den = np.where(np.isfinite(t.astype(np.float64)), rel_k, 0).max(axis=1) + 2 * D * U
    rel_w = ((1.0 + rel_k) * (1.0 + U) / (1.0 - rel_den[:, None]) - 1.0) * F
    post, ppost = wt[:, :D], wt[:, D:]
    dp = ppost.sum(axis=1)
    B_dp = ((rel_w[:, D:] * ppost.astype(np.float64)).sum(axis=1) + D * U * dp.astype(np.float64)) * F
    if D > 1:
        best_pair, pair_ok = dr._decide(y, B_y * F, code, np.zeros(D), a)
    else:
        best_pair, pair_ok = np.full(N, dr.NONE), np.ones(N, bool)
    pb = post[r, best]
    thr = float(prm["posterior_threshold"])
    status = np.where(cnt < int(prm["min_loci"]), 255, np.where(dp > 0.5, 1, np.where(pb >= thr, 0, 2)))
    dpf, pbf = dp.astype(np.float64), pb.astype(np.float64)
    off_half = np.abs(dpf - 0.5) > B_dp + np.spacing(0.5)
    off_thr = np.abs(pbf - thr) > rel_w[r, best] * pbf + np.spacing(thr)
    status_ok = (cnt < int(prm["min_loci"])) | (off_half & ((dpf > 0.5) | (off_thr & best_ok)))
    return dict(s=s, p=p, B_s=B_s * F, B_p=B_p * F, posterior=post, pair_posterior=ppost, rel_post=rel_w[:, :D], rel_pair=rel_w[:, D:],
                doublet_posterior=dp, B_dp=B_dp, best=best.astype(np.uint8), second=second.astype(np.uint8),
                best_pair=best_pair.astype(np.uint8), status=status.astype(np.uint8), anchor=a.astype(np.uint8), n_entries=cnt,
                best_ok=best_ok, second_ok=second_ok, pair_ok=pair_ok, status_ok=status_ok)


compare = dr.compare  # (the dicts have donor_reference's keys)
ratio = dr._ratio


def match_reference(alt, ref, tab1, w, kind, mask=None):
    """(ll [K, D] longdouble, bound) from the class tallies alt, ref [K, L] and DOUBLE tables"""
    w, kind = np.asarray(w, np.float64), np.asarray(kind, np.int64)
    K, L = np.asarray(alt).shape
    use = np.flatnonzero(np.ones(L, bool) if mask is None else np.asarray(mask) != 0)
    w4 = _four(w, kind)
    ll, B = np.zeros((K, kind.shape[1]), LD), np.zeros((K, kind.shape[1]))
    t1 = np.asarray(tab1, np.float64)
    for k in range(K):
        term, B_t = _terms(np.asarray(alt)[k, use], np.asarray(ref)[k, use], t1[use], w4[use], kind[use] == SOFT, 0)
        ll[k] = term.sum(axis=0)
        B[k] = B_t.sum(axis=0) + len(use) * U * np.abs(term).sum(axis=0).astype(np.float64)
    return ll, B * dr.F


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
PATTERNS = ("three", "zero0", "zero1", "zero2", "unnormalised", "1e-30", "denormal")
_case = {}


def _soft_row(rng, pattern):
    """one soft row (float32) of the named pattern"""
    x = rng.dirichlet(np.ones(3) * 2.0) * 0.98 + 0.006
    if pattern.startswith("zero"):
        x[int(pattern[4])] = 0.0
    elif pattern == "unnormalised":
        x = x / x.sum() * 2.5
    elif pattern == "1e-30":
        x[rng.integers(3)] = 1e-30
    elif pattern == "denormal":
        x[rng.integers(3)] = 1e-45  # (rounds to the smallest float denormal, 2^-149)
    return x.astype(np.float32)


def head_locus():
    """the locus of the entries (0, 40) and (40, 0) at the head of dr.case_matrix(): one locus, one cell"""
    L, N, (lo, ce, al, re) = dr.case_matrix()
    at = np.flatnonzero(((al == 40) & (re == 0)) | ((al == 0) & (re == 40)))
    assert len(at) == 2 and lo[at[0]] == lo[at[1]] and ce[at[0]] == ce[at[1]] and lo[at[0]] != 5, at
    return int(lo[at[0]]), int(ce[at[0]])


def hard_donor(d):
    """the donors whose every row is one-hot or a no-call: their columns carry the hard call's bits"""
    return d == 1 or d % 3 == 2


def case_gp(D, L=dr.CASE_L, seed=3):
    """gp [D, L, 3] float32 from dr.case_gt(D): its no-calls are kept (three NaN); about half of the called rows are the one-hot of the
    call, the others run through PATTERNS; the donors of hard_donor() are one-hot throughout.  With the case matrix' L the rows of the
    head locus (every donor but the hard ones; donor 0 even where case_gt has no call there) rule out the genotype that is largest
    at one of the two head entries: (0, 0.7, 0.3) for even d, where t_0 is largest at (alt 0, ref 40), and (0.6, 0.4, 0) for odd d,
    where t_2 is largest at (alt 40, ref 0)."""
    key = ("gp", D, L, seed)
    if key not in _case:
        gt = dr.case_gt(D, L, seed)
        rng = np.random.default_rng(1009 * seed + 31 * D + L)
        gp = np.zeros((D, L, 3), np.float32)
        for g in range(3):
            gp[..., g] = gt == g
        gp[gt == 3] = np.nan
        k = 0
        for d in range(D):
            if hard_donor(d):
                continue
            for l in np.flatnonzero((gt[d] < 3) & (rng.random(L) < 0.5)):
                gp[d, l] = _soft_row(rng, PATTERNS[k % len(PATTERNS)])
                k += 1
        if L == dr.CASE_L:
            l1, _ = head_locus()
            for d in range(D):
                if not hard_donor(d) and (gt[d, l1] < 3 or d == 0):
                    gp[d, l1] = (0.0, 0.7, 0.3) if d % 2 == 0 else (0.6, 0.4, 0.0)
        _case[key] = gp
    return _case[key]


DEEP_L, DEEP_N = 13, 37


def deep_matrix():
    """(L, N, coo): 37 cells x 13 loci, 1 .. 5 entries a cell, counts up to 2000 on one side and 0 .. 3 on the other: under a row
    that leaves two genotypes open t_g - m falls below -745 and exp returns 0"""
    if "deep" not in _case:
        rng = np.random.default_rng(77)
        lo, ce = [], []
        for c in range(DEEP_N):
            k = 1 + c % 5
            lo.append(rng.choice(DEEP_L, k, replace=False)); ce.append(np.full(k, c))
        lo.append(np.arange(DEEP_L)); ce.append(np.arange(DEEP_L) % DEEP_N)
        lo, ce = np.concatenate(lo), np.concatenate(ce)
        big, small = rng.integers(200, 2001, len(lo)), rng.integers(0, 4, len(lo))
        big[0] = 2000
        side = rng.random(len(lo)) < 0.5
        al, re = np.where(side, big, small), np.where(side, small, big)
        order = rng.permutation(len(lo))
        order = order[np.argsort(lo[order], kind="stable")]
        _case["deep"] = (DEEP_L, DEEP_N, [np.asarray(x, np.int64)[order] for x in (lo, ce, al, re)])
    return _case["deep"]


def deep_gp(D):
    return case_gp(D, DEEP_L, seed=11)


# ---- the planted pool with degraded calls ----------------------------------------------------------------------------------------------
def degraded_pool(seed):
    """dr.planted_pool(seed) with every called row degraded at probability 0.5 to (truth 0.35, one wrong genotype 0.60, the other
    0.05); the other called rows one-hot, the no-calls three NaN.  Returns (L, N, coo, gp [4, L, 3], truth).
    How many singlets the argmax calls get right depends on the draw far more than on the pool: over twelve draws of one pool it
    ran from 654 to 883 of 906 (the degraded loci are shared by all cells, so the cells' errors move together), while the mixture
    stayed at 901 .. 904.  The generator is fixed by rule, 1000 + the pool's seed."""
    L, N, coo, gt, truth, _ = dr.planted_pool(seed)
    rng = np.random.default_rng(1000 + seed)  # (two draws over the whole [4, L] array: which rows, and which wrong genotype)
    degrade = (gt < 3) & (rng.random(gt.shape) < 0.5)
    step = 1 + rng.integers(0, 2, gt.shape)
    gp = np.zeros(gt.shape + (3,), np.float32)
    for g in range(3):
        gp[..., g] = gt == g
    gp[gt == 3] = np.nan
    for d, l in np.argwhere(degrade):
        g = int(gt[d, l])
        row = np.full(3, 0.05, np.float32)
        row[g], row[(g + int(step[d, l])) % 3] = 0.35, 0.60
        gp[d, l] = row
    return L, N, coo, gp, truth
