"""80-bit reference of the donor calls (cellector_donor_tables / cellector_donor_posteriors / cellector_match_donors;
csrc/kernels_donors.hip), the device's error bounds, and the cases the CPU and the GPU tests share.

A plain helper for the tests (no fixtures, no GPU), independent of cellector_amd/donors.py: it shares no code with the twin.  The model
is stated once more here, in np.longdouble (u64 = 2^-64): theta from the loci's totals, the two tables, the singlet and pair sums with
np.add.reduceat over the COO sorted by cell, one softmax over the 2 D - 1 hypotheses.

Bounds (u = 2^-53; nothing here is fitted to observed errors).  n = the entries of the cell at used, unmasked loci.

  tab    theta is a chain of IEEE operations on doubles (whole-number totals, the two parameters): the device's theta IS the double
         theta formed here in double, so tab = log(double theta) and log(double (1.0 - theta)) are held to C_LOG u |log| = one ulp of log
         as a relative error (ROCm device-libs documents 1 ulp for the f64 log; cluster_reference's tab bound).
  s, p   the sums of doubles (the tables the device returned): B = (n + 1) u sum (|alt la| + |ref lb|), as cluster_reference's B_s.
  x      = (s + lp) + log_singlet: B_x = B_s + u |s + lp| + u |x|;  y = p + log_pair: B_y = B_p + u |y|.
  w      d_k = t_k - m rounds once and carries the errors of both operands: e_k = B_t[k] + max_j B_t[j] + u |d_k|; exp is good to an ulp:
         rel_k = expm1(e_k) + C_EXP u.  den adds 2 D terms in order (the anchor's pair column is an exact 0): rel_den = max_k rel_k +
         2 D u.  The division rounds once: rel(w_k) = (1 + rel_k) (1 + u) / (1 - rel_den) - 1.
  dp     the sum of the D pair posteriors in order: B_dp = sum_d rel(w_d) w_d + D u dp.
  match  ll_kd: B = (n_l + 1) u sum (|a la| + |r lb|) over the n_l unmasked loci; the tallies are whole numbers below 2^53.

The reference repeats the operations at 2^-64: every bound is widened by posterior_reference.REF_SHARE of itself for it, and a
comparison adds half an ulp of the double the reference is rounded to where it is compared as one.

Decisions (best, second, best_pair, status) are compared where the reference decides them by more than the bounds.  Two donors with
the same genotypes at every entry of a cell (and the same prior) have the same bits on every side, whatever the rounding: such a tie
is structural, it is broken by the smaller index here and on the device, and it does not count as undecided.
"""
import math

import numpy as np

import posterior_reference as pr
import tile_reference as tr

LD = np.longdouble
U = tr.U53
C_EXP = pr.C_EXP
C_LOG = 2.0
NONE = 255
DEFAULTS = dict(err=0.01, ambient=0.03, doublet_rate=0.1, posterior_threshold=0.999, min_loci=1)
F = 1.0 + pr.REF_SHARE


def params(**kw):
    p = dict(DEFAULTS)
    assert set(kw) <= set(p), kw
    p.update(kw)
    return p


# ---- tables ----------------------------------------------------------------------------------------------------------------------
def theta_double(A, R, err, ambient):
    """theta [L, 4] in double, operation by operation as the header states it"""
    A, R = np.asarray(A, np.float64), np.asarray(R, np.float64)
    soup = (A + 1.0) / ((A + R) + 2.0)
    out = np.empty((len(A), 4))
    for g, e in enumerate((err, 0.5, 1.0 - err, None)):
        out[:, g] = ((1.0 - ambient) * (soup if e is None else e)) + (ambient * soup)
    return out


def tab_reference(A, R, err=0.01, ambient=0.03, mask=None):
    """(tab1 [L, 4, 2], tab2 [L, 16, 2]) in longdouble from the double thetas, and their bounds"""
    th = theta_double(A, R, err, ambient)
    th2 = np.empty((len(th), 16))
    for a in range(4):
        for b in range(4):
            th2[:, 4 * a + b] = 0.5 * (th[:, a] + th[:, b])
    out = []
    for t in (th, th2):
        tab = np.stack([np.log(t.astype(LD)), np.log((1.0 - t).astype(LD))], axis=-1)
        if mask is not None:
            tab[np.asarray(mask) == 0] = 0
        out.append(tab)
    return out[0], out[1], [C_LOG * U * np.abs(t).astype(np.float64) * F for t in out]


def _ratio(got, want, bound):
    d = np.abs(np.asarray(got, np.float64).astype(LD) - want).astype(np.float64)
    bound = bound + np.where(bound > 0, 0.5 * np.spacing(np.abs(want.astype(np.float64))), 0.0)
    return float(np.where(bound > 0, d / np.where(bound > 0, bound, 1.0), np.where(d == 0, 0.0, np.inf)).max(initial=0.0))


def compare_tabs(A, R, err, ambient, mask, tab1, tab2):
    w1, w2, (b1, b2) = tab_reference(A, R, err, ambient, mask)
    return dict(tab1=_ratio(tab1, w1, b1), tab2=_ratio(tab2, w2, b2))


def pack_reference(gt_used):
    """packed [L, W] from gt_used [D, L], bit by bit"""
    D, L = gt_used.shape
    out = [[0] * ((D + 31) // 32) for _ in range(L)]
    for d in range(D):
        for l in range(L):
            out[l][d >> 5] |= int(gt_used[d, l]) << (2 * (d & 31))
    return np.array(out, np.uint64).reshape(L, (D + 31) // 32)


# ---- the cell calls --------------------------------------------------------------------------------------------------------------
def _rows(coo, mask):
    """the entries at unmasked loci in by-cell CSR order (a stable sort by locus, then a stable sort by cell)"""
    lo, ce, al, re = (np.asarray(x, np.int64) for x in coo)
    if mask is not None:
        keep = np.asarray(mask)[lo] != 0
        lo, ce, al, re = lo[keep], ce[keep], al[keep], re[keep]
    o = np.argsort(lo, kind="stable")
    o = o[np.argsort(ce[o], kind="stable")]
    return lo[o], ce[o], al[o], re[o]


def _seg_sum(ce, vals, n):
    out = np.zeros((n, vals.shape[1]), LD)
    cnt = np.bincount(ce, minlength=n)
    if len(ce):
        starts = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        nz = cnt > 0
        out[nz] = np.add.reduceat(vals, starts[nz], axis=0)
    return out, cnt


def _codes(ce, gl, n):
    """per (cell, donor) the sequence of the donor's genotypes at the cell's entries as one integer (rows of up to 32 entries; a
    longer row: a code no other donor has), for the structural ties"""
    D = gl.shape[1]
    cnt = np.bincount(ce, minlength=n)
    pos = np.arange(len(ce)) - np.repeat(np.concatenate([[0], np.cumsum(cnt)[:-1]]), cnt)
    code = np.zeros((n, D), np.uint64)
    ok = pos < 32
    np.add.at(code, ce[ok], gl[ok].astype(np.uint64) << (2 * pos[ok]).astype(np.uint64)[:, None])
    code[cnt > 32] = np.iinfo(np.uint64).max - np.arange(D, dtype=np.uint64)
    return code


def _decide(v, B, code, lp, exclude=None):
    """(idx, decided): per row the smallest column attaining the maximum of v (longdouble) over the columns != exclude, and whether
    every other column is a structural tie of it or further below than the two bounds together"""
    n, D = v.shape
    ok = np.ones((n, D), bool)
    if exclude is not None:
        ok[np.arange(n), exclude] = False
    w = np.where(ok, v, -np.inf)
    idx = np.argmax(ok & (w == w.max(axis=1)[:, None]), axis=1)
    r = np.arange(n)
    tie = (code == code[r, idx][:, None]) & (lp[None, :] == lp[idx][:, None])
    with np.errstate(invalid="ignore"):  # (-inf against -inf: no gap, not clear)
        gap = (w[r, idx][:, None] - w).astype(np.float64)
        clear = gap > (B + B[r, idx][:, None])
    tie |= np.isneginf(w.astype(np.float64)) & np.isneginf(w[r, idx].astype(np.float64))[:, None]  # (-inf is -inf on every side)
    return idx, (tie | clear | ~ok).all(axis=1)


def reference(L, N, coo, gt_used, tab1, tab2, log_prior=None, anchor=None, mask=None, **kw):
    """The donor posteriors of every cell in longdouble from DOUBLE tables (the device's, or the twin's), with the bounds of the
    module docstring.  anchor None = the reference's own best.  Returns a dict (values longdouble, bounds double)."""
    prm = params(**kw)
    g = np.asarray(gt_used, np.int64).T  # [L, D]
    D = g.shape[1]
    lo, ce, al, re = _rows(coo, mask)
    t1, t2 = np.asarray(tab1, np.float64).astype(LD), np.asarray(tab2, np.float64).astype(LD)
    gl = g[lo]
    alL, reL = al.astype(LD)[:, None], re.astype(LD)[:, None]

    def sums(t):
        pa, pb = alL * t[:, :, 0], reL * t[:, :, 1]
        s, cnt = _seg_sum(ce, pa + pb, N)
        mag, _ = _seg_sum(ce, np.abs(pa) + np.abs(pb), N)
        return s, (cnt[:, None] + 1.0) * U * mag.astype(np.float64), cnt

    s, B_s, cnt = sums(t1[lo[:, None], gl])
    lp = np.zeros(D) if log_prior is None else np.asarray(log_prior, np.float64)
    u = s + lp.astype(LD)[None, :]
    B_u = B_s + U * np.abs(np.where(np.isfinite(u), u, 0)).astype(np.float64)
    code = _codes(ce, gl, N)
    best, best_ok = _decide(u, B_u * F, code, lp)
    if D > 1:
        second, second_ok = _decide(u, B_u * F, code, lp, best)
    else:
        second, second_ok = np.full(N, NONE), np.ones(N, bool)
    second_ok &= best_ok
    a = best if anchor is None else np.asarray(anchor, np.int64)
    p, B_p, _ = sums(t2[lo[:, None], 4 * gl[np.arange(len(lo)), a[ce]][:, None] + gl])
    rate = float(prm["doublet_rate"])
    ls = math.log(1.0 - rate)
    lpair = (math.log(rate / float(D - 1)) if rate > 0 else -math.inf) if D > 1 else 0.0
    x = u + LD(ls)
    y = p + LD(lpair)
    y[np.arange(N), a] = -np.inf
    fin = lambda v: np.abs(np.where(np.isfinite(v), v, 0)).astype(np.float64)
    B_x, B_y = B_u + U * fin(x), B_p + U * fin(y)
    t = np.concatenate([x, y], axis=1)
    B_t = np.concatenate([B_x, B_y], axis=1)
    m = t.max(axis=1)
    d = t - m[:, None]
    ex = np.exp(d)
    den = ex.sum(axis=1)
    w = ex / den[:, None]
    e = B_t + np.where(np.isfinite(t), B_t, 0).max(axis=1)[:, None] + U * fin(d)
    rel_k = np.expm1(e) + C_EXP * U
    rel_den = np.where(np.isfinite(t.astype(np.float64)), rel_k, 0).max(axis=1) + 2 * D * U
    rel_w = ((1.0 + rel_k) * (1.0 + U) / (1.0 - rel_den[:, None]) - 1.0) * F
    post, ppost = w[:, :D], w[:, D:]
    dp = ppost.sum(axis=1)
    B_dp = ((rel_w[:, D:] * ppost.astype(np.float64)).sum(axis=1) + D * U * dp.astype(np.float64)) * F
    if D > 1:
        best_pair, pair_ok = _decide(y, B_y * F, code, np.zeros(D), a)
    else:
        best_pair, pair_ok = np.full(N, NONE), np.ones(N, bool)
    r = np.arange(N)
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


def _rel_ratio(got, want, rel):
    got = np.asarray(got, np.float64)
    seen = want >= pr.OBSERVABLE
    ratio = (np.abs(got.astype(LD) - want) / (rel * np.where(seen, want, LD(1)))).astype(np.float64)
    ratio = np.where(seen, ratio, np.where((got >= 0) & (got < pr.UNOBSERVED_BELOW), 0.0, np.inf))
    return float(np.where(np.isfinite(got), ratio, np.inf).max(initial=0.0))


def compare(ref, got):
    """got: the dict of Cellector.donor_posteriors (or the twin's).  Returns ({name: worst observed / bound}, undecided [cells] bool):
    sums and posteriors against their bounds; the decisions are compared on the decided cells (1.0 = a difference there)."""
    out = dict(ll=_ratio(got["ll"], ref["s"], ref["B_s"]), pair_ll=_ratio(got["pair_ll"], ref["p"], ref["B_p"]),
               posterior=_rel_ratio(got["posterior"], ref["posterior"], ref["rel_post"]),
               pair_posterior=_rel_ratio(got["pair_posterior"], ref["pair_posterior"], ref["rel_pair"]),
               doublet_posterior=_ratio(got["doublet_posterior"], ref["doublet_posterior"], ref["B_dp"]))
    undecided = np.zeros(len(ref["best"]), bool)
    for name, okname in (("best", "best_ok"), ("second", "second_ok"), ("best_pair", "pair_ok"), ("status", "status_ok")):
        dec = ref[okname]
        undecided |= ~dec
        out[name] = 0.0 if np.array_equal(np.asarray(got[name])[dec], ref[name][dec]) else np.inf
    out["n_entries"] = 0.0 if np.array_equal(np.asarray(got["n_entries"]).astype(np.int64), ref["n_entries"]) else np.inf
    return out, undecided


def match_reference(alt, ref, tab1, gt_used, mask=None):
    """(ll [K, D] longdouble, bound) from the class tallies alt, ref [K, L] and DOUBLE tables"""
    g = np.asarray(gt_used, np.int64).T
    t = np.asarray(tab1, np.float64).astype(LD)[np.arange(g.shape[0])[:, None], g]  # [L, D, 2]
    use = np.ones(g.shape[0], bool) if mask is None else np.asarray(mask) != 0
    a, r = np.asarray(alt).astype(LD)[:, use, None], np.asarray(ref).astype(LD)[:, use, None]
    t = t[use]
    pa, pb = a * t[None, :, :, 0], r * t[None, :, :, 1]
    ll = (pa + pb).sum(axis=1)
    B = (use.sum() + 1.0) * U * (np.abs(pa) + np.abs(pb)).sum(axis=1).astype(np.float64) * F
    return ll, B


# ---- the cases -------------------------------------------------------------------------------------------------------------------
DONORS = (1, 2, 3, 5, 9, 16, 31, 32, 33, 64)  # every lane width 2 ... 64
CASE_L, CASE_N = 487, 677  # neither a multiple of 64; 677 is odd: no multiple of any rows-per-wave
_case = {}


def case_matrix():
    """(L, N, coo) in file order: rows of 0, 1 ... 9 distinct loci (cell c: c % 10, around the prefetch depth of 4), every 50th cell
    with one of its pairs twice more under other counts, every locus with at least one entry, counts 0 .. 40 with zeros on either
    side"""
    if "m" not in _case:
        rng = np.random.default_rng(23)
        lo, ce = [], []
        for c in range(CASE_N):
            k = c % 10
            l = rng.choice(CASE_L, k, replace=False)
            lo.append(l); ce.append(np.full(k, c))
            if k and c % 50 == 1:
                lo.append(np.repeat(l[:1], 2)); ce.append(np.full(2, c))
        lo.append(np.arange(CASE_L)); ce.append(1 + 10 * (np.arange(CASE_L) % 60) + 8)  # (cells with 9 entries take the cover: up to 18)
        lo, ce = np.concatenate(lo), np.concatenate(ce)
        tot = rng.geometric(0.35, len(lo))
        al = rng.binomial(tot, rng.choice([0.03, 0.5, 0.97], len(lo)))
        re = tot - al
        al[:4], re[:4] = [0, 40, 0, 7], [0, 0, 40, 0]
        order = rng.permutation(len(lo))
        order = order[np.argsort(lo[order], kind="stable")]
        _case["m"] = (CASE_L, CASE_N, [np.asarray(x, np.int64)[order] for x in (lo, ce, al, re)])
    return _case["m"]


def case_gt(D, L=CASE_L, seed=3):
    """gt [D, L]: calls 0 / 1 / 2 with 10 % blanked to 3; locus 5 without any call; with D >= 3 donor 1 without any call"""
    rng = np.random.default_rng(seed + 7 * D)
    gt = rng.choice(3, (D, L), p=[0.45, 0.3, 0.25]).astype(np.uint8)
    gt[rng.random((D, L)) < 0.1] = 3
    gt[:, 5] = 3
    if D >= 3:
        gt[1] = 3
    return gt


def case_mask(L=CASE_L):
    return (np.random.default_rng(911 + L).random(L) < 0.8).astype(np.uint8)


def case_prior(D):
    """a prior that is not flat, with one donor ruled out (D >= 2)"""
    lp = np.log(np.random.default_rng(17 + D).dirichlet(np.ones(D) * 3.0))
    if D >= 2:
        lp[D // 2] = -np.inf
    return lp


def totals(L, coo):
    lo, _, al, re = coo
    return np.bincount(lo, weights=al, minlength=L), np.bincount(lo, weights=re, minlength=L)


# ---- the planted pool ------------------------------------------------------------------------------------------------------------
def planted_pool(seed=5):
    """The refine mixture with its 60 planted cross-genotype doublets (class_doublet_reference.doublet_mixture at rate 0), the three
    genotypes called from the planted classes by cellector_amd.genotypes as the donors, a decoy donor of random calls behind them,
    10 % of all calls blanked.  Returns (L, N, coo, gt [4, L], truth [N] (255: a doublet), parents [60, 2])."""
    if ("pool", seed) not in _case:
        import class_doublet_reference as cdr
        from cellector_amd import genotypes as gtw
        L, N, coo, truth, par = cdr.doublet_mixture(0.0, seed)
        _, alt, ref = gtw.class_genotype_tallies(L, coo, truth, 3)
        called, _, _ = gtw.genotype_posteriors(alt, ref)
        gt = np.array([3, 2, 1, 0], np.uint8)[called]  # (genotypes: 1 = 1/1, 2 = 0/1, 3 = 0/0, 0 = ./.)
        rng = np.random.default_rng(seed + 41)
        gt = np.concatenate([gt, rng.choice(3, (1, L)).astype(np.uint8)])
        gt[rng.random(gt.shape) < 0.1] = 3
        _case[("pool", seed)] = (L, N, coo, gt, truth, par)
    return _case[("pool", seed)]
