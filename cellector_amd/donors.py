"""Donor demultiplexing on host arrays: the numpy twin of cellector_donor_tables / cellector_donor_posteriors /
cellector_match_donors (include/cellector_ffi.h states the model; csrc/kernels_donors.hip runs it), and the reader of the donors'
genotypes from a VCF.

Every cell, and every class of a labelling, is scored against D donors whose genotypes are known: per locus four binomial allele
fractions (hom-ref, het, hom-alt, no call) under an ambient mix, a singlet sum per (cell, donor), a pair sum per (cell, anchor
donor, donor), one softmax over the 2 D - 1 hypotheses.

The sums are the library's sums in the library's order (a cell's entries in by-cell CSR row order, a class' loci in ascending
order, one rounded product and one rounded add at a time): fed the DEVICE's tables, singlet_sums, pair_sums and match_sums carry the
device's bits.  log and exp are numpy's, not the device's: the tables made here and the posteriors agree with the device's to a few
ulps.

The same calls from genotype probabilities (cellector_donor_weights / cellector_donor_posteriors_gp / cellector_match_donors_gp):
soft_weights, soft_singlet_sums, soft_pair_sums, soft_match_sums, posteriors_gp, match_gp, and read_donor_vcf_gp for the GP, GL or PL
of a donor VCF.

Donor panels (cellector_donor_panel / cellector_match_donors_panel; csrc/kernels_donor_panel.hip), up to 4096 donors with the pairs
of a cell's anchor and a shortlist of its best singlets: panel_shortlist, panel_posteriors, panel_present, panel_match.  The shortlist,
best, second and the sums are the device's exactly when fed the device's tables.

The fit of the called hypothesis (cellector_donor_moment_tables / cellector_donor_fit): moment_tables, fit_sums, fit_calls, fit.  The
four moment sums carry the device's bits when fed the device's tables; z passes through a sqrt and a division and agrees to 2 ulp;
the hypothesis, the keys, their statistics and the flags follow exactly from the numbers they are given.
"""
import math
import re

import numpy as np

from . import combine
from .cluster import Matrix  # noqa: F401  (the matrix in the library's row order; callers build one and pass it in)

NO_CALL = 3
NONE = 255
SINGLET, DOUBLET, AMBIGUOUS, UNASSIGNED = 0, 1, 2, 255
STATUS_NAMES = {SINGLET: "singlet", DOUBLET: "doublet", AMBIGUOUS: "ambiguous", UNASSIGNED: "unassigned"}
DEFAULTS = dict(err=0.01, ambient=0.03, doublet_rate=0.1, posterior_threshold=0.999, min_loci=1)


def _params(params):
    p = dict(DEFAULTS)
    for k, v in params.items():
        if k not in p:
            raise TypeError(f"unknown parameter {k!r}")
        p[k] = v
    return p


# ---- packing and tables ----------------------------------------------------------------------------------------------------------
def pack(gt, locus_ids):
    """packed [L, W] uint64, W = ceil(D / 32): donor d of used locus l at bits 2 (d & 31) of word d >> 5, from gt [D, total_loci]"""
    gt = np.asarray(gt, np.uint8)
    D = gt.shape[0]
    g = gt[:, np.asarray(locus_ids, np.int64)].astype(np.uint64)  # [D, L]
    out = np.zeros((g.shape[1], (D + 31) // 32), np.uint64)
    for d in range(D):
        out[:, d >> 5] |= g[d] << np.uint64(2 * (d & 31))
    return out


def unpack(packed, D):
    """g [L, D] uint8 from packed [L, W]"""
    packed = np.asarray(packed, np.uint64)
    return np.stack([(packed[:, d >> 5] >> np.uint64(2 * (d & 31))) & np.uint64(3) for d in range(D)], axis=1).astype(np.uint8)


def thetas(alt_total, ref_total, err=0.01, ambient=0.03):
    """theta [L, 4]: ((1 - ambient) e_g) + (ambient soup), e = (err, 0.5, 1 - err, soup), soup = (A + 1) / ((A + R) + 2)"""
    A, R = np.asarray(alt_total, np.float64), np.asarray(ref_total, np.float64)
    soup = (A + 1.0) / ((A + R) + 2.0)
    keep, amb = 1.0 - ambient, ambient * soup
    e = np.stack([np.full_like(soup, err), np.full_like(soup, 0.5), np.full_like(soup, 1.0 - err), soup], axis=1)
    return keep * e + amb[:, None]


def tables(alt_total, ref_total, err=0.01, ambient=0.03, mask=None, log=np.log):
    """(tab1 [L, 4, 2], tab2 [L, 16, 2]) = (log theta, log(1 - theta)); tab2 at 4 g_a + g_b from 0.5 (theta_a + theta_b); a masked
    locus carries (0, 0)"""
    th = thetas(alt_total, ref_total, err, ambient)
    th2 = (0.5 * (th[:, :, None] + th[:, None, :])).reshape(len(th), 16)
    tab1 = np.stack([log(th), log(1.0 - th)], axis=-1)
    tab2 = np.stack([log(th2), log(1.0 - th2)], axis=-1)
    if mask is not None:
        tab1[np.asarray(mask) == 0] = 0.0
        tab2[np.asarray(mask) == 0] = 0.0
    return tab1, tab2


# ---- the ordered sums ------------------------------------------------------------------------------------------------------------
def singlet_sums(mat, tab1, g):
    """s [cells, D]: per (cell, donor) the sum over the cell's entries in row order of ((alt la) + (ref lb)), (la, lb) =
    tab1[l][g[l, d]]; mat: a cluster.Matrix over the used loci (built with the call's mask), g [L, D] the donors' genotypes there"""
    tab1, g = np.asarray(tab1, np.float64), np.asarray(g, np.int64)
    s = np.zeros((mat.N, g.shape[1]))
    for rows, ent in mat.rows.steps:
        l = mat.r_lo[ent]
        t = tab1[l[:, None], g[l]]  # [m, D, 2]
        s[rows] = s[rows] + ((mat.r_al[ent, None] * t[:, :, 0]) + (mat.r_re[ent, None] * t[:, :, 1]))
    return s


def pair_sums(mat, tab2, g, anchor):
    """p [cells, D]: the same sum with tab2[l][4 g[l, anchor_c] + g[l, d]]"""
    tab2, g, anchor = np.asarray(tab2, np.float64), np.asarray(g, np.int64), np.asarray(anchor, np.int64)
    p = np.zeros((mat.N, g.shape[1]))
    for rows, ent in mat.rows.steps:
        l = mat.r_lo[ent]
        t = tab2[l[:, None], 4 * g[l, anchor[rows]][:, None] + g[l]]
        p[rows] = p[rows] + ((mat.r_al[ent, None] * t[:, :, 0]) + (mat.r_re[ent, None] * t[:, :, 1]))
    return p


def match_sums(alt, ref, tab1, g, mask=None):
    """ll [K, D]: per (class, donor) the sum over ascending unmasked loci of ((a la) + (r lb)) from the class tallies alt, ref [K, L]"""
    alt, ref = np.asarray(alt).astype(np.float64), np.asarray(ref).astype(np.float64)
    tab1, g = np.asarray(tab1, np.float64), np.asarray(g, np.int64)
    K, L = alt.shape
    ll = np.zeros((K, g.shape[1]))
    for l in range(L):
        if mask is not None and not mask[l]:
            continue
        t = tab1[l, g[l]]  # [D, 2]
        ll = ll + ((alt[:, l, None] * t[None, :, 0]) + (ref[:, l, None] * t[None, :, 1]))
    return ll


def _argmax_first(v, exclude=None):
    """per row the smallest column that attains the maximum over the columns other than exclude[row]"""
    v = np.asarray(v, np.float64)
    if exclude is None:
        return np.argmax(v, axis=1)
    ok = np.arange(v.shape[1])[None, :] != np.asarray(exclude, np.int64)[:, None]
    w = np.where(ok, v, -np.inf)
    return np.argmax(ok & (w == w.max(axis=1)[:, None]), axis=1)


# ---- the chain -------------------------------------------------------------------------------------------------------------------
def best_second(s, log_prior=None):
    """(best, second) uint8 of u = s + log_prior: the smallest d on ties; second = 255 with one donor"""
    n, D = s.shape
    u = s + (np.zeros(D) if log_prior is None else np.asarray(log_prior, np.float64))[None, :]
    best = _argmax_first(u)
    second = _argmax_first(u, best).astype(np.uint8) if D > 1 else np.full(n, NONE, np.uint8)
    return best.astype(np.uint8), second


def chain(s, p, anchor, entries, log_prior=None, **params):
    """dict of posterior, pair_posterior [cells, D], doublet_posterior, best, second, best_pair, status from the sums: the softmax
    over the D singlets x = (s + log_prior) + log_singlet and the D - 1 pairs y = p + log_pair (d != anchor), in that order"""
    prm = _params(params)
    n, D = s.shape
    anchor = np.asarray(anchor, np.int64)
    lp = np.zeros(D) if log_prior is None else np.asarray(log_prior, np.float64)
    rate = float(prm["doublet_rate"])
    with np.errstate(divide="ignore"):
        log_singlet = math.log(1.0 - rate)
        log_pair = (math.log(rate / float(D - 1)) if rate > 0 else -math.inf) if D > 1 else 0.0
    x = (s + lp[None, :]) + log_singlet
    y = p + log_pair
    y[np.arange(n), anchor] = -np.inf
    m = np.maximum(x.max(axis=1), y.max(axis=1))
    ex, ey = np.exp(x - m[:, None]), np.exp(y - m[:, None])
    den = np.zeros(n)
    for d in range(D):
        den = den + ex[:, d]
    for d in range(D):
        den = den + ey[:, d]
    post, ppost = ex / den[:, None], ey / den[:, None]
    dp = np.zeros(n)
    for d in range(D):
        dp = dp + ppost[:, d]
    best, second = best_second(s, log_prior)
    best_pair = _argmax_first(y, anchor).astype(np.uint8) if D > 1 else np.full(n, NONE, np.uint8)
    pb = post[np.arange(n), best]
    status = np.where(np.asarray(entries) < int(prm["min_loci"]), UNASSIGNED,
                      np.where(dp > 0.5, DOUBLET, np.where(pb >= float(prm["posterior_threshold"]), SINGLET, AMBIGUOUS))).astype(np.uint8)
    return dict(posterior=post, pair_posterior=ppost, doublet_posterior=dp, best=best, second=second, best_pair=best_pair, status=status,
                x=x, y=y)


def posteriors(mat, gt_used, alt_total, ref_total, log_prior=None, anchor=None, tab1=None, tab2=None, **params):
    """cellector_donor_posteriors on host arrays.  mat: a cluster.Matrix over the used loci, built with the call's mask; gt_used
    [D, L] the donors' genotypes at the used loci; alt_total, ref_total [L] the loci's totals (Cellector.locus_counts).  tab1 / tab2:
    the device's tables, for the device's bits in ll and pair_ll; None = numpy's.  Returns the dict of Cellector.donor_posteriors
    (summary: a dict)."""
    prm = _params(params)
    g = np.asarray(gt_used, np.uint8).T
    if tab1 is None or tab2 is None:
        tab1, tab2 = tables(alt_total, ref_total, prm["err"], prm["ambient"], mat.mask)
    s = singlet_sums(mat, tab1, g)
    best, _ = best_second(s, log_prior)
    anchor = best if anchor is None else np.asarray(anchor, np.uint8)
    p = pair_sums(mat, tab2, g, anchor)
    out = chain(s, p, anchor, mat.entries, log_prior, **prm)
    st = out["status"]
    out.update(ll=s, pair_ll=p, anchor=anchor, n_entries=mat.entries.astype(np.uint32), tab1=tab1, tab2=tab2,
               summary=dict(n_singlet=int((st == SINGLET).sum()), n_doublet=int((st == DOUBLET).sum()),
                            n_ambiguous=int((st == AMBIGUOUS).sum()), n_unassigned=int((st == UNASSIGNED).sum()),
                            donor_cells=np.bincount(out["best"][st == SINGLET], minlength=g.shape[1])))
    return out


def match(alt, ref, cells, gt_used, alt_total, ref_total, mask=None, tab1=None, **params):
    """cellector_match_donors on host arrays from the class tallies alt, ref [K, L] and cells [K]: dict of ll [K, D], best, margin"""
    prm = _params(params)
    g = np.asarray(gt_used, np.uint8).T
    if tab1 is None:
        tab1 = tables(alt_total, ref_total, prm["err"], prm["ambient"], mask)[0]
    return _match_calls(match_sums(alt, ref, tab1, g, mask), cells)


def _match_calls(ll, cells):
    K, D = ll.shape
    best = np.argmax(ll, axis=1)
    if D > 1:
        rest = ll.copy()
        rest[np.arange(K), best] = -np.inf
        margin = ll[np.arange(K), best] - rest.max(axis=1)
    else:
        margin = np.full(K, np.inf)
    live = np.asarray(cells) > 0
    return dict(ll=ll, best=np.where(live, best, NONE).astype(np.uint8), margin=np.where(live, margin, 0.0))


# ---- donor panels ------------------------------------------------------------------------------------------------------------------
# The twin of cellector_donor_panel / cellector_match_donors_panel (csrc/kernels_donor_panel.hip): up to 4096 donors, one softmax over
# the D singlets and the pairs of the anchor with a shortlist of the cell's M best singlets.  Donor indices are uint16, 65535 = none.
PANEL_NONE = 65535
PANEL_MAX_DONORS = 4096


def panel_shortlist(u, M):
    """cand [cells, M] uint16: per cell the first M donors in (u descending, d ascending), listed in ascending d; a function of the
    bits of u alone (a stable sort: equal values, -inf among them, keep their index order)"""
    u = np.asarray(u, np.float64)
    M = min(int(M), u.shape[1])
    first = np.argsort(-u, axis=1, kind="stable")[:, :M]
    return np.sort(first, axis=1).astype(np.uint16)


def _panel_pair_sums(mat, tab2, g, anchor, cand):
    """p [cells, M]: pair_sums' sum for the donors cand [cells, M] of each cell alone"""
    tab2, g, anchor, cand = np.asarray(tab2, np.float64), np.asarray(g, np.int64), np.asarray(anchor, np.int64), np.asarray(cand, np.int64)
    p = np.zeros((mat.N, cand.shape[1]))
    for rows, ent in mat.rows.steps:
        l = mat.r_lo[ent]
        t = tab2[l[:, None], 4 * g[l, anchor[rows]][:, None] + g[l[:, None], cand[rows]]]
        p[rows] = p[rows] + ((mat.r_al[ent, None] * t[:, :, 0]) + (mat.r_re[ent, None] * t[:, :, 1]))
    return p


def panel_posteriors(mat, gt_used, alt_total, ref_total, shortlist=8, log_prior=None, anchor=None, tab1=None, tab2=None, s=None, **params):
    """cellector_donor_panel on host arrays.  mat: a cluster.Matrix over the used loci, built with the call's mask; gt_used [D, L] the
    donors' genotypes at the used loci; tab1 / tab2: the device's tables, for the device's bits in ll, cand_ll and cand_pair_ll; None =
    numpy's.  s: singlet_sums(mat, tab1, gt_used.T) where the caller has them already (they depend on neither the shortlist nor the
    anchor).  Returns the dict of Cellector.donor_panel with ll (summary: a dict).  The chain adds its D + M terms one at a time, in
    the model's order."""
    prm = _params(params)
    g = np.asarray(gt_used, np.uint8).T
    n, D = mat.N, g.shape[1]
    if not 1 <= D <= PANEL_MAX_DONORS:
        raise ValueError(f"{D} donors, 1..{PANEL_MAX_DONORS} are supported")
    if not 1 <= int(shortlist) <= 64:
        raise ValueError(f"a shortlist of {shortlist}, 1..64 are supported")
    M = min(int(shortlist), D)
    if tab1 is None or tab2 is None:
        tab1, tab2 = tables(alt_total, ref_total, prm["err"], prm["ambient"], mat.mask)
    lp = np.zeros(D) if log_prior is None else np.asarray(log_prior, np.float64)
    r = np.arange(n)
    s = singlet_sums(mat, tab1, g) if s is None else np.asarray(s, np.float64)
    u = s + lp[None, :]
    best = _argmax_first(u)
    second = _argmax_first(u, best).astype(np.uint16) if D > 1 else np.full(n, PANEL_NONE, np.uint16)
    cand = panel_shortlist(u, M)
    ci = cand.astype(np.int64)
    a = best.astype(np.int64) if anchor is None else np.asarray(anchor, np.int64)
    p = _panel_pair_sums(mat, tab2, g, a, ci)
    rate = float(prm["doublet_rate"])
    with np.errstate(divide="ignore"):
        log_singlet = math.log(1.0 - rate)
        log_pair = (math.log(rate / float(D - 1)) if rate > 0 else -math.inf) if D > 1 else 0.0
    x = u + log_singlet
    pair_ok = ci != a[:, None]
    y = np.where(pair_ok, p + log_pair, -np.inf)
    m = np.maximum(x.max(axis=1), y.max(axis=1))
    ex, ey = np.exp(x - m[:, None]), np.exp(y - m[:, None])
    den = np.zeros(n)
    for d in range(D):
        den = den + ex[:, d]
    for j in range(M):
        den = den + ey[:, j]
    post, ppost = ex[r[:, None], ci] / den[:, None], ey / den[:, None]
    dp = np.zeros(n)
    for j in range(M):
        dp = dp + ppost[:, j]
    top = np.where(pair_ok, y, -np.inf).max(axis=1)
    j_pair = np.argmax(pair_ok & (y == top[:, None]), axis=1)
    best_pair = np.where(pair_ok.any(axis=1), ci[r, j_pair], PANEL_NONE).astype(np.uint16)
    pb = ex[r, best] / den
    entries = np.asarray(mat.entries)
    status = np.where(entries < int(prm["min_loci"]), UNASSIGNED,
                      np.where(dp > 0.5, DOUBLET, np.where(pb >= float(prm["posterior_threshold"]), SINGLET, AMBIGUOUS))).astype(np.uint8)
    cells = np.bincount(best[status == SINGLET], minlength=D).astype(np.uint64)
    return dict(cand=cand, cand_ll=s[r[:, None], ci], cand_pair_ll=p, cand_posterior=post, cand_pair_posterior=ppost, doublet_posterior=dp,
                best_posterior=pb, best=best.astype(np.uint16), second=second, best_pair=best_pair, anchor=a.astype(np.uint16),
                n_entries=entries.astype(np.uint32), status=status, donor_cells=cells, ll=s, tab1=tab1, tab2=tab2, x=x, y=y,
                summary=dict(n_singlet=int((status == SINGLET).sum()), n_doublet=int((status == DOUBLET).sum()),
                             n_ambiguous=int((status == AMBIGUOUS).sum()), n_unassigned=int((status == UNASSIGNED).sum()),
                             n_present=int((cells > 0).sum())))


def panel_present(result, min_cells=1):
    """the ascending indices of the donors with at least min_cells status-0 cells in the dict of donor_panel / panel_posteriors: the
    donors the 64-donor calls (donor_fit, estimate_ambient, ...) are then run on, as gt[panel_present(result)]"""
    return np.flatnonzero(np.asarray(result["donor_cells"]) >= max(int(min_cells), 1))


def panel_match(alt, ref, cells, gt_used, alt_total, ref_total, mask=None, tab1=None, **params):
    """cellector_match_donors_panel on host arrays: match() with best as uint16, 65535 for a class without a cell"""
    out = match(alt, ref, cells, gt_used, alt_total, ref_total, mask, tab1, **params)
    out["best"] = np.where(np.asarray(cells) > 0, np.argmax(out["ll"], axis=1), PANEL_NONE).astype(np.uint16)
    return out


# ---- the fit of the called hypothesis ----------------------------------------------------------------------------------------------
# The twin of cellector_donor_moment_tables / cellector_donor_fit: how well the hypothesis the donor call chose explains the cell.  An
# entry's term under Binomial(n, theta) has mean n h and variance n v, (h, v) a constant of (locus, genotype); the sums of both in the
# library's order carry the device's bits when fed the device's tables.
FIT_DEFAULTS = dict(iqr_multiple=3.0, min_cells=8)


def moment_tables(alt_total, ref_total, err=0.01, ambient=0.03, mask=None, log=np.log):
    """(mom1 [L, 4, 2], mom2 [L, 16, 2]) = (h, v): h = (th log th) + (rest log rest), v = (th rest) (d d), d = log th - log rest, rest =
    1 - th, th the theta of tables(); a masked locus carries (0, 0)"""
    th = thetas(alt_total, ref_total, err, ambient)
    th2 = (0.5 * (th[:, :, None] + th[:, None, :])).reshape(len(th), 16)
    out = []
    for t in (th, th2):
        rest = 1.0 - t
        la, lb = log(t), log(rest)
        d = la - lb
        mom = np.stack([(t * la) + (rest * lb), (t * rest) * (d * d)], axis=-1)
        if mask is not None:
            mom[np.asarray(mask) == 0] = 0.0
        out.append(mom)
    return out[0], out[1]


def fit_sums(mat, mom1, mom2, g, anchor):
    """(E, V, PE, PV) [cells, D]: per (cell, donor) the sums over the cell's entries in row order of n h and n v, n = alt + ref, (h, v)
    = mom1[l][g[l, d]], and of the same from mom2[l][4 g[l, anchor_c] + g[l, d]]"""
    mom1, mom2, g = np.asarray(mom1, np.float64), np.asarray(mom2, np.float64), np.asarray(g, np.int64)
    anchor = np.asarray(anchor, np.int64)
    E, V, PE, PV = (np.zeros((mat.N, g.shape[1])) for _ in range(4))
    for rows, ent in mat.rows.steps:
        l = mat.r_lo[ent]
        n = (mat.r_al[ent] + mat.r_re[ent])[:, None]  # (whole numbers: exact)
        t1 = mom1[l[:, None], g[l]]
        t2 = mom2[l[:, None], 4 * g[l, anchor[rows]][:, None] + g[l]]
        E[rows] = E[rows] + (n * t1[:, :, 0])
        V[rows] = V[rows] + (n * t1[:, :, 1])
        PE[rows] = PE[rows] + (n * t2[:, :, 0])
        PV[rows] = PV[rows] + (n * t2[:, :, 1])
    return E, V, PE, PV


def order_statistics(keys, iqr_multiple):
    """(median, iqr, threshold) of the keys as cellector_order_statistics forms them (statrs' median and quartiles on exact order
    statistics, threshold = q1 - iqr_multiple iqr); at least 4 keys"""
    srt = np.sort(np.asarray(keys, np.float64))
    n = len(srt)
    k = n // 2
    med = srt[k] if n % 2 else (srt[k - 1] + srt[k]) / 2.0
    h1, h3 = (n + 1.0 / 3.0) * 0.25 + 1.0 / 3.0, (n + 1.0 / 3.0) * 0.75 + 1.0 / 3.0
    q1 = srt[int(h1) - 1] + (h1 - int(h1)) * (srt[int(h1)] - srt[int(h1) - 1])
    q3 = srt[int(h3) - 1] + (h3 - int(h3)) * (srt[int(h3)] - srt[int(h3) - 1])
    iqr = q3 - q1
    return float(med), float(iqr), float(q1 - iqr_multiple * iqr)


def fit_calls(s, p, E, V, PE, PV, anchor, best, best_pair, status, iqr_multiple=3.0, min_cells=8):
    """z, pair_z, the called hypothesis, its z, the keys' statistics and the flags from the sums and the donor call's decisions"""
    n, D = s.shape
    with np.errstate(invalid="ignore", divide="ignore"):
        z = np.where(V != 0.0, (s - E) / np.sqrt(V), 0.0)
        pz = np.where(PV != 0.0, (p - PE) / np.sqrt(PV), 0.0)
    r = np.arange(n)
    status, best, anchor = np.asarray(status), np.asarray(best, np.int64), np.asarray(anchor, np.int64)
    pair = status == DOUBLET
    bp = np.where(pair, np.asarray(best_pair, np.int64), 0)
    call_z = np.where(status == UNASSIGNED, 0.0, np.where(pair, pz[r, bp], z[r, best]))
    keys = call_z[status == SINGLET]
    med, iqr, thr = (math.nan, math.nan, -math.inf) if len(keys) < int(min_cells) else order_statistics(keys, float(iqr_multiple))
    unmatched = ((status != UNASSIGNED) & (call_z < thr)).astype(np.uint8)
    flagged = unmatched != 0
    return dict(z=z, pair_z=pz, call_z=call_z, hyp_a=np.where(pair, anchor, best).astype(np.uint8),
                hyp_b=np.where(pair, bp, NONE).astype(np.uint8), status=status.astype(np.uint8), unmatched=unmatched,
                summary=dict(n_keys=len(keys), median=med, iqr=iqr, threshold=thr, n_unmatched=int(flagged.sum()),
                             n_unmatched_singlet=int((flagged & (status == SINGLET)).sum()),
                             n_unmatched_doublet=int((flagged & pair).sum()),
                             n_unmatched_ambiguous=int((flagged & (status == AMBIGUOUS)).sum()),
                             donor_unmatched=np.bincount(best[flagged], minlength=D)))


def fit(mat, gt_used, alt_total, ref_total, log_prior=None, anchor=None, tab1=None, tab2=None, mom1=None, mom2=None, call=None,
        iqr_multiple=3.0, min_cells=8, **params):
    """cellector_donor_fit on host arrays: posteriors() (or call, a donor call's dict with ll, pair_ll, anchor, best, best_pair and
    status: the device's, for its bits) and the fit of the hypothesis it chose.  mom1 / mom2: the device's moment tables, or None =
    numpy's.  Returns the dict of Cellector.donor_fit (summary: a dict) with the donor call under "call"."""
    prm = _params(params)
    if call is None:
        call = posteriors(mat, gt_used, alt_total, ref_total, log_prior, anchor, tab1, tab2, **prm)
    if mom1 is None or mom2 is None:
        mom1, mom2 = moment_tables(alt_total, ref_total, prm["err"], prm["ambient"], mat.mask)
    E, V, PE, PV = fit_sums(mat, mom1, mom2, np.asarray(gt_used, np.uint8).T, call["anchor"])
    out = fit_calls(call["ll"], call["pair_ll"], E, V, PE, PV, call["anchor"], call["best"], call["best_pair"], call["status"],
                    iqr_multiple, min_cells)
    out.update(fit_e=E, fit_v=V, pair_e=PE, pair_v=PV, mom1=mom1, mom2=mom2, call=call)
    return out


# ---- genotype probabilities in place of hard calls ---------------------------------------------------------------------------------
# The twin of cellector_donor_weights / cellector_donor_posteriors_gp / cellector_match_donors_gp.  A donor's row at a locus is three
# weights; an entry's term is the mixture over the genotypes of positive weight, m + log(sum_g w_g exp(t_g - m)).  A one-hot row and a
# no-call take the hard call's lookup, as the device does.  exp and log are passed in, as tables() takes log.
SOFT = 4


def one_hot(gt):
    """gp [D, total_loci, 3] float32 from hard calls gt [D, total_loci]: weight 1 on the call, three NaN for a no-call"""
    gt = np.asarray(gt, np.uint8)
    gp = np.zeros(gt.shape + (3,), np.float32)
    for g in range(3):
        gp[..., g] = gt == g
    gp[gt == NO_CALL] = np.nan
    return gp


def hard_codes(gp):
    """gt [D, total_loci] uint8: the argmax of every row of gp, the smallest g on ties, 3 for a no-call (three NaN)"""
    gp = np.asarray(gp, np.float32)
    none = np.isnan(gp).all(axis=-1)
    return np.where(none, NO_CALL, np.argmax(np.where(none[..., None], 0.0, gp), axis=-1)).astype(np.uint8)


def soft_weights(gp, locus_ids):
    """(w [L, D, 3] float64, kind [L, D] uint8) over the used loci from gp [D, total_loci, 3]: w_g = gp_g / ((gp_0 + gp_1) + gp_2) in
    f64; kind 0, 1, 2 = a one-hot row of that genotype, 3 = a no-call (three NaN; w 0), 4 = a soft row.  Any other row is refused."""
    gp = np.asarray(gp, np.float32)
    x = gp[:, np.asarray(locus_ids, np.int64), :].astype(np.float64).transpose(1, 0, 2)
    none = np.isnan(x).all(axis=2)
    with np.errstate(invalid="ignore"):
        fine = np.isfinite(x).all(axis=2) & (x >= 0).all(axis=2) & (x > 0).any(axis=2)
    if not (none | fine).all():
        l, d = np.argwhere(~(none | fine))[0]
        raise ValueError(f"gp of donor {d} at locus {int(np.asarray(locus_ids)[l])} is {tuple(x[l, d])}: three NaN (no call), or three "
                         "finite weights >= 0 that are not all zero")
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.where(none[..., None], 0.0, x / ((x[..., 0] + x[..., 1]) + x[..., 2])[..., None])
        pos = x > 0
    kind = np.where(none, NO_CALL, np.where(pos.sum(axis=2) > 1, SOFT, np.argmax(pos, axis=2))).astype(np.uint8)
    return w, kind


def _mix(t, w, exp, log):
    """m + log(z) over the last axis: m = the maximum of t where w > 0, z = the sum in ascending order from 0.0 of w exp(t - m) there.
    A row without a positive weight gives nan: the callers select no such row."""
    P = w > 0
    m = np.where(P, t, -np.inf).max(axis=-1)
    z = np.zeros(m.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        for g in range(t.shape[-1]):
            e = exp(np.where(P[..., g], t[..., g] - m, 0.0))
            z = np.where(P[..., g], z + (w[..., g] * e), z)
        return m + log(z)


def _soft_singlet_terms(a, r, t1, w, kind, exp, log):
    """[m, D] terms from the counts a, r [m, 1], the loci's table rows t1 [m, 4, 2] and the donors' rows w [m, D, 3], kind [m, D]"""
    m = len(t1)
    hard = t1[np.arange(m)[:, None], np.minimum(kind, NO_CALL)]
    term = (a * hard[:, :, 0]) + (r * hard[:, :, 1])
    soft = kind == SOFT
    if soft.any():
        t = (a[:, :, None] * t1[:, None, :3, 0]) + (r[:, :, None] * t1[:, None, :3, 1])  # [m, 1, 3]
        term = np.where(soft, _mix(np.broadcast_to(t, w.shape), w, exp, log), term)
    return term


def soft_singlet_sums(mat, tab1, w, kind, exp=np.exp, log=np.log):
    """s [cells, D]: singlet_sums with the mixture term at the soft rows (w, kind: soft_weights' or the device's)"""
    tab1, w, kind = np.asarray(tab1, np.float64), np.asarray(w, np.float64), np.asarray(kind, np.int64)
    s = np.zeros((mat.N, kind.shape[1]))
    for rows, ent in mat.rows.steps:
        l = mat.r_lo[ent]
        s[rows] = s[rows] + _soft_singlet_terms(mat.r_al[ent, None], mat.r_re[ent, None], tab1[l], w[l], kind[l], exp, log)
    return s


def _four(w, kind):
    """[..., 4]: a row's weights over the four table rows; a one-hot row and a no-call are 1.0 on their own row"""
    out = np.zeros(kind.shape + (4,))
    out[..., :3] = np.where((kind == SOFT)[..., None], w, 0.0)
    for g in range(4):
        out[..., g] = np.where(kind == g, 1.0, out[..., g])
    return out


def soft_pair_sums(mat, tab2, w, kind, anchor, s, exp=np.exp, log=np.log):
    """p [cells, D]: pair_sums with the mixture over the anchor row's and the donor row's genotypes (g ascending, then h) wherever
    either is soft; column anchor_c is a copy of s[c, anchor_c]"""
    tab2, w, kind = np.asarray(tab2, np.float64), np.asarray(w, np.float64), np.asarray(kind, np.int64)
    anchor = np.asarray(anchor, np.int64)
    D = kind.shape[1]
    p = np.zeros((mat.N, D))
    for rows, ent in mat.rows.steps:
        l, a, r = mat.r_lo[ent], mat.r_al[ent, None], mat.r_re[ent, None]
        ka, kd = kind[l, anchor[rows]], kind[l]
        hard = tab2[l[:, None], 4 * np.minimum(ka, NO_CALL)[:, None] + np.minimum(kd, NO_CALL)]
        term = (a * hard[:, :, 0]) + (r * hard[:, :, 1])
        soft = (ka == SOFT)[:, None] | (kd == SOFT)
        if soft.any():
            wa, wd = _four(w[l, anchor[rows]], ka), _four(w[l], kd)
            ww = (wa[:, None, :, None] * wd[:, :, None, :]).reshape(len(l), D, 16)
            t2 = tab2[l]
            t = (a[:, :, None] * t2[:, None, :, 0]) + (r[:, :, None] * t2[:, None, :, 1])  # [m, 1, 16]
            term = np.where(soft, _mix(np.broadcast_to(t, ww.shape), ww, exp, log), term)
        p[rows] = p[rows] + term
    c = np.arange(mat.N)
    p[c, anchor] = np.asarray(s)[c, anchor]
    return p


def soft_match_sums(alt, ref, tab1, w, kind, mask=None, exp=np.exp, log=np.log):
    """ll [K, D]: match_sums with the mixture term at the soft rows"""
    alt, ref = np.asarray(alt).astype(np.float64), np.asarray(ref).astype(np.float64)
    tab1, w, kind = np.asarray(tab1, np.float64), np.asarray(w, np.float64), np.asarray(kind, np.int64)
    K, L = alt.shape
    D = kind.shape[1]
    ll = np.zeros((K, D))
    for l in range(L):
        if mask is not None and not mask[l]:
            continue
        rep = lambda x: np.broadcast_to(x[None], (K,) + x.shape)
        ll = ll + _soft_singlet_terms(alt[:, l, None], ref[:, l, None], rep(tab1[l]), rep(w[l]), rep(kind[l]), exp, log)
    return ll


def posteriors_gp(mat, w, kind, alt_total, ref_total, log_prior=None, anchor=None, tab1=None, tab2=None, exp=np.exp, log=np.log, **params):
    """cellector_donor_posteriors_gp on host arrays: posteriors() with (w [L, D, 3], kind [L, D]) = soft_weights(gp, locus_ids) in
    place of the hard calls.  tab1 / tab2: the device's tables, or None = numpy's."""
    prm = _params(params)
    if tab1 is None or tab2 is None:
        tab1, tab2 = tables(alt_total, ref_total, prm["err"], prm["ambient"], mat.mask, log=log)
    s = soft_singlet_sums(mat, tab1, w, kind, exp, log)
    best, _ = best_second(s, log_prior)
    anchor = best if anchor is None else np.asarray(anchor, np.uint8)
    p = soft_pair_sums(mat, tab2, w, kind, anchor, s, exp, log)
    out = chain(s, p, anchor, mat.entries, log_prior, **prm)
    st = out["status"]
    out.update(ll=s, pair_ll=p, anchor=anchor, n_entries=mat.entries.astype(np.uint32), tab1=tab1, tab2=tab2,
               summary=dict(n_singlet=int((st == SINGLET).sum()), n_doublet=int((st == DOUBLET).sum()),
                            n_ambiguous=int((st == AMBIGUOUS).sum()), n_unassigned=int((st == UNASSIGNED).sum()),
                            donor_cells=np.bincount(out["best"][st == SINGLET], minlength=kind.shape[1])))
    return out


def match_gp(alt, ref, cells, w, kind, alt_total, ref_total, mask=None, tab1=None, exp=np.exp, log=np.log, **params):
    """cellector_match_donors_gp on host arrays: match() with (w, kind) in place of the hard calls"""
    prm = _params(params)
    if tab1 is None:
        tab1 = tables(alt_total, ref_total, prm["err"], prm["ambient"], mask, log=log)[0]
    return _match_calls(soft_match_sums(alt, ref, tab1, w, kind, mask, exp, log), cells)


# ---- the donors' genotypes from a VCF ----------------------------------------------------------------------------------------------
def parse_gt(field, gt_index=0):
    """0, 1 or 2 = the number of alt alleles of a diploid biallelic GT ("0/1", "1|0", ...) in a sample field; 3 for anything else (a
    missing or half-missing call, a third allele, another ploidy, no GT at that index)"""
    parts = field.split(":")
    if gt_index < 0 or gt_index >= len(parts):
        return NO_CALL
    al = parts[gt_index].replace("|", "/").split("/")
    if len(al) != 2 or any(a not in ("0", "1") for a in al):
        return NO_CALL
    return int(al[0]) + int(al[1])


def _sample_names(path):
    import gzip
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "rt") as f:
        for line in f:
            if line.startswith("#CHROM"):
                return line.rstrip("\n").split("\t")[9:]
            if not line.startswith("#"):
                break
    raise ValueError(f"{path}: no #CHROM header line with sample columns")


def read_donor_vcf(donor_vcf, variant_vcf):
    """(names, gt): the donors' genotypes gt [D, total_loci] uint8 in the row order of the variant VCF the matrix was counted on.  A
    donor record is matched to the variant VCF's record with the same (chrom, pos, ref, alt); one whose ref and alt are swapped is
    matched too and its calls are mirrored (0/0 <-> 1/1).  A variant without a donor record, and an unparsable, missing or
    non-biallelic GT, is 3 (no call); when the donor VCF repeats a record the last one counts."""
    names = _sample_names(donor_vcf)
    rows = {}
    n = 0
    for chrom, pos, toks in combine._vcf_records(variant_vcf, columns=True):
        rows[(chrom, pos, toks[3], toks[4])] = n  # (a repeated variant: the last row takes the calls)
        n += 1
    gt = np.full((len(names), n), NO_CALL, np.uint8)
    for chrom, pos, toks in combine._vcf_records(donor_vcf, columns=True):
        if len(toks) < 10:
            continue
        at, swap = rows.get((chrom, pos, toks[3], toks[4])), False
        if at is None:
            at, swap = rows.get((chrom, pos, toks[4], toks[3])), True
        if at is None:
            continue
        fmt = toks[8].split(":")
        gi = fmt.index("GT") if "GT" in fmt else -1
        for d in range(len(names)):
            g = parse_gt(toks[9 + d], gi) if 9 + d < len(toks) else NO_CALL
            gt[d, at] = g if g == NO_CALL or not swap else 2 - g
    return names, gt


# ---- the donors' genotype probabilities from a VCF ---------------------------------------------------------------------------------

_NUMBER = re.compile(r"[+-]?([0-9]+\.?[0-9]*|\.[0-9]+)([eE][+-]?[0-9]+)?\Z")
FIELDS = ("GP", "GL", "PL")


def parse_weights(field, index, kind):
    """the three weights (floats, in double) of a sample field's GP, GL or PL at position index, or None: the field absent, '.', not
    three plain decimal numbers, a GP or PL below 0, a value that is not finite, or three zeros.  GP: as written.  GL: 10^(GL_g - max
    GL).  PL: 10^(-(PL_g - min PL) / 10)."""
    parts = field.split(":")
    if index < 0 or index >= len(parts):
        return None
    toks = parts[index].split(",")
    if len(toks) != 3 or not all(_NUMBER.match(t) for t in toks):
        return None
    v = [float(t) for t in toks]
    if not all(math.isfinite(x) for x in v) or (kind != "GL" and min(v) < 0):
        return None
    if kind == "GL":
        v = [10.0 ** (x - max(v)) for x in v]
    elif kind == "PL":
        v = [10.0 ** (-(x - min(v)) / 10.0) for x in v]
    return v if max(v) > 0 else None


def read_donor_vcf_gp(donor_vcf, variant_vcf, field="GP"):
    """(names, gp): the donors' genotype weights gp [D, total_loci, 3] float32 from the GP, GL or PL of a donor VCF, matched to the
    variant VCF as read_donor_vcf matches (a record whose ref and alt are swapped has its three values reversed).  A sample whose
    field parse_weights refuses falls back to the one-hot row of its GT if that parses, else to a no-call (three NaN); so does a
    variant without a donor record.  GL and PL are computed in double and stored as float."""
    if field not in FIELDS:
        raise ValueError(f"field: one of {FIELDS} expected, got {field!r}")
    names = _sample_names(donor_vcf)
    rows = {}
    n = 0
    for chrom, pos, toks in combine._vcf_records(variant_vcf, columns=True):
        rows[(chrom, pos, toks[3], toks[4])] = n
        n += 1
    gp = np.full((len(names), n, 3), np.nan, np.float32)
    for chrom, pos, toks in combine._vcf_records(donor_vcf, columns=True):
        if len(toks) < 10:
            continue
        at, swap = rows.get((chrom, pos, toks[3], toks[4])), False
        if at is None:
            at, swap = rows.get((chrom, pos, toks[4], toks[3])), True
        if at is None:
            continue
        fmt = toks[8].split(":")
        gi = fmt.index("GT") if "GT" in fmt else -1
        fi = fmt.index(field) if field in fmt else -1
        for d in range(len(names)):
            v = parse_weights(toks[9 + d], fi, field) if 9 + d < len(toks) else None
            if v is None:
                g = parse_gt(toks[9 + d], gi) if 9 + d < len(toks) else NO_CALL
                v = [math.nan] * 3 if g == NO_CALL else [float(g == k) for k in range(3)]
            gp[d, at] = v[::-1] if swap else v
    return names, gp
