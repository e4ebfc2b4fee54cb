"""80-bit reference of the donor panel (cellector_donor_panel; csrc/kernels_donor_panel.hip): steps 4b - 8 of the panel model on top
of donor_reference, whose statement of steps 1 - 4 (tables, rows, sums, structural ties) and whose constants it imports unchanged.

A plain helper for the tests (no fixtures, no GPU), independent of cellector_amd/donors.py.  The work is split where the tests share
it: singlets() holds everything that depends on the donors and the prior alone (s, u, best, second, the tie codes; formed in blocks of
donors, a panel of 4096 does not fit otherwise), chain() the shortlist, the pairs and the softmax for one (shortlist, anchor).

Bounds (u = 2^-53; nothing is fitted to observed errors): donor_reference's, operation for operation, with the chain's term count.
  s, p, x, y   as there: B = (n + 1) u sum (|alt la| + |ref lb|); B_x = B_s + u |s + lp| + u |x|; B_y = B_p + u |y|.
  w            d_k = t_k - m: e_k = B_t[k] + max_j B_t[j] + u |d_k|; rel_k = expm1(e_k) + C_EXP u.  den adds the D singlets and the M
               shortlist slots in order (the anchor's slot is an exact 0): D + M terms where the 64-donor chain has 2 D, so rel_den =
               max_k rel_k + (D + M) u.  rel(w_k) = (1 + rel_k) (1 + u) / (1 - rel_den) - 1.
  dp           the sum of the M pair posteriors in order: B_dp = sum_j rel(w_j) w_j + M u dp.
Every bound is widened by posterior_reference.REF_SHARE for the reference's own 2^-64 arithmetic, as there.

The shortlist (step 4b) is a decision: the reference lists its own first M donors by (u descending, d ascending) and says where that is
decided: the last donor taken and the first one left out are further apart than their bounds, or tie structurally (then the index
decides on every side).  The chain is evaluated on the shortlist it is GIVEN (the device's or the twin's), so that the posteriors are
compared over the same hypotheses; a cell whose shortlist is not decided counts as undecided.
"""
import math

import numpy as np

import donor_reference as dr

LD = np.longdouble
U = dr.U
F = dr.F
NONE = 65535
BLOCK = 256  # donors per block of the sums


def _classes(lo, al, re, tab2):
    """cls [nnz, 4]: per entry the smallest genotype value whose terms are the same operations on the same operands as g's, in the
    singlet sum and in the pair sum under any anchor: the same table rows bit for bit (the diagonal of tab2 is tab1), where a count of 0
    makes its product an exact 0 whatever the row holds.  Two donors whose classes agree at every entry of a cell carry the same bits on
    every side, as two donors with the same genotypes do: soup == 0.5 exactly (A == R) makes a het and a no-call such a pair."""
    t = np.asarray(tab2, np.float64)[lo].reshape(len(lo), 4, 4, 2).transpose(0, 2, 1, 3).copy()  # [nnz, g, ga, 2]
    t[al == 0, :, :, 0] = 0.0
    t[re == 0, :, :, 1] = 0.0
    key = t.reshape(len(lo), 4, 8).view(np.uint64)
    same = (key[:, :, None, :] == key[:, None, :, :]).all(axis=3)  # [nnz, g, g']
    return np.argmax(same, axis=2)


def singlets(L, N, coo, gt_used, tab1, log_prior=None, mask=None, tab2=None):
    """step 4 for all D donors in longdouble from the DOUBLE table: dict of s, B_s, u, B_u [N, D], best, second, best_ok, second_ok,
    code [N, D] (the structural ties; with tab2 over the classes of _classes, else over the genotypes), cnt [N] and what chain() needs
    of the rows"""
    g = np.asarray(gt_used, np.int64).T  # [L, D]
    D = g.shape[1]
    lo, ce, al, re = dr._rows(coo, mask)
    cls = None if tab2 is None else _classes(lo, al, re, tab2)
    t1 = np.asarray(tab1, np.float64).astype(LD)
    alL, reL = al.astype(LD)[:, None], re.astype(LD)[:, None]
    s, B_s, code = np.zeros((N, D), LD), np.zeros((N, D)), np.zeros((N, D), np.uint64)
    cnt = np.bincount(ce, minlength=N)
    for d0 in range(0, D, BLOCK):
        gl = g[lo, d0:d0 + BLOCK]
        t = t1[lo[:, None], gl]
        pa, pb = alL * t[:, :, 0], reL * t[:, :, 1]
        s[:, d0:d0 + BLOCK], _ = dr._seg_sum(ce, pa + pb, N)
        mag, _ = dr._seg_sum(ce, np.abs(pa) + np.abs(pb), N)
        B_s[:, d0:d0 + BLOCK] = (cnt[:, None] + 1.0) * U * mag.astype(np.float64)
        code[:, d0:d0 + BLOCK] = dr._codes(ce, gl if cls is None else cls[np.arange(len(lo))[:, None], gl], N)
    long_rows = cnt > 32  # (dr._codes gives such a row a code per donor of its block: make it one per donor of the panel)
    code[long_rows] = np.iinfo(np.uint64).max - np.arange(D, dtype=np.uint64)
    lp = np.zeros(D) if log_prior is None else np.asarray(log_prior, np.float64)
    u = s + lp.astype(LD)[None, :]
    B_u = B_s + U * np.abs(np.where(np.isfinite(u), u, 0)).astype(np.float64)
    best, best_ok = dr._decide(u, B_u * F, code, lp)
    if D > 1:
        second, second_ok = dr._decide(u, B_u * F, code, lp, best)
    else:
        second, second_ok = np.full(N, NONE), np.ones(N, bool)
    return dict(L=L, N=N, D=D, g=g, rows=(lo, ce, al, re), s=s, B_s=B_s, u=u, B_u=B_u, lp=lp, code=code, cnt=cnt, best=best, best_ok=best_ok,
                second=second, second_ok=second_ok & best_ok)


def shortlist(S, M):
    """step 4b in longdouble: (cand [N, M] ascending, decided [N]).  Decided: every donor taken lies above every donor left out by
    more than their two bounds.  Where the last donor taken and the first one left out tie structurally (the same bits on every side:
    the index decides; two donors at -inf tie likewise), the donors of that tie are set aside and all others have to be clear of it."""
    u, B, code, lp, N, D = S["u"], S["B_u"] * F, S["code"], S["lp"], S["N"], S["D"]
    M = min(M, D)
    order = np.argsort(-u.astype(LD), axis=1, kind="stable")
    cand = np.sort(order[:, :M], axis=1)
    if M == D:
        return cand, np.ones(N, bool)
    r = np.arange(N)
    last, nxt = order[:, M - 1], order[:, M]
    taken = np.zeros((N, D), bool)
    taken[r[:, None], cand] = True
    ninf = np.isneginf(u.astype(np.float64))
    like_last = ((code == code[r, last][:, None]) & (lp[None, :] == lp[last][:, None])) | (ninf & ninf[r, last][:, None])
    tied = like_last[r, nxt]
    aside = like_last & tied[:, None]
    with np.errstate(invalid="ignore"):
        low_in = np.where(taken & ~aside, u - B, np.inf).min(axis=1)
        high_out = np.where(~taken & ~aside, u + B, -np.inf).max(axis=1)
        u_t, B_t = u[r, last], B[r, last]
        above = ~(taken & ~aside).any(axis=1) | (low_in > u_t + B_t)    # (nobody else taken, or all of them clear of the tie)
        below = ~(~taken & ~aside).any(axis=1) | (u_t - B_t > high_out)  # (nobody else left out, ...)
        clear = np.where(tied, above & below, low_in > high_out)
    return cand, clear


def _decide_slots(v, B, code, ok):
    """(slot, any, decided): per row the first slot among ok that attains the maximum of v, whether there is one, and whether every
    other ok slot is a structural tie of it or further below than the two bounds together"""
    n = v.shape[0]
    r = np.arange(n)
    w = np.where(ok, v, -np.inf)
    j = np.argmax(ok & (w == w.max(axis=1)[:, None]), axis=1)
    tie = code == code[r, j][:, None]
    with np.errstate(invalid="ignore"):
        gap = (w[r, j][:, None] - w).astype(np.float64)
        clear = gap > (B + B[r, j][:, None])
    tie |= np.isneginf(w.astype(np.float64)) & np.isneginf(w[r, j].astype(np.float64))[:, None]
    return j, ok.any(axis=1), (tie | clear | ~ok).all(axis=1)


def chain(S, tab2, M, anchor=None, cand=None, **kw):
    """steps 4b - 8 on the singlets S for one shortlist size and one anchor (None = the reference's best); cand: the shortlist the chain
    runs on (None = the reference's own).  Returns a dict (values longdouble, bounds double)."""
    prm = dr.params(**kw)
    N, D, g = S["N"], S["D"], S["g"]
    M = min(int(M), D)
    lo, ce, al, re = S["rows"]
    own, cand_ok = shortlist(S, M)
    ci = own if cand is None else np.asarray(cand, np.int64)
    r = np.arange(N)
    a = S["best"] if anchor is None else np.asarray(anchor, np.int64)
    t2 = np.asarray(tab2, np.float64).astype(LD)
    ga = g[lo, a[ce]]
    gd = g[lo[:, None], ci[ce]]  # [nnz, M]
    t = t2[lo[:, None], 4 * ga[:, None] + gd]
    pa, pb = al.astype(LD)[:, None] * t[:, :, 0], re.astype(LD)[:, None] * t[:, :, 1]
    p, cnt = dr._seg_sum(ce, pa + pb, N)
    mag, _ = dr._seg_sum(ce, np.abs(pa) + np.abs(pb), N)
    B_p = (cnt[:, None] + 1.0) * U * mag.astype(np.float64)
    rate = float(prm["doublet_rate"])
    ls = math.log(1.0 - rate)
    lpair = (math.log(rate / float(D - 1)) if rate > 0 else -math.inf) if D > 1 else 0.0
    fin = lambda v: np.abs(np.where(np.isfinite(v), v, 0)).astype(np.float64)
    x = S["u"] + LD(ls)
    pair_ok = ci != a[:, None]
    y = np.where(pair_ok, p + LD(lpair), LD(-np.inf))
    B_x, B_y = S["B_u"] + U * fin(x), B_p + U * fin(y)
    tt = np.concatenate([x, y], axis=1)
    B_t = np.concatenate([B_x, B_y], axis=1)
    m = tt.max(axis=1)
    d = tt - m[:, None]
    ex = np.exp(d)
    den = ex.sum(axis=1)
    w = ex / den[:, None]
    live = np.isfinite(tt.astype(np.float64))
    e = B_t + np.where(live, B_t, 0).max(axis=1)[:, None] + U * fin(d)
    rel_k = np.expm1(e) + dr.C_EXP * U
    rel_den = np.where(live, rel_k, 0).max(axis=1) + (D + M) * U
    rel_w = ((1.0 + rel_k) * (1.0 + U) / (1.0 - rel_den[:, None]) - 1.0) * F
    post_all, ppost = w[:, :D], w[:, D:]
    dp = ppost.sum(axis=1)
    B_dp = ((rel_w[:, D:] * ppost.astype(np.float64)).sum(axis=1) + M * U * dp.astype(np.float64)) * F
    j, have_pair, pair_dec = _decide_slots(y, B_y * F, S["code"][r[:, None], ci], pair_ok)
    best_pair = np.where(have_pair, ci[r, j], NONE)
    best = S["best"]
    pb_ = post_all[r, best]
    thr = float(prm["posterior_threshold"])
    few = S["cnt"] < int(prm["min_loci"])
    status = np.where(few, 255, np.where(dp > 0.5, 1, np.where(pb_ >= thr, 0, 2)))
    dpf, pbf = dp.astype(np.float64), pb_.astype(np.float64)
    off_half = np.abs(dpf - 0.5) > B_dp + np.spacing(0.5)
    off_thr = np.abs(pbf - thr) > rel_w[r, best] * pbf + np.spacing(thr)
    status_ok = few | (off_half & ((dpf > 0.5) | (off_thr & S["best_ok"])))
    return dict(cand_own=own.astype(np.uint16), cand_ok=cand_ok, cand=ci.astype(np.uint16), s=S["s"], B_s=S["B_s"] * F,
                cand_ll=S["s"][r[:, None], ci], B_cand_ll=S["B_s"][r[:, None], ci] * F, cand_pair_ll=p, B_cand_pair_ll=B_p * F,
                cand_posterior=post_all[r[:, None], ci], rel_post=rel_w[:, :D][r[:, None], ci], cand_pair_posterior=ppost,
                rel_pair=rel_w[:, D:], best_posterior=pb_, rel_best=rel_w[r, best], doublet_posterior=dp, B_dp=B_dp,
                best=best.astype(np.uint16), second=np.asarray(S["second"]).astype(np.uint16), best_pair=best_pair.astype(np.uint16),
                status=status.astype(np.uint8), anchor=a.astype(np.uint16), n_entries=S["cnt"], best_ok=S["best_ok"],
                second_ok=S["second_ok"], pair_ok=pair_dec, status_ok=status_ok)


def compare(ref, got):
    """got: the dict of Cellector.donor_panel (or the twin's) whose cand the reference ran on.  Returns ({name: worst observed / bound},
    undecided [cells] bool): sums and posteriors against their bounds, the decisions on the decided cells (inf = a difference there)."""
    assert np.array_equal(ref["cand"], got["cand"])
    out = dict(cand_ll=dr._ratio(got["cand_ll"], ref["cand_ll"], ref["B_cand_ll"]),
               cand_pair_ll=dr._ratio(got["cand_pair_ll"], ref["cand_pair_ll"], ref["B_cand_pair_ll"]),
               cand_posterior=dr._rel_ratio(got["cand_posterior"], ref["cand_posterior"], ref["rel_post"]),
               cand_pair_posterior=dr._rel_ratio(got["cand_pair_posterior"], ref["cand_pair_posterior"], ref["rel_pair"]),
               best_posterior=dr._rel_ratio(got["best_posterior"], ref["best_posterior"], ref["rel_best"]),
               doublet_posterior=dr._ratio(got["doublet_posterior"], ref["doublet_posterior"], ref["B_dp"]))
    if "ll" in got:
        out["ll"] = dr._ratio(got["ll"], ref["s"], ref["B_s"])
    undecided = ~ref["cand_ok"]
    out["cand"] = 0.0 if np.array_equal(ref["cand_own"][ref["cand_ok"]], np.asarray(got["cand"])[ref["cand_ok"]]) else np.inf
    for name, okname in (("best", "best_ok"), ("second", "second_ok"), ("best_pair", "pair_ok"), ("status", "status_ok")):
        dec = ref[okname]
        undecided = undecided | ~dec
        out[name] = 0.0 if np.array_equal(np.asarray(got[name])[dec], ref[name][dec]) else np.inf
    out["n_entries"] = 0.0 if np.array_equal(np.asarray(got["n_entries"]).astype(np.int64), ref["n_entries"]) else np.inf
    return out, undecided


# ---- the cases -------------------------------------------------------------------------------------------------------------------
DONORS = (1, 2, 33, 64, 65, 96, 127, 128, 129, 1000, 2048, 2049, 4096)  # every Q = 1 ... 64, the edges of a lane's block and of a word
SHORTLISTS = (1, 2, 8, 33, 64)


def case_prior(D, ruled_out=0):
    """a prior that is not flat; ruled_out donors at -inf (spread over the panel), at least one left"""
    rng = np.random.default_rng(29 + D)
    lp = np.log(rng.dirichlet(np.ones(D) * 3.0))
    k = min(int(ruled_out), D - 1)
    if k:
        lp[rng.choice(D, k, replace=False)] = -np.inf
    return lp


def planted_panel(seed, D):
    """dr.planted_pool(seed) with its three called donors at random rows of a panel of D donors of random calls (p = 0.45 / 0.3 / 0.25,
    10 % blanked).  Returns (L, N, coo, gt [D, L], rows [3], truth, parents)."""
    L, N, coo, gt4, truth, par = dr.planted_pool(seed)
    rng = np.random.default_rng(1000 * seed + D)
    gt = rng.choice(3, (D, L), p=[0.45, 0.3, 0.25]).astype(np.uint8)
    gt[rng.random((D, L)) < 0.1] = 3
    rows = np.sort(rng.choice(D, 3, replace=False))
    gt[rows] = gt4[:3]
    return L, N, coo, gt, rows, truth, par
