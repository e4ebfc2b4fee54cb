"""High-precision reference of the K-class doublet scoring (cellector_class_pair_alpha_betas / _class_doublets /
cellector_refine_class_doublets; the second half of csrc/kernels_classes.hip) and the device's error bound.

A plain helper for the tests (no fixtures, no GPU), built on class_reference.py and tile_reference.py and independent of
cellector_amd/classes.py.  From a matrix in COO form over its used loci, a labelling (0..K-1, 255 = unlabelled) and held flags it
forms

  * the integer tallies over the unheld labelled cells (class_reference.tallies with the held cells sent to slot K);
  * the K singlet distributions (class_reference.alpha_betas) and the P = K (K - 1) / 2 pair distributions alpha_ab = (alt_a * ps_a
    + alt_b * ps_b) + 1 in numpy doubles: two rounded products, a rounded sum, a rounded + 1, the device's bits; the default
    ps_k = n_min / n_k and the default priors log(f_k), log(N / 1000 / 100 * max(min(f_a, f_b), 0.1)) with Python's log;
  * the K + P per-cell sums in 80-bit longdouble (class_reference.CellSums), a dead class or pair -inf;
  * step 6 in longdouble (chain) and for one cell in mpmath (chain_mp): the terms t are the live singlets in ascending k, then the
    live pairs in ascending p; x_t = prior_t + sum_t, den = m + log(sum_t exp(x_t - m)), posterior_k = exp(x_k - den), q_p =
    exp(y_p - den), doublet_posterior = sum_p q_p, best / best_pair the first maxima, call = doublet_posterior > 0.5, rest = (call ?
    sum_k posterior_k : sum_{k != best} posterior_k + doublet_posterior).

The device's bound is class_reference's derivation with K' = live singlets + live pairs terms (u = 2^-53; nothing is fitted):

  e_t      = B_t + u |x_t| + u |prior_t|   (the sum's bound with G partial sums, the rounding of prior + sum, a unit of the prior)
  E_den    = sum_t w_t e_t + (0.37 (K' - 1) + 2 + (K' - 1) + 2 ln K') u + u |den|,   w_t = exp(x_t - den): the softmax weights of
             ALL K' terms, which add up to 1 (class_reference's docstring counts the operations; they are the same here, the
             device's sum runs over the K' terms in one order)
  rel_t    = expm1(e_t + E_den + u |x_t - den|) + 2 u,   for posterior_k and for q_p
  doublet_posterior = sum_p q_p: absolute error <= sum_p q_p rel_p + (P' - 1) u sum_p q_p (P' live pairs, P' - 1 additions of
             non-negative terms), i.e. rel_d = (sum_p q_p rel_p) / doublet_posterior + (P' - 1) u
  all widened by posterior_reference.REF_SHARE for the reference's own roundings.

Bands.  best: as class_reference, over the live singlets: x_best - x_k < BAND (e_best + e_k) for some live k != best.  best_pair:
the same over the live pairs.  call: |doublet_posterior - 0.5| <= rel_d * doublet_posterior, the bound itself around the
threshold (no factor: outside it the device's comparison cannot come out the other way).  Inside a band the output is not
compared.  qual depends on best and call: compared where both are clear, by class_reference.qual_range's admitted-range rule with
rel_rest = the largest rel of rest's terms + (their number - 1) u.
"""
import math

import numpy as np

import class_reference as cr
import posterior_reference as pr
import tile_reference as tr

LD = np.longdouble
U = tr.U53
UNLABELLED = cr.UNLABELLED
BAND = cr.BAND
SENSITIVE = cr.SENSITIVE


def n_pairs(K):
    return K * (K - 1) // 2


def pairs(K):
    return [(a, b) for a in range(K) for b in range(a + 1, K)]


def unheld(labels, held):
    labels = np.asarray(labels, np.uint8)
    return labels if held is None else np.where(np.asarray(held) != 0, UNLABELLED, labels).astype(np.uint8)


def default_pair_scales(cells, K):
    live = [int(x) for x in cells[:K] if x]
    n_min = min(live)
    return [float(n_min) / float(int(x)) if x else 0.0 for x in cells[:K]]


def fractions(cells, K):
    n_lab, k_live = int(sum(cells[:K])), int(sum(1 for x in cells[:K] if x))
    return [(int(x) + 1.0) / (float(n_lab) + float(k_live)) for x in cells[:K]]


def default_log_pair_priors(cells, K, N):
    f = fractions(cells, K)
    return [math.log((float(N) / 1000.0 / 100.0) * max(min(f[a], f[b]), 0.1)) for a, b in pairs(K)]


def pair_alpha_betas(alt, ref, ps):
    out = []
    for a, b in pairs(len(ps)):
        out.append(((alt[a].astype(np.float64) * ps[a] + alt[b].astype(np.float64) * ps[b]) + 1.0,
                    (ref[a].astype(np.float64) * ps[a] + ref[b].astype(np.float64) * ps[b]) + 1.0))
    return out


# ---- step 6 ----------------------------------------------------------------------------------------------------------------
def chain(s_ld, sp_ld, lp, lpp, live):
    """longdouble, per cell, from the K + P sums (rows of dead classes / pairs are ignored) and their log priors"""
    K = len(live)
    ab = pairs(K)
    ks = [k for k in range(K) if live[k]]
    ps = [p for p, (a, b) in enumerate(ab) if live[a] and live[b]]
    n = len(s_ld[ks[0]])
    x, y = np.full((K, n), -np.inf, LD), np.full((len(ab), n), -np.inf, LD)
    for k in ks:
        x[k] = LD(lp[k]) + np.asarray(s_ld[k], LD)
    for p in ps:
        y[p] = LD(lpp[p]) + np.asarray(sp_ld[p], LD)
    with np.errstate(invalid="ignore", divide="ignore"):
        ms = x[ks].max(axis=0)
        best = np.array(ks)[np.argmax(x[ks] == ms, axis=0)]
        m = ms
        bp = np.full((n, 2), UNLABELLED, np.uint8)
        if ps:
            mp = y[ps].max(axis=0)
            bp = np.array([ab[p] for p in ps], np.uint8)[np.argmax(y[ps] == mp, axis=0)]
            m = np.maximum(ms, mp)
        den = m + np.log(sum((np.exp(x[k] - m) for k in ks), np.zeros(n, LD)) + sum((np.exp(y[p] - m) for p in ps), np.zeros(n, LD)))
        post, q = np.zeros((K, n), LD), np.zeros((len(ab), n), LD)
        for k in ks:
            post[k] = np.exp(x[k] - den)
        for p in ps:
            q[p] = np.exp(y[p] - den)
    if not tr.HAVE_X87:
        for i in range(n):
            pm, qm = chain_mp([s_ld[k][i] if live[k] else None for k in range(K)], [sp_ld[p][i] if p in ps else None for p in range(len(ab))],
                              lp, lpp, live)
            post[:, i], q[:, i] = [LD(float(v)) for v in pm], [LD(float(v)) for v in qm]
    dp = sum((q[p] for p in ps), np.zeros(n, LD))
    call = (dp > LD(0.5)).astype(np.uint8)
    others = sum((np.where(best == k, LD(0), post[k]) for k in ks), np.zeros(n, LD))
    every = sum((post[k] for k in ks), np.zeros(n, LD))
    rest = np.where(call == 1, every, others + dp)
    return dict(x=x, y=y, m=m, den=den, posterior=post, q=q, doublet_posterior=dp, best=best.astype(np.uint8), best_pair=bp, call=call,
                rest=rest, live=np.asarray(live, bool), ks=ks, ps=ps)


def chain_mp(s, sp, lp, lpp, live):
    """one cell with mpmath at 50 digits: (posteriors [K], q [P])"""
    import mpmath as mp
    mp.mp.dps = 50
    K = len(live)
    ab = pairs(K)
    x = {("s", k): pr._mpf(lp[k]) + pr._mpf(s[k]) for k in range(K) if live[k]}
    x.update({("p", p): pr._mpf(lpp[p]) + pr._mpf(sp[p]) for p, (a, b) in enumerate(ab) if live[a] and live[b]})
    fin = {t: v for t, v in x.items() if v != mp.mpf("-inf")}
    den = mp.log(sum(mp.exp(v) for v in fin.values()))
    return ([mp.exp(fin[("s", k)] - den) if ("s", k) in fin else mp.mpf(0) for k in range(K)],
            [mp.exp(fin[("p", p)] - den) if ("p", p) in fin else mp.mpf(0) for p in range(len(ab))])


# ---- a (labels, held)'s reference and its bound ----------------------------------------------------------------------------------
def reference(L, N, coo, labels, K, held=None, scale=None, pair_scale=None, log_prior=None, log_pair_prior=None, mask=None, sums_of=None):
    labels = np.asarray(labels, np.uint8)
    eff = unheld(labels, held)
    cells, alt, ref = cr.tallies(L, coo, eff, K)
    ab = cr.alpha_betas(alt[:K], ref[:K], scale)
    live = [bool(cells[k]) for k in range(K)]
    ps = default_pair_scales(cells, K) if pair_scale is None else [float(v) for v in pair_scale]
    pab = pair_alpha_betas(alt[:K], ref[:K], ps)
    lp = cr.default_log_priors(cells, K) if log_prior is None else [float(v) for v in log_prior]
    lpp = default_log_pair_priors(cells, K, N) if log_pair_prior is None else [float(v) for v in log_pair_prior]
    cs = sums_of if sums_of is not None else cr.CellSums(N, coo, mask)
    sums = [cs(ab[k][0], ab[k][1]) if live[k] else None for k in range(K)]
    psums = [cs(pab[p][0], pab[p][1]) if live[a] and live[b] else None for p, (a, b) in enumerate(pairs(K))]
    ch = chain([s["ll_ld"] if s else None for s in sums], [s["ll_ld"] if s else None for s in psums], lp, lpp, live)
    count = next(s["count"] for s in sums if s)
    return dict(N=N, L=L, K=K, P=n_pairs(K), labels=labels, held=held, cells=cells, alt=alt, ref=ref, ab=ab, pab=pab, live=live, lp=lp,
                lpp=lpp, ps=ps, sums=sums, psums=psums, chain=ch, count=count, mask=mask, _bounds={})


def _f64(x):
    with np.errstate(invalid="ignore"):
        return np.abs(x).astype(np.float64)


def bounds(ref, G):
    """dict: B / Bp (per-cell bounds of the sums), e (per term), rel [K, N], rel_q [P, N], rel_d [N], band_best, band_pair, band_call
    [N] bool, rel_rest [N]"""
    if G in ref["_bounds"]:
        return ref["_bounds"][G]
    ch, K, P, N = ref["chain"], ref["K"], ref["P"], ref["N"]
    ks, ps = ch["ks"], ch["ps"]
    kl = len(ks) + len(ps)
    B = [tr.cell_bound(ref["sums"][k], G)[0] if k in ks else None for k in range(K)]
    Bp = [tr.cell_bound(ref["psums"][p], G)[0] if p in ps else None for p in range(P)]

    def err(bound, x, prior):  # (a caller's prior may be -inf: the term is exactly 0)
        fin = np.isfinite(x.astype(np.float64))
        return np.where(fin, bound + U * np.where(fin, _f64(x), 0.0) + U * (abs(prior) if math.isfinite(prior) else 0.0), 0.0), fin

    e, fin = {}, {}
    for k in ks:
        e["s", k], fin["s", k] = err(B[k], ch["x"][k], ref["lp"][k])
    for p in ps:
        e["p", p], fin["p", p] = err(Bp[p], ch["y"][p], ref["lpp"][p])
    w = {("s", k): ch["posterior"][k].astype(np.float64) for k in ks}
    w.update({("p", p): ch["q"][p].astype(np.float64) for p in ps})
    e_den = sum(w[t] * e[t] for t in e) + (0.37 * (kl - 1) + 2 + (kl - 1) + 2 * math.log(kl)) * U + U * _f64(ch["den"])

    def rel_of(t, x):
        d = np.where(fin[t], _f64(x - ch["den"]), 0.0)
        return (np.expm1(e[t] + e_den + U * d) + pr.C_EXP * U) * (1.0 + pr.REF_SHARE)

    rel, rel_q = np.zeros((K, N)), np.zeros((P, N))
    for k in ks:
        rel[k] = rel_of(("s", k), ch["x"][k])
    for p in ps:
        rel_q[p] = rel_of(("p", p), ch["y"][p])
    dp = ch["doublet_posterior"].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        num = sum((w["p", p] * rel_q[p] for p in ps), np.zeros(N))
        rel_d = np.where(dp > 0, num / np.where(dp > 0, dp, 1.0), rel_q.max(axis=0) if ps else 0.0) + max(len(ps) - 1, 0) * U

    def band(terms, first, xs):
        """a first maximum among `terms` that another term comes within BAND errors of.  Not a band: two terms whose sums both have
        a zero bound (no entry, or zero-total entries only: the device's sums are exactly the reference's) under one and the same
        prior double.  The device adds the same two doubles on both sides: an exact tie there as here, which both resolve to the
        lower index."""
        out = np.zeros(N, bool)
        if not terms:
            return out
        ix = {t: j for j, t in enumerate(terms)}
        pos = np.array([ix[t] for t in first])
        xb = xs[pos, np.arange(N)]
        eb = np.stack([e[t] for t in terms])[pos, np.arange(N)]
        bb = np.stack([bsum[t] for t in terms])[pos, np.arange(N)]
        pb = np.array([prior[t] for t in terms])[pos]
        for j, t in enumerate(terms):
            with np.errstate(invalid="ignore"):
                gap = (xb - xs[j]).astype(np.float64)
            exact_tie = (bb == 0) & (bsum[t] == 0) & (pb == prior[t]) & (gap == 0)
            out |= (pos != j) & (gap < BAND * (eb + e[t])) & ~exact_tie
        return out

    bsum = {("s", k): B[k] for k in ks}
    bsum.update({("p", p): Bp[p] for p in ps})
    prior = {("s", k): ref["lp"][k] for k in ks}
    prior.update({("p", p): ref["lpp"][p] for p in ps})

    sing = [("s", k) for k in ks]
    band_best = band(sing, [("s", int(k)) for k in ch["best"]], np.stack([ch["x"][k] for k in ks]))
    pidx = {ab: p for p, ab in enumerate(pairs(K))}
    band_pair = band([("p", p) for p in ps], [("p", pidx[(int(a), int(b))]) for a, b in ch["best_pair"]] if ps else [],
                     np.stack([ch["y"][p] for p in ps]) if ps else None)
    band_call = np.abs(dp - 0.5) <= rel_d * dp
    # rest: call 1 -> every singlet posterior; call 0 -> the singlets but best, and doublet_posterior (when there is a live pair)
    best = ch["best"].astype(np.int64)
    call = ch["call"] == 1
    rel_rest, terms = np.zeros(N), np.zeros(N)
    for k in ks:
        inc = call | (best != k)
        rel_rest = np.where(inc, np.maximum(rel_rest, rel[k]), rel_rest)
        terms += inc
    if ps:
        rel_rest = np.where(~call, np.maximum(rel_rest, rel_d), rel_rest)
        terms += ~call
    rel_rest = rel_rest + np.maximum(terms - 1, 0) * U
    ref["_bounds"][G] = dict(B=B, Bp=Bp, e=e, rel=rel, rel_q=rel_q, rel_d=rel_d, band_best=band_best, band_pair=band_pair,
                             band_call=band_call, rel_rest=rel_rest)
    return ref["_bounds"][G]


def qual_range(ref, G):
    """class_reference.qual_range's rule on this chain's rest and rel_rest"""
    shim = dict(chain=dict(rest=ref["chain"]["rest"]), _bounds={G: dict(rel_rest=bounds(ref, G)["rel_rest"])})
    return cr.qual_range(shim, G)


def _sum_ratio(v, r, B):
    bound = B * (1.0 + pr.REF_SHARE) + np.where(B > 0, 0.5 * np.spacing(np.abs(r["ll"])), 0.0)
    d = np.abs(v - r["ll"])
    ratio = np.where(bound > 0, d / np.where(bound > 0, bound, 1.0), np.where(d == 0, 0.0, np.inf))
    return np.where(np.isfinite(v), ratio, np.inf)


def _rel_ratio(p, want, rel):
    seen = want >= pr.OBSERVABLE
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = (np.abs(p.astype(LD) - want) / (rel * np.where(seen, want, LD(1)))).astype(np.float64)
    ratio = np.where(seen, ratio, np.where((p >= 0) & (p < pr.UNOBSERVED_BELOW), 0.0, np.inf))
    return np.where(np.isfinite(p), ratio, np.inf)


def compare(ref, got, G):
    """got: dict of ll [K, N], ll_pair [P, N], posterior [K, N], doublet_posterior, best, best_pair [N, 2], call, qual.  Returns
    {name: (worst observed / bound, cells beyond it)} for ll, ll_pair, posterior, doublet_posterior and {name: (cells compared,
    cells that differ)} for best, best_pair, call, qual; "left_out": cells in any band or, for doublet_posterior, unobservable."""
    b = bounds(ref, G)
    ch, K, P, N = ref["chain"], ref["K"], ref["P"], ref["N"]
    none = np.zeros(0, np.int64)
    worst = dict(ll=0.0, ll_pair=0.0, posterior=0.0)
    bad = dict(ll=[none], ll_pair=[none], posterior=[none])
    for k in range(K):
        v, p = np.asarray(got["ll"][k], np.float64), np.asarray(got["posterior"][k], np.float64)
        if not ref["live"][k]:
            if not (np.isneginf(v).all() and (p == 0).all()):
                worst["ll"] = worst["posterior"] = math.inf
                bad["ll"].append(np.nonzero(~np.isneginf(v))[0]); bad["posterior"].append(np.nonzero(p != 0)[0])
            continue
        r = _sum_ratio(v, ref["sums"][k], b["B"][k])
        worst["ll"] = max(worst["ll"], float(r.max())); bad["ll"].append(np.nonzero(r > 1.0)[0])
        r = _rel_ratio(p, ch["posterior"][k], b["rel"][k])
        worst["posterior"] = max(worst["posterior"], float(r.max())); bad["posterior"].append(np.nonzero(r > 1.0)[0])
    for p in range(P):
        v = np.asarray(got["ll_pair"][p], np.float64)
        if p not in ch["ps"]:
            if not np.isneginf(v).all():
                worst["ll_pair"] = math.inf; bad["ll_pair"].append(np.nonzero(~np.isneginf(v))[0])
            continue
        r = _sum_ratio(v, ref["psums"][p], b["Bp"][p])
        worst["ll_pair"] = max(worst["ll_pair"], float(r.max())); bad["ll_pair"].append(np.nonzero(r > 1.0)[0])
    out = {k: (worst[k], np.unique(np.concatenate(bad[k]))) for k in worst}
    dpg = np.asarray(got["doublet_posterior"], np.float64)
    if ch["ps"]:
        r = _rel_ratio(dpg, ch["doublet_posterior"], b["rel_d"])
    else:
        r = np.where(dpg == 0, 0.0, np.inf)
    out["doublet_posterior"] = (float(r.max()), np.nonzero(r > 1.0)[0])
    cb, cp, cc = ~b["band_best"], ~b["band_pair"], ~b["band_call"]
    out["best"] = (int(cb.sum()), np.nonzero(cb & (np.asarray(got["best"]) != ch["best"]))[0])
    out["best_pair"] = (int(cp.sum()), np.nonzero(cp & (np.asarray(got["best_pair"]).reshape(N, 2) != ch["best_pair"]).any(axis=1))[0])
    out["call"] = (int(cc.sum()), np.nonzero(cc & (np.asarray(got["call"]) != ch["call"]))[0])
    lo, hi = qual_range(ref, G)
    q = np.asarray(got["qual"], np.uint64)
    cq = cb & cc
    out["qual"] = (int(cq.sum()), np.nonzero(cq & ((q < lo) | (q > hi)))[0])
    out["qual_edges"] = int((cq & (lo != hi)).sum())
    unobs = (ch["doublet_posterior"] < pr.OBSERVABLE) if ch["ps"] else np.zeros(N, bool)
    out["left_out"] = int((b["band_best"] | b["band_pair"] | b["band_call"] | unobs).sum())
    return out


NAMES = ("ll", "ll_pair", "posterior", "doublet_posterior", "best", "best_pair", "call", "qual")


def ok(res):
    return all(res[k][1].size == 0 for k in NAMES)


def describe(ref, got, res, n=4):
    lines = []
    for name in NAMES:
        bad = res[name][1]
        if bad.size:
            i = bad[:n]
            g = np.asarray(got[name])
            g = g[i] if name in ("doublet_posterior", "best", "best_pair", "call", "qual") else g[..., i]
            lines.append(f"{name}: {bad.size} of {ref['N']} cells (worst / compared {res[name][0]}), first {i}: device {g.tolist()}, "
                         f"entries {ref['count'][i]}, reference best {ref['chain']['best'][i]}, doublet_posterior "
                         f"{ref['chain']['doublet_posterior'][i].astype(np.float64)}")
    return "; ".join(lines)


def left_out(ref, G):
    """cells the reference leaves out of some comparison: inside a band, or (with a live pair) a doublet posterior below OBSERVABLE"""
    b = bounds(ref, G)
    ch = ref["chain"]
    unobs = (ch["doublet_posterior"] < pr.OBSERVABLE) if ch["ps"] else np.zeros(ref["N"], bool)
    return b["band_best"] | b["band_pair"] | b["band_call"] | unobs


# ---- sensitivity ---------------------------------------------------------------------------------------------------------------------
def drop_one_pair_entry(ref, coo, G, p, j):
    """entry j of the COO (a cell of class a or b of pair p) left out of the pair's distribution: the largest |change of ll_pair_p|
    over the cells with an entry at that locus, in units of the cell's bound"""
    lo, ce, al, re = (np.asarray(x, np.int64) for x in coo)
    a, b = pairs(ref["K"])[p]
    l = lo[j]
    side = a if unheld(ref["labels"], ref["held"])[ce[j]] == a else b
    other = b if side == a else a
    ps = ref["ps"]
    pa, pb = ref["pab"][p]
    terms_a = {side: (float(ref["alt"][side, l]) - al[j]) * ps[side], other: float(ref["alt"][other, l]) * ps[other]}
    terms_r = {side: (float(ref["ref"][side, l]) - re[j]) * ps[side], other: float(ref["ref"][other, l]) * ps[other]}
    a2, b2 = (terms_a[a] + terms_a[b]) + 1.0, (terms_r[a] + terms_r[b]) + 1.0
    if ref["mask"] is not None and not ref["mask"][l]:
        return 0.0
    at = np.nonzero(lo == l)[0]
    t0, _, _ = tr.term_values(np.full(len(at), pa[l]), np.full(len(at), pb[l]), al[at], re[at])
    t1, _, _ = tr.term_values(np.full(len(at), a2), np.full(len(at), b2), al[at], re[at])
    delta = np.zeros(ref["N"], LD)
    np.add.at(delta, ce[at], t1 - t0)
    B = bounds(ref, G)["Bp"][p]
    with np.errstate(divide="ignore", invalid="ignore"):
        moved = np.where(delta != 0, np.abs(delta).astype(np.float64) / B, 0.0)
    return float(moved.max())


def drop_smallest_pair_term(ref, G):
    """the denominator formed without each cell's smallest live pair term: the largest relative change of a posterior (every output
    grows by 1 / (1 - q_min)), in units of its bound"""
    ch = ref["chain"]
    if not ch["ps"]:
        return math.inf
    b = bounds(ref, G)
    qmin = np.min(np.stack([ch["q"][p] for p in ch["ps"]]), axis=0).astype(np.float64)
    with np.errstate(divide="ignore"):
        change = qmin / (1.0 - qmin)  # (a cell whose one pair takes everything: nothing else is left, inf)
    relmax = np.maximum(b["rel"][ch["ks"]].max(axis=0), b["rel_q"][ch["ps"]].max(axis=0))
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.nanmax(np.where(qmin < 1.0, change / relmax, np.inf)))


# ---- the cases of the sweep --------------------------------------------------------------------------------------------------------
def reference_doublet_scales(n_excluded, n_cells):
    """pair_scale and the pair prior that make K = 2 the reference's three-way posterior (main.rs:245-246, :259), as the host
    computes them"""
    mf0 = (n_excluded + 1.0) / (n_cells + 1.0)
    return [1.0, mf0], [pr.priors(n_excluded, n_cells)[3]]


def case_names(mname):
    """(K, which): K = 2 from the matrix' exclusion sets, K = 3 / 5 from a seeded draw with 5 % unlabelled and 5 % held; K = 16 on
    row-lengths only"""
    return [(2, s) for s in cr.K2_SETS] + [(3, "draw"), (5, "draw")] + ([(16, "draw")] if mname == "row-lengths" else [])


def case_inputs(mname, K, which):
    """(labels, held, scale, pair_scale, log_prior, log_pair_prior)"""
    L, N, coo, _ = pr.matrix(mname)
    if which == "draw":
        rng = np.random.default_rng(1000 * K + N)
        lab = rng.integers(0, K, N).astype(np.uint8)
        lab[rng.random(N) < 0.05] = UNLABELLED
        held = (rng.random(N) < 0.05).astype(np.uint8)
        return lab, held, None, None, None, None
    lab, scale, lp = cr.case_labels(mname, 2, which)
    ps, lpp = reference_doublet_scales(int((lab == 0).sum()), N)
    return lab, None, scale, ps, lp, lpp


_cases = {}


def case(mname, K, which, masked):
    key = (mname, K, which, bool(masked))
    if key not in _cases:
        L, N, coo, _ = pr.matrix(mname)
        lab, held, scale, ps, lp, lpp = case_inputs(mname, K, which)
        mask = cr.case_mask(mname) if masked else None
        if (mname, bool(masked)) not in cr._sums:
            cr._sums[(mname, bool(masked))] = cr.CellSums(N, coo, mask)
        ref = reference(L, N, coo, lab, K, held, scale, ps, lp, lpp, mask, cr._sums[(mname, bool(masked))])
        ref["args"] = dict(held=held, scale=scale, pair_scale=ps, log_prior=lp, log_pair_prior=lpp, mask=mask)
        _cases[key] = ref
    return _cases[key]


# ---- the refine mixture with planted doublets ------------------------------------------------------------------------------------
N_DOUBLETS = 60
RATES = (0.0, 0.5)
DOUBLET_SEED = 11
_dmix = {}


def doublet_mixture(rate, seed=5):
    """class_reference.mixture() plus N_DOUBLETS synthetic doublets (cellector_amd.doublets, the twin of cellector_add_doublets)
    from cross-genotype parents among the 900 cells, the parents' reads thinned at `rate`.  Returns (L, N, coo, truth [N] with the
    doublets 255, parents [N_DOUBLETS, 2] as genotypes (a < b))."""
    if (rate, seed) not in _dmix:
        from cellector_amd import doublets as dbl
        L, N0, coo, truth = cr.mixture(seed)
        rng = np.random.default_rng(DOUBLET_SEED + seed)
        a, b = [], []
        while len(a) < N_DOUBLETS:
            i, j = rng.integers(0, cr.MIX_N, 2)
            if truth[i] != truth[j]:
                a.append(i); b.append(j)
        a, b = np.array(a), np.array(b)
        lo, ce, al, re, n, _, _ = dbl.add_doublets_coo(coo, N0, a, b, rate, seed=4)
        par = np.sort(np.stack([truth[a], truth[b]], axis=1), axis=1)
        _dmix[(rate, seed)] = (L, int(n), [np.asarray(x, np.int64) for x in (lo, ce, al, re)],
                               np.concatenate([truth, np.full(N_DOUBLETS, UNLABELLED, np.uint8)]), par)
    return _dmix[(rate, seed)]


DOUBLET_STARTS = ("truth", "noisy")


def doublet_start(which, rate, seed=5):
    """(labels, K = 3): "truth": every singlet its genotype, every doublet the genotype of its first parent (a caller does not know
    them); "noisy": 15 % of those labels reassigned at random and 5 % unlabelled.  Nothing is held at the start."""
    L, N, coo, truth, par = doublet_mixture(rate, seed)
    start = truth.copy()
    start[N - N_DOUBLETS:] = par[:, 0]
    if which == "noisy":
        rng = np.random.default_rng(seed + 21)
        r = rng.random(N)
        start[r < 0.15] = rng.integers(0, 3, int((r < 0.15).sum()))
        start[r > 0.95] = UNLABELLED
        start[cr.MIX_N:cr.MIX_N + 6] = np.arange(6) % 3  # the one-entry cells stay labelled
    return start, 3
