"""High-precision reference of the K-genotype class scoring (cellector_class_tallies / _class_alpha_betas / _class_posteriors /
cellector_refine_classes; csrc/kernels_classes.hip) and the device's error bound.

A plain helper for the tests (no fixtures, no GPU), independent of cellector_amd/classes.py.  From a matrix in COO form over its
used loci and a labelling (0..K-1, 255 = unlabelled) it forms

  * the integer tallies per (class, locus), slot K the unlabelled cells (tallies: np.bincount over a combined key with whole-number
    weights, exact below 2^53, which is asserted);
  * alpha_k = alt_k * scale_k + 1, beta_k likewise, in numpy doubles: a rounded product and a rounded sum, the device's bits;
  * the K per-cell sums in 80-bit longdouble (tile_reference.cell_reference, key ll_ld), a dead class (no cell) -inf;
  * step 6 from those sums in longdouble (chain), for one cell in mpmath (chain_mp), and in double in the device's order
    (chain_double):  x_k = lp_k + ll_k, m = max, den = m + log(sum exp(x_k - m)), posterior_k = exp(x_k - den), best = the lowest k
    attaining m, rest = sum_{k != best} posterior_k, qual = (int) min(-10 log10(rest), 255).

The device's bound (u = 2^-53; nothing here is fitted to observed errors), for K' live classes:

  B_k      tile_reference.cell_bound of the sum of class k with G partial sums (posterior_reference's docstring names G).
  e_k      = B_k + u |x_k| + u |lp_k|: the sum's error, the rounding of lp_k + ll_k, one unit of the prior (the host's log and
           numpy's need not agree in the last bit).
  den      the errors of the arguments enter with the softmax weights w_k = posterior_k (the derivatives of logsumexp, positive,
           adding up to 1): sum_k w_k e_k.  Its own operations: d_k = x_k - m rounds once, u |d_k|, and exp is good to an ulp, at
           most 2 u relative (ROCm device-libs: "exp: 1 ulp", "log: 1 ulp"); term k enters S = sum exp(d_k) with weight
           exp(d_k) / S <= 1 and |d| e^d <= 0.37: 0.37 u for each of the K' - 1 terms below the largest (its d is exactly 0) and 2 u
           for the exps together; the K' - 1 additions round once each, (K' - 1) u relative on S, i.e. absolute on its log; log(S)
           lies in [0, ln K']: one ulp of it, at most 2 u ln K'; the addition m + log(S): u |den|.
           E_den = sum_k w_k e_k + (0.37 (K' - 1) + 2 + (K' - 1) + 2 ln K') u + u |den|
  rel(posterior_k) <= expm1(e_k + E_den + u |x_k - den|) + 2 u: the subtraction's rounding; exp turns the absolute error of its
           argument into a relative one and adds an ulp of its own.
  The reference repeats these operations at 2^-64: both are widened by posterior_reference.REF_SHARE of themselves for it.

best: the device takes the largest of its own x_k.  A cell is inside the margin band when for some live k != best
x_best - x_k < BAND (e_best + e_k), BAND = 1000: there the device's best (and with it qual, and in a refine step the cell's
next label) is not compared.  Outside it best is exact.  qual is the integer part of v = -10 log10(rest): rest carries the largest
rel of its terms and K' - 2 additions, v four more units of its own size (log10 good to two ulps, the product); where the interval
this gives v holds an integer both neighbours are accepted, elsewhere qual is exact.
"""
import math

import numpy as np

import posterior_reference as pr
import tile_reference as tr

LD = np.longdouble
U = tr.U53
UNLABELLED = 255
BAND = 1000.0
SENSITIVE = 100.0


# ---- steps 1, 2, 5 ---------------------------------------------------------------------------------------------------------
def tallies(L, coo, labels, K):
    """(cells [K + 1] ints, alt [K + 1, L], ref [K + 1, L] uint64); slot K = the unlabelled cells"""
    lo, ce, al, re = (np.asarray(x, np.int64) for x in coo)
    slot = np.asarray(labels).astype(np.int64)
    slot = np.where(slot == UNLABELLED, K, slot)
    assert ((slot >= 0) & (slot <= K)).all()
    key = slot[ce] * L + lo
    out = []
    for w in (al, re):
        s = np.bincount(key, weights=w.astype(np.float64), minlength=(K + 1) * L)
        assert s.max(initial=0.0) < 2.0 ** 53
        out.append(s.astype(np.uint64).reshape(K + 1, L))
    return np.bincount(slot, minlength=K + 1), out[0], out[1]


def alpha_betas(alt, ref, scale):
    s = np.ones(len(alt)) if scale is None else np.asarray(scale, np.float64)
    return [(alt[k].astype(np.float64) * s[k] + 1.0, ref[k].astype(np.float64) * s[k] + 1.0) for k in range(len(s))]


def default_log_priors(cells, K):
    n_lab, k_live = int(sum(cells[:K])), int(sum(1 for x in cells[:K] if x))
    return [math.log((int(x) + 1.0) / (float(n_lab) + float(k_live))) if x else -math.inf for x in cells[:K]]


# ---- step 6 ----------------------------------------------------------------------------------------------------------------
def chain(s_ld, lp, live):
    """longdouble, per cell, from the K sums (rows of dead classes are ignored) and the K log priors"""
    ks = [k for k in range(len(live)) if live[k]]
    K, n = len(live), len(s_ld[ks[0]])
    x = np.full((K, n), -np.inf, LD)
    for k in ks:
        x[k] = LD(lp[k]) + np.asarray(s_ld[k], LD)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = x[ks].max(axis=0)
        best = np.array(ks)[np.argmax(x[ks] == m, axis=0)]  # the lowest live k attaining m
        den = m + np.log(sum(np.exp(x[k] - m) for k in ks))
        post = np.zeros((K, n), LD)
        for k in ks:
            post[k] = np.exp(x[k] - den)
        rest = sum((np.where(best == k, LD(0), post[k]) for k in ks), np.zeros(n, LD))
    if not tr.HAVE_X87:
        for i in range(n):
            p, r = chain_mp([s_ld[k][i] if live[k] else None for k in range(K)], lp, live)
            post[:, i], rest[i] = [LD(float(v)) for v in p], LD(float(r))
    return dict(x=x, m=m, den=den, posterior=post, best=best.astype(np.uint8), rest=rest, live=np.asarray(live, bool))


def chain_mp(s, lp, live):
    """one cell with mpmath at 50 digits: (posteriors [K], rest)"""
    import mpmath as mp
    mp.mp.dps = 50
    ks = [k for k in range(len(live)) if live[k]]
    x = {k: pr._mpf(lp[k]) + pr._mpf(s[k]) for k in ks}
    fin = [k for k in ks if x[k] != mp.mpf("-inf")]
    den = mp.log(sum(mp.exp(x[k]) for k in fin))
    post = [mp.exp(x[k] - den) if k in fin else mp.mpf(0) for k in range(len(live))]
    best = min(fin, key=lambda k: (-x[k], k))
    return post, sum(post[k] for k in fin if k != best)


def chain_double(ll, lp, live):
    """the device's operations, one cell at a time in Python doubles: (posterior [K, n], best, qual)"""
    ll = np.asarray(ll, np.float64)
    K, n = ll.shape
    post, best, qual = np.zeros((K, n)), np.zeros(n, np.uint8), np.zeros(n, np.uint64)
    ks = [k for k in range(K) if live[k]]
    for i in range(n):
        x = {k: lp[k] + float(ll[k, i]) for k in ks}
        m, b = -math.inf, ks[0]
        for j, k in enumerate(ks):
            if j == 0 or x[k] > m:
                m, b = x[k], k
        s = 0.0
        for k in ks:
            s += math.exp(x[k] - m)
        den = m + math.log(s)
        rest = 0.0
        for k in ks:
            post[k, i] = math.exp(x[k] - den)
            if k != b:
                rest += post[k, i]
        best[i] = b
        qual[i] = 255 if rest == 0.0 else max(0, int(min(-10.0 * math.log10(rest), 255.0)))
    return post, best, qual


def qual_of(rest):
    with np.errstate(divide="ignore"):
        v = np.fmin(-10.0 * np.log10(np.asarray(rest, np.float64)), 255.0)
    return np.where(v > 0, v, 0.0).astype(np.uint64)


# ---- step 3: the per-class sums ------------------------------------------------------------------------------------------------
class CellSums:
    """tile_reference.cell_reference's log-likelihood half for several alpha / beta sets over one matrix and mask: the distinct
    (locus, alt, ref) keys and the cell order are found once and shared by the K classes; the expected column, which the class
    scoring does not use, is not formed.  Every value is cell_reference's to the bit (tests/test_class_reference.py asserts it)."""

    def __init__(self, n_cells, coo, mask=None):
        lo, ce, al, re = (np.asarray(x, np.int64) for x in coo)
        keep = np.ones(len(lo), bool) if mask is None else np.asarray(mask)[lo] != 0
        lo, ce, al, re = lo[keep], ce[keep], al[keep], re[keep]
        assert (al < 65536).all() and (re < 65536).all()
        uk, self.inv = np.unique((lo << 32) | (al << 16) | re, return_inverse=True)
        self.kl, self.ka, self.kr = uk >> 32, (uk >> 16) & 0xFFFF, uk & 0xFFFF
        self.order = np.argsort(ce, kind="stable")
        self.cnt = np.bincount(ce, minlength=n_cells)
        self.starts = np.concatenate([[0], np.cumsum(self.cnt)[:-1]])
        self.n = n_cells

    def _per_cell(self, v):
        v = v[self.inv][self.order]
        out = np.zeros(self.n, v.dtype)
        nz = self.cnt > 0
        if len(v):
            out[nz] = np.add.reduceat(v, self.starts[nz])
        return out

    def __call__(self, alpha, beta):
        alpha, beta = np.asarray(alpha, np.float64), np.asarray(beta, np.float64)
        t, log_ulps, _ = tr.term_values(alpha[self.kl], beta[self.kl], self.ka, self.kr)
        bt = tr.term_bound(self.ka + self.kr, self.ka, log_ulps)
        ll_ld = self._per_cell(t)
        zero = np.zeros(self.n)
        return dict(ll=ll_ld.astype(np.float64), ll_ld=ll_ld, loci_used=self.cnt.astype(np.float64), count=self.cnt,
                    abs_ll=self._per_cell(np.abs(t)).astype(np.float64), b_ll=self._per_cell(bt), abs_ell=zero, b_ell=zero)


# ---- a labelling's reference and its bound -------------------------------------------------------------------------------------
def reference(L, N, coo, labels, K, scale=None, log_prior=None, mask=None, sums_of=None):
    """sums_of: a CellSums of (N, coo, mask) to share between labellings of one matrix"""
    labels = np.asarray(labels, np.uint8)
    cells, alt, ref = tallies(L, coo, labels, K)
    ab = alpha_betas(alt[:K], ref[:K], scale)
    live = [bool(cells[k]) for k in range(K)]
    lp = default_log_priors(cells, K) if log_prior is None else [float(v) for v in log_prior]
    cs = sums_of if sums_of is not None else CellSums(N, coo, mask)
    sums = [cs(ab[k][0], ab[k][1]) if live[k] else None for k in range(K)]
    ch = chain([s["ll_ld"] if s else None for s in sums], lp, live)
    count = next(s["count"] for s in sums if s)
    return dict(N=N, L=L, K=K, labels=labels, cells=cells, alt=alt, ref=ref, ab=ab, live=live, lp=lp, sums=sums, chain=ch,
                count=count, mask=mask, scale_used=[1.0] * K if scale is None else [float(v) for v in scale], _bounds={})


def _f64(x):
    with np.errstate(invalid="ignore"):
        return np.abs(x).astype(np.float64)


def bounds(ref, G):
    """dict: B [K] (per-cell bounds of the sums, None for a dead class), e [K], rel [K, N], in_band [N], rel_rest [N]"""
    if G not in ref["_bounds"]:
        ch, K, N = ref["chain"], ref["K"], ref["N"]
        ks = [k for k in range(K) if ref["live"][k]]
        kl = len(ks)
        B = [tr.cell_bound(ref["sums"][k], G)[0] if ref["live"][k] else None for k in range(K)]
        fin = {k: np.isfinite(ch["x"][k].astype(np.float64)) for k in ks}  # (a caller's prior may be -inf: the term is exactly 0)
        e = {k: np.where(fin[k], B[k] + U * np.where(fin[k], _f64(ch["x"][k]), 0.0) + U * (abs(ref["lp"][k]) if math.isfinite(ref["lp"][k]) else 0.0), 0.0)
             for k in ks}
        w = {k: ch["posterior"][k].astype(np.float64) for k in ks}
        e_den = sum(w[k] * e[k] for k in ks) + (0.37 * (kl - 1) + 2 + (kl - 1) + 2 * math.log(kl)) * U + U * _f64(ch["den"])
        rel = np.zeros((K, N))
        for k in ks:
            d = np.where(fin[k], _f64(ch["x"][k] - ch["den"]), 0.0)
            rel[k] = (np.expm1(e[k] + e_den + U * d) + pr.C_EXP * U) * (1.0 + pr.REF_SHARE)
        best = ch["best"].astype(np.int64)
        xb = np.take_along_axis(ch["x"], best[None, :], 0)[0]
        eb = np.stack([e[k] if k in e else np.zeros(N) for k in range(K)])[best, np.arange(N)]
        in_band = np.zeros(N, bool)
        rel_rest = np.zeros(N)
        for k in ks:
            other = best != k
            with np.errstate(invalid="ignore"):
                gap = (xb - ch["x"][k]).astype(np.float64)
            in_band |= other & (gap < BAND * (eb + e[k]))
            rel_rest = np.where(other, np.maximum(rel_rest, rel[k]), rel_rest)
        rel_rest = rel_rest + max(kl - 2, 0) * U
        ref["_bounds"][G] = dict(B=B, e=e, rel=rel, in_band=in_band, rel_rest=rel_rest)
    return ref["_bounds"][G]


def qual_range(ref, G):
    """(lo, hi) [N]: the quals the bound admits"""
    b = bounds(ref, G)
    rest = ref["chain"]["rest"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        v_hi = -10.0 * np.log10(rest * (1.0 - b["rel_rest"]))
        v_lo = -10.0 * np.log10(rest * (1.0 + b["rel_rest"]))
        v_hi = np.where(rest > 0, v_hi + 4 * U * np.abs(v_hi), np.inf)  # (rest == 0: inf - inf in the branch not taken)
        v_lo = np.where(rest > 0, v_lo - 4 * U * np.abs(v_lo), np.inf)
    f = lambda v: np.where(np.fmin(v, 255.0) > 0, np.fmin(v, 255.0), 0.0).astype(np.uint64)
    return f(v_lo), f(v_hi)


def compare(ref, got, G):
    """got: dict of ll [K, N], posterior [K, N], best, qual.  Returns {name: (worst observed / bound, cells beyond it)} for "ll",
    "posterior" (every class), and {"best", "qual"}: (cells compared, cells that differ)."""
    b = bounds(ref, G)
    ch, K, N = ref["chain"], ref["K"], ref["N"]
    worst_ll, bad_ll, worst_p, bad_p = 0.0, [], 0.0, []
    for k in range(K):
        v, p = np.asarray(got["ll"][k], np.float64), np.asarray(got["posterior"][k], np.float64)
        if not ref["live"][k]:
            if not (np.isneginf(v).all() and (p == 0).all()):
                worst_ll = worst_p = math.inf
                bad_ll.append(np.nonzero(~np.isneginf(v))[0]); bad_p.append(np.nonzero(p != 0)[0])
            continue
        r = ref["sums"][k]
        bound = b["B"][k] * (1.0 + pr.REF_SHARE) + np.where(b["B"][k] > 0, 0.5 * np.spacing(np.abs(r["ll"])), 0.0)
        d = np.abs(v - r["ll"])
        ratio = np.where(bound > 0, d / np.where(bound > 0, bound, 1.0), np.where(d == 0, 0.0, np.inf))
        ratio = np.where(np.isfinite(v), ratio, np.inf)
        worst_ll = max(worst_ll, float(ratio.max())); bad_ll.append(np.nonzero(ratio > 1.0)[0])
        want = ch["posterior"][k]
        seen = want >= pr.OBSERVABLE
        ratio = (np.abs(p.astype(LD) - want) / (b["rel"][k] * np.where(seen, want, LD(1)))).astype(np.float64)
        ratio = np.where(seen, ratio, np.where((p >= 0) & (p < pr.UNOBSERVED_BELOW), 0.0, np.inf))
        ratio = np.where(np.isfinite(p), ratio, np.inf)
        worst_p = max(worst_p, float(ratio.max())); bad_p.append(np.nonzero(ratio > 1.0)[0])
    out = dict(ll=(worst_ll, np.unique(np.concatenate(bad_ll))), posterior=(worst_p, np.unique(np.concatenate(bad_p))))
    clear = ~b["in_band"]
    out["best"] = (int(clear.sum()), np.nonzero(clear & (np.asarray(got["best"]) != ch["best"]))[0])
    lo, hi = qual_range(ref, G)
    q = np.asarray(got["qual"], np.uint64)
    out["qual"] = (int(clear.sum()), np.nonzero(clear & ((q < lo) | (q > hi)))[0])
    out["qual_edges"] = int((clear & (lo != hi)).sum())
    return out


def ok(res):
    return all(res[k][1].size == 0 for k in ("ll", "posterior", "best", "qual"))


def describe(ref, got, res, n=4):
    lines = []
    for name in ("ll", "posterior", "best", "qual"):
        bad = res[name][1]
        if bad.size:
            i = bad[:n]
            lines.append(f"{name}: {bad.size} of {ref['N']} cells (worst / compared {res[name][0]}), first {i}: device "
                         f"{np.asarray(got[name])[..., i].tolist()}, entries {ref['count'][i]}, reference best {ref['chain']['best'][i]}")
    return "; ".join(lines)


# ---- sensitivity (what a wrong tally or a lost term would do) ------------------------------------------------------------------------
def drop_one_entry(ref, coo, G, k, j):
    """entry j of the COO (a cell of class k) left out of class k's tally: the largest |change of ll_k| over the cells with an
    entry at that locus, in units of the cell's bound"""
    lo, ce, al, re = (np.asarray(x, np.int64) for x in coo)
    l = lo[j]
    a, b = ref["ab"][k]
    s = ref["scale_used"][k]
    a2, b2 = (float(ref["alt"][k, l]) - al[j]) * s + 1.0, (float(ref["ref"][k, l]) - re[j]) * s + 1.0
    at = np.nonzero(lo == l)[0]
    if ref["mask"] is not None and not ref["mask"][l]:
        return 0.0
    t0, _, _ = tr.term_values(np.full(len(at), a[l]), np.full(len(at), b[l]), al[at], re[at])
    t1, _, _ = tr.term_values(np.full(len(at), a2), np.full(len(at), b2), al[at], re[at])
    delta = np.zeros(ref["N"], LD)
    np.add.at(delta, ce[at], t1 - t0)
    B = bounds(ref, G)["B"][k]
    with np.errstate(divide="ignore", invalid="ignore"):
        moved = np.where(delta != 0, np.abs(delta).astype(np.float64) / B, 0.0)
    return float(moved.max())


def drop_smallest_term(ref, G):
    """the denominator formed without its smallest live term: the largest relative change of a posterior, in units of its bound"""
    ch = ref["chain"]
    ks = [k for k in range(ref["K"]) if ref["live"][k]]
    if len(ks) < 2:
        return math.inf  # (nothing to lose: a single live class has posterior 1 by construction)
    b = bounds(ref, G)
    wmin = np.min(np.stack([ch["posterior"][k] for k in ks]), axis=0).astype(np.float64)
    change = wmin / (1.0 - wmin)  # every posterior grows by 1 / (1 - w_min)
    return float((change / b["rel"][ks].max(axis=0)).max())


# ---- the cases -----------------------------------------------------------------------------------------------------------------
K2_SETS = ("three", "planted", "every-second")  # exclusion sets of posterior_reference: class 0 = the set, class 1 = the rest
_cases, _sums = {}, {}


def reference_scales(n_excluded, n_cells):
    """scale and log priors that make K = 2 the reference's two-class posterior without the doublet term (main.rs:250-265), as the
    host computes them"""
    mf = max((n_excluded + 1.0) / (n_cells + 1.0), 0.01)
    return [1.0, mf], [math.log(mf), math.log(1.0 - mf)]


def case_mask(mname):
    L = pr.matrix(mname)[0]
    return (np.random.default_rng(4242 + L).random(L) < 0.8).astype(np.uint8)


def case_names(mname):
    """(K, which): K = 2 from the matrix' exclusion sets, K = 3 / 16 from a seeded draw with 5 % unlabelled"""
    return [(2, s) for s in K2_SETS] + [(3, "draw"), (16, "draw")]


def case_labels(mname, K, which):
    L, N, coo, _ = pr.matrix(mname)
    if which == "draw":
        rng = np.random.default_rng(100 * K + N)
        lab = rng.integers(0, K, N).astype(np.uint8)
        lab[rng.random(N) < 0.05] = UNLABELLED
        return lab, None, None
    exc = pr.exclusion_set(mname, which)
    scale, lp = reference_scales(int(exc.sum()), N)
    return np.where(exc, 0, 1).astype(np.uint8), scale, lp


def case(mname, K, which, masked):
    """the reference of a (matrix, labelling, mask) case, computed once per process"""
    key = (mname, K, which, bool(masked))
    if key not in _cases:
        L, N, coo, _ = pr.matrix(mname)
        lab, scale, lp = case_labels(mname, K, which)
        mask = case_mask(mname) if masked else None
        if (mname, bool(masked)) not in _sums:
            _sums[(mname, bool(masked))] = CellSums(N, coo, mask)
        ref = reference(L, N, coo, lab, K, scale, lp, mask, _sums[(mname, bool(masked))])
        ref["scale"], ref["log_prior"] = scale, lp
        _cases[key] = ref
    return _cases[key]


# the refine mixture: three genotypes, 900 cells x 600 loci, ~40 % density, totals 1 + Geometric, classes 70 / 20 / 10 %; per-locus
# allele fractions drawn from {0.02, 0.5, 0.98} independently per genotype
MIX_N, MIX_L = 900, 600
_mix = {}


def mixture(seed=5):
    if seed not in _mix:
        rng = np.random.default_rng(seed)
        truth = rng.choice(3, MIX_N, p=[0.7, 0.2, 0.1]).astype(np.uint8)
        af = rng.choice([0.02, 0.5, 0.98], (3, MIX_L))
        lo, ce = np.nonzero(rng.random((MIX_L, MIX_N)) < 0.4)
        tot = rng.geometric(0.7, len(lo))  # 1 + Geometric
        alt = rng.binomial(tot, af[truth[ce], lo])
        coo = [np.asarray(x, np.int64) for x in (lo, ce, alt, tot - alt)]
        # a few cells with a single entry each behind them (min_loci): cells MIX_N .. MIX_N + 5
        one = np.arange(6)
        coo = [np.concatenate([coo[0], 7 * one + 3]), np.concatenate([coo[1], MIX_N + one]), np.concatenate([coo[2], one % 2]),
               np.concatenate([coo[3], 1 - one % 2])]
        order = np.lexsort((coo[1], coo[0]))
        _mix[seed] = (MIX_L, MIX_N + 6, [x[order] for x in coo], np.concatenate([truth, np.arange(6, dtype=np.uint8) % 3]))
    return _mix[seed]


REFINE_STARTS = ("noisy", "empties")


def refine_start(which, seed=5):
    """(labels, K): the truth with 15 % of the labels reassigned at random and 5 % unlabelled; "empties": a fourth class of three
    cells on top, which they leave on the way"""
    L, N, coo, truth = mixture(seed)
    rng = np.random.default_rng(seed + 1)
    start = truth.copy()
    r = rng.random(N)
    start[r < 0.15] = rng.integers(0, 3, int((r < 0.15).sum()))
    start[r > 0.95] = UNLABELLED
    start[MIX_N:] = np.arange(6) % 3  # the one-entry cells stay labelled
    if which == "empties":
        start[rng.choice(MIX_N, 3, replace=False)] = 3
        return start, 4
    return start, 3


def ll_fn_80bit(N, coo):
    """the per-cell sums of tile_reference.cell_reference rounded to double, as classes.refine's ll function"""
    cache = {}

    def fn(alpha, beta, mask):
        key = None if mask is None else bytes(np.asarray(mask, np.uint8))
        if key not in cache:
            cache[key] = CellSums(N, coo, mask)
        r = cache[key](alpha, beta)
        return r["ll"], r["loci_used"]
    return fn


def g_any(L):
    """the largest number of partial sums either engine adds a cell's sum from, whatever the geometry"""
    return max(pr.WAVE_STEPS, pr.g_max(L, 8), pr.g_max(L, 6))
