"""High-precision reference of the posterior phase (calculate_posteriors, main.rs:228-280) and the device's error bound.

A plain helper for the tests (no fixtures, no GPU).  From a matrix in COO form and an exclusion set it forms

  * the three alpha / beta sets and the priors (mf0, lp_min, lp_maj, lp_dbl) in the reference's operation order, in numpy doubles
    (posterior_alpha_betas, priors: the library is built with -ffp-contract=off, so these are the device's bits);
  * the three per-cell sums in 80-bit longdouble (tile_reference.cell_reference, key ll_ld: the sum before it is rounded);
  * the chain of main.rs:266-278 in longdouble from those sums (chain):
        log_num = lp_min + s_min,  l1 = logsumexp(log_num, lp_maj + s_maj),  log_dbl = lp_dbl + s_dbl,  log_den = logsumexp(l1, log_dbl),
        x_p = log_num - log_den,   x_d = log_dbl - log_den,   posterior = exp(x_p),   doublet_posterior = exp(x_d).
    lp_maj = -inf (every cell excluded: log(1 - 1)) gives exp(-inf) = 0 in the first logsumexp and a finite chain; no warning is
    raised and nothing is turned into NaN.  Where np.longdouble is not the x87 format the chain is evaluated with mpmath.

The device's bound (u = 2^-53; csrc/kernels_tiled.hip k_posterior_finalize, csrc/kernels_em.hip k_posterior, csrc/device_math.h
dm_logsumexp; nothing here is fitted to observed errors)

  B_k      the bound of the sum of set k (tile_reference.cell_bound with G partial sums: for engine 1 the six steps of wave_sum,
           for engine 2 the chunk groups + the tier-2 tile set's groups + the overflow sum, for a ctx of logical shards the largest
           count a shard can have: g_max).
  e_k      = B_k + u |lp_k + s_k| + u |lp_k|: the sum's error, the rounding of the addition of the prior, and one unit of the prior
           itself (the host's std::log and numpy's log need not agree in the last bit).  lp_maj = -inf: the term is -inf on both
           sides, e_maj = 0.
  one logsumexp step  m + log(exp(x - m) + exp(y - m)),  m = max(x, y),  d = min - max <= 0:
           the errors of the two arguments, e_x + e_y (the derivatives of logsumexp are positive and add up to 1);
           the larger argument's exp(0) = 1 is exact; the smaller one's E = exp(d) carries the rounding of d, u |d|, and one ulp
           of exp (ROCm device-libs, ocml: "exp: 1 ulp", "log: 1 ulp" for double precision; one ulp is at most 2 u relative),
           and enters the sum S = 1 + E multiplied by E / S <= 1/2:  u |d| e^d <= 0.37 u  and  2 u / 2 = u;
           the addition 1 + E rounds once, u relative on S, i.e. absolute on its log;
           log(S) in [0, ln 2]: one ulp of it, at most 2 u ln 2 = 1.39 u;
           the addition m + log(S): u |result|.
           0.37 + 1 + 1 + 1.39 < C_LSE = 4 roundings of u, plus u |result|.
  E_den    = (e_min + e_maj + 4 u + u |l1|) + e_dbl + 4 u + u |log_den|
  rel(posterior)         <= e_min + E_den + u |x_p| + 2 u   (the subtraction's rounding; exp turns the absolute error of its
  rel(doublet_posterior) <= e_dbl + E_den + u |x_d| + 2 u    argument into a relative one, expm1 of it to be exact, and adds one ulp
                                                             of its own, which also covers the result's rounding).
  The reference repeats each of these operations at 2^-64 instead of 2^-53, i.e. with 2^-11 of the error, and its terms with about
  twice the operations (tile_reference.ref_ops): both bounds are widened by REF_SHARE = 2^-10 of themselves for it.

Rule of comparison (compare): a value whose reference is >= 1e-290 — a normal double — is held to the relative bound, against the
longdouble value (no rounding of the reference enters); a value whose reference is below must come out < 1e-280 and >= 0.  A
posterior that saturates at exactly 1.0 needs no special case under a relative bound.  ll_minority and ll_majority are held to
B_k and half an ulp of the reference's rounding to double, as tests/test_gpu_tile_sweep.py holds every sum.

The cases (matrix x exclusion set) of tests/test_gpu_posterior_sweep.py are named here, so that tests/test_posterior_reference.py
can show on the CPU that each of them lets the doublet set be seen (observability, sensitivity).
"""
import numpy as np

import tile_reference as tr

LD = np.longdouble
U = tr.U53
OBSERVABLE = 1e-290    # a reference value from here on is held to the relative bound
UNOBSERVED_BELOW = 1e-280  # what the device must stay below where the reference is not observable
C_LSE = 4.0            # roundings of u inside one logsumexp step (module docstring)
C_EXP = 2.0            # one ulp of exp as a relative error
REF_SHARE = 2.0 ** -10
WAVE_STEPS = 6         # engine 1: the partial sums of wave_sum
T_GROUPS_MAX = 64
BLU, T2_BLU = 639, {8: 338, 6: 767}
OUTPUTS = ("ll_minority", "ll_majority", "posterior", "doublet_posterior")


# ---- alpha / beta and the priors -----------------------------------------------------------------------------------------------
def priors(n_excluded, n_cells):
    """(mf0, lp_min, lp_maj, lp_dbl) of main.rs:240-265 as the host computes them (api_posteriors.cpp posterior_priors)"""
    mf0 = (n_excluded + 1.0) / (n_cells + 1.0)
    mf = max(mf0, 0.01)
    with np.errstate(divide="ignore"):  # every cell excluded: log(1 - 1) = -inf
        return mf0, float(np.log(mf)), float(np.log(1.0 - mf)), float(np.log(n_cells / 1000.0 / 100.0 * max(mf, 0.1)))


def posterior_alpha_betas(lc, alt_min, ref_min, n_excluded, n_cells):
    """The three alpha/beta sets of calculate_posteriors (main.rs:239-254) from the per-locus totals and the
    minority tallies, in the reference's operation order."""
    s_ref, s_alt = lc[:, 0], lc[:, 1]
    a_maj, b_maj = (s_alt + 1.0) - alt_min, (s_ref + 1.0) - ref_min
    a_min, b_min = (s_alt + 1.0) - (s_alt - alt_min), (s_ref + 1.0) - (s_ref - ref_min)
    mf0, lp_min, lp_maj, lp_dbl = priors(n_excluded, n_cells)
    a_dbl = (a_maj - 1.0) * mf0 + (a_min - 1.0) + 1.0
    b_dbl = (b_maj - 1.0) * mf0 + (b_min - 1.0) + 1.0
    mf = max(mf0, 0.01)
    a_maj, b_maj = (a_maj - 1.0) * mf + 1.0, (b_maj - 1.0) * mf + 1.0
    return (a_min, b_min), (a_maj, b_maj), (a_dbl, b_dbl), (lp_min, lp_maj, lp_dbl)


def tallies(L, coo, exc):
    """(locus_counts [L, 2] = (sum ref, sum alt), alt_min, ref_min) of the matrix and the set: whole numbers in doubles"""
    lo, ce, al, re = (np.asarray(x, np.int64) for x in coo)
    sel = np.asarray(exc, bool)[ce]
    lc = np.stack([np.bincount(lo, weights=re.astype(np.float64), minlength=L),
                   np.bincount(lo, weights=al.astype(np.float64), minlength=L)], axis=1)
    alt_min = np.bincount(lo[sel], weights=al[sel].astype(np.float64), minlength=L)
    ref_min = np.bincount(lo[sel], weights=re[sel].astype(np.float64), minlength=L)
    return lc, alt_min, ref_min


# ---- the chain -----------------------------------------------------------------------------------------------------------------
def _lse(a, b):
    m = np.maximum(a, b)
    return m + np.log(np.exp(a - m) + np.exp(b - m))


def _mpf(x):
    """a longdouble as an mpmath value, exactly"""
    import mpmath as mp
    mp.mp.dps = 50
    hi = float(x)
    if not np.isfinite(hi):
        return mp.mpf(hi)
    return mp.mpf(hi) + mp.mpf(float(LD(x) - LD(hi)))


def chain_mp(s_min, s_maj, s_dbl, lp):
    """the chain for one cell with mpmath at 50 digits: (x_p, x_d)"""
    import mpmath as mp
    mp.mp.dps = 50
    num = _mpf(lp[0]) + _mpf(s_min)
    dbl = _mpf(lp[2]) + _mpf(s_dbl)
    tot = mp.exp(num) + mp.exp(dbl)
    if np.isfinite(lp[1]):
        tot += mp.exp(_mpf(lp[1]) + _mpf(s_maj))
    den = mp.log(tot)
    return num - den, dbl - den


def chain(s, lp):
    """main.rs:266-278 in longdouble, per cell, from the three sums (longdouble arrays) and the three log priors"""
    s = [np.asarray(x, LD) for x in s]
    lpl = [LD(x) for x in lp]
    log_num, log_maj, log_dbl = lpl[0] + s[0], lpl[1] + s[1], lpl[2] + s[2]
    l1 = _lse(log_num, log_maj)
    den = _lse(l1, log_dbl)
    out = dict(log_num=log_num, log_maj=log_maj, log_dbl=log_dbl, l1=l1, den=den, x_p=log_num - den, x_d=log_dbl - den)
    if not tr.HAVE_X87:
        for i in range(len(s[0])):
            out["x_p"][i], out["x_d"][i] = (LD(float(v)) for v in chain_mp(s[0][i], s[1][i], s[2][i], lp))
    out["posterior"], out["doublet_posterior"] = np.exp(out["x_p"]), np.exp(out["x_d"])
    return out


def chain_double(s_min, s_maj, s_dbl, lp):
    """the device's own operations (k_posterior_finalize) in numpy doubles: (posterior, doublet_posterior).  What an honest
    double-precision evaluation gives; exp and log are numpy's, not the device's, so its last bits are not the device's."""
    s_min, s_maj, s_dbl = (np.asarray(x, np.float64) for x in (s_min, s_maj, s_dbl))
    log_num = lp[0] + s_min
    log_den = _lse(log_num, lp[1] + s_maj)
    log_dbl = lp[2] + s_dbl
    log_den = _lse(log_den, log_dbl)
    return np.exp(log_num - log_den), np.exp(log_dbl - log_den)


# ---- the reference of one (matrix, set) and its bound ----------------------------------------------------------------------------
def reference(L, N, coo, exc):
    """Everything the comparison needs for one matrix and one exclusion set (arrays per cell unless said otherwise)."""
    exc = np.asarray(exc, bool)
    lc, alt_min, ref_min = tallies(L, coo, exc)
    ab_min, ab_maj, ab_dbl, lp = posterior_alpha_betas(lc, alt_min, ref_min, int(exc.sum()), N)
    sums = []
    for k, (a, b) in enumerate((ab_min, ab_maj, ab_dbl)):
        r = tr.cell_reference(N, *coo, a, b)
        if k == 2:  # the smallest |term| of the cell's doublet terms (zero-total entries add exactly 0: not a term that can be lost)
            t = np.abs(r["term"])
            min_term = np.full(N, np.inf)
            np.minimum.at(min_term, np.asarray(coo[1], np.int64)[r["keep"]], np.where(t > 0, t, np.inf))
        sums.append({key: r[key] for key in ("ll", "ll_ld", "count", "abs_ll", "abs_ell", "b_ll", "b_ell")})
    ch = chain([r["ll_ld"] for r in sums], lp)
    return dict(N=N, L=L, excluded=exc, locus_counts=lc, ab=(ab_min, ab_maj, ab_dbl), lp=lp, mf0=priors(int(exc.sum()), N)[0],
                sums=sums, chain=ch, count=sums[0]["count"], min_term=min_term, _bounds={})


def _f64(x):
    return np.abs(x).astype(np.float64)


def bounds(ref, G):
    """dict: B (the three sums' bounds), rel_p, rel_d (relative bounds of the two posteriors) for G partial sums"""
    if G not in ref["_bounds"]:
        ch, lp = ref["chain"], ref["lp"]
        B = [tr.cell_bound(r, G)[0] for r in ref["sums"]]
        e = [B[k] + U * _f64(ch[name]) + U * abs(lp[k]) if np.isfinite(lp[k]) else np.zeros(ref["N"])
             for k, name in enumerate(("log_num", "log_maj", "log_dbl"))]
        e_den = (e[0] + e[1] + C_LSE * U + U * _f64(ch["l1"])) + e[2] + C_LSE * U + U * _f64(ch["den"])
        rel_p = (np.expm1(e[0] + e_den + U * _f64(ch["x_p"])) + C_EXP * U) * (1.0 + REF_SHARE)
        rel_d = (np.expm1(e[2] + e_den + U * _f64(ch["x_d"])) + C_EXP * U) * (1.0 + REF_SHARE)
        ref["_bounds"][G] = dict(B=B, rel_p=rel_p, rel_d=rel_d)
    return ref["_bounds"][G]


def compare(ref, got, G):
    """The four outputs of a posterior phase against the reference, every cell.  Returns {output: (worst observed / bound,
    indices of the cells beyond it)}; asserts nothing itself.  A cell whose sum has a zero bound (no entry, or zero-total entries
    only) must have that sum exactly."""
    b = bounds(ref, G)
    out = {}
    for name, k in (("ll_minority", 0), ("ll_majority", 1)):
        r = ref["sums"][k]
        bound = b["B"][k] * (1.0 + REF_SHARE) + np.where(b["B"][k] > 0, 0.5 * np.spacing(np.abs(r["ll"])), 0.0)
        v = np.asarray(got[name], np.float64)
        d = np.abs(v - r["ll"])
        ratio = np.where(bound > 0, d / np.where(bound > 0, bound, 1.0), np.where(d == 0, 0.0, np.inf))
        ratio = np.where(np.isfinite(v), ratio, np.inf)
        out[name] = (float(ratio.max()), np.nonzero(ratio > 1.0)[0])
    for name, rel in (("posterior", b["rel_p"]), ("doublet_posterior", b["rel_d"])):
        want = ref["chain"][name]
        v = np.asarray(got[name], np.float64)
        seen = want >= OBSERVABLE
        ratio = (np.abs(v.astype(LD) - want) / (rel * np.where(seen, want, LD(1)))).astype(np.float64)
        ratio = np.where(seen, ratio, np.where((v >= 0) & (v < UNOBSERVED_BELOW), 0.0, np.inf))
        ratio = np.where(np.isfinite(v), ratio, np.inf)
        out[name] = (float(ratio.max()), np.nonzero(ratio > 1.0)[0])
    return out


def describe(ref, got, res, G, n=4):
    """a failure message: the first cells beyond their bound, per output"""
    b = bounds(ref, G)
    lines = []
    for name, (worst, bad) in res.items():
        if bad.size:
            want = ref["chain"][name] if name in ref["chain"] else ref["sums"][OUTPUTS.index(name)]["ll"]
            bd = {"posterior": b["rel_p"], "doublet_posterior": b["rel_d"]}.get(name)
            lines.append(f"{name}: {bad.size} of {ref['N']} cells beyond the bound (worst {worst:.3g}), first {bad[:n]}: device "
                         f"{np.asarray(got[name])[bad[:n]]}, reference {np.asarray(want[bad[:n]], np.float64)}, entries "
                         f"{ref['count'][bad[:n]]}" + (f", relative bound {bd[bad[:n]]}" if bd is not None else ""))
    return "; ".join(lines)


def sensitivity(ref, G):
    """(cells, moved): the cells with a non-zero doublet term and an observable doublet_posterior, and by how many bounds the
    larger of the two posteriors' relative changes moves when s_dbl is shifted by the cell's smallest |term|"""
    b = bounds(ref, G)
    ch = ref["chain"]
    has = np.isfinite(ref["min_term"])
    s = [r["ll_ld"] for r in ref["sums"]]
    sh = chain([s[0], s[1], s[2] + np.where(has, ref["min_term"], 0.0).astype(LD)], ref["lp"])
    moved = np.maximum(np.abs(np.expm1((sh["x_p"] - ch["x_p"]).astype(np.float64))) / b["rel_p"],
                       np.abs(np.expm1((sh["x_d"] - ch["x_d"]).astype(np.float64))) / b["rel_d"])
    cells = has & (ch["doublet_posterior"] >= OBSERVABLE)
    return cells, moved


# ---- the cases -----------------------------------------------------------------------------------------------------------------
MATRICES = ("row-lengths", "tier2", "shallow-ragged", "second-trip")
SETS = ("empty", "three", "below-0.01", "above-0.01", "planted", "above-0.1", "every-second", "all-but-one", "all")
_matrices, _cases = {}, {}


def matrix(name):
    """(L, N, coo, planted): the builders of tests/test_gpu_tile_sweep.py; planted = the minority _two_populations drew"""
    if name not in _matrices:
        import test_gpu_tile_sweep as S
        if name == "row-lengths":
            (L, N, coo), seed = S._em_row_lengths(), 6
        elif name == "tier2":
            (L, N, coo), seed = S._em_tier2(), 12
        elif name == "shallow-ragged":
            L, N, seed = 3 * BLU - 17, 5 * 1024 + 1, 77
            coo = S._two_populations(S._random_coo(77, L, N, 130_000), N, L, seed=seed)
        elif name == "second-trip":
            N, L, coo = S._second_trip_coo()
            coo, seed = S._two_populations(coo, N, L, seed=3), 3
        else:
            raise KeyError(name)
        planted = np.random.default_rng(seed).random(N) < 0.07  # (_two_populations' first draw)
        _matrices[name] = (L, N, [np.asarray(x, np.int64) for x in coo], planted)
    return _matrices[name]


def set_names(mname):
    return ("planted",) if mname == "second-trip" else SETS


def exclusion_set(mname, sname):
    """Each set puts a clamp of main.rs:240-259 on an edge (mf0 = (n + 1) / (N + 1) against 0.01 and 0.1)."""
    L, N, coo, planted = matrix(mname)
    rng = np.random.default_rng(1009 * SETS.index(sname) + N)

    def pick(n):
        f = np.zeros(N, bool)
        f[rng.choice(N, n, replace=False)] = True
        return f

    below = max(n for n in range(N) if (n + 1.0) / (N + 1.0) < 0.01)  # the largest set still under the clamp
    if sname == "empty":
        return np.zeros(N, bool)
    if sname == "three":
        return np.isin(np.arange(N), [0, N // 3, N - 1])
    if sname == "below-0.01":
        return pick(below)
    if sname == "above-0.01":
        return pick(below + 1)
    if sname == "planted":
        return planted
    if sname == "above-0.1":
        return pick(int(0.12 * N))
    if sname == "every-second":
        return np.arange(N) % 2 == 0
    if sname == "all-but-one":
        return np.arange(N) != 7
    if sname == "all":
        return np.ones(N, bool)
    raise KeyError(sname)


def case(mname, sname):
    """the reference of a (matrix, set) case, computed once per process"""
    if (mname, sname) not in _cases:
        L, N, coo, _ = matrix(mname)
        _cases[(mname, sname)] = reference(L, N, coo, exclusion_set(mname, sname))
    return _cases[(mname, sname)]


def g_max(L, t2_tiles=0):
    """the largest number of partial sums any geometry of engine 2 gives a cell of a matrix of L loci: the chunk groups, the tier-2
    tile set's groups and the overflow sum (tests/test_gpu_tile_sweep.py _n_partials with groups at its cap)"""
    g2 = min(T_GROUPS_MAX, -(-L // T2_BLU[t2_tiles])) if t2_tiles in T2_BLU else 0
    return min(T_GROUPS_MAX, max(1, -(-L // BLU))) + g2 + 1
