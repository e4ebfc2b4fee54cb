"""80-bit reference of cellector_donor_genotypes (csrc/kernels_donor_genotypes.hip), the device's error bounds, and the cases the
CPU and the GPU tests share.

A plain helper for the tests (no fixtures, no GPU), independent of cellector_amd/donor_genotypes.py: it shares no code with the twin.
The model is stated once more here: integer tallies slot by slot, theta / w / v in double operation by operation (chains of IEEE
operations on doubles: the device's values ARE these), everything behind them in np.longdouble (u64 = 2^-64).

Bounds (u = 2^-53; nothing here is fitted to observed errors), per (donor, locus) with tallies (a, r):

  tab    la = log(double theta), lb = log(double (1.0 - theta)): C_LOG u |log| = one ulp of log as a relative error
         (donor_reference's tab bound; the same kernel operations).
  lam    from the DOUBLE tab the device returned: two rounded products and one rounded sum:
         B_lam = u (|a la| + |r lb|) + u |lam|.
  x      = lam + log(v), v a double formed as the header states it (four IEEE operations on doubles): the device's log is good to an
         ulp, the sum rounds once: B_x = B_lam + C_LOG u |log v| + u |x|.
  q      d_g = x_g - m rounds once and carries the errors of both operands: e_g = B_x[g] + max_j B_x[j] + u |d_g|; exp is good to an
         ulp: rel_g = expm1(e_g) + C_EXP u.  den adds at most 3 terms in order: rel_den = max_g rel_g + 3 u.  The division rounds
         once: rel(q_g) = (1 + rel_g) (1 + u) / (1 - rel_den) - 1.  A g with v_g == 0 has q_g = 0 exactly on every side.

The reference repeats the operations at 2^-64: every bound is widened by posterior_reference.REF_SHARE of itself for it, and a
comparison adds half an ulp of the double the reference is rounded to where it is compared as one.

Decisions.  gt_out is decided where the largest q is off gt_threshold by more than its bound and, if it is above, the runner-up is
further below it than the two bounds together.  kind follows from gt_out, the depth and prior_call (an argmax over doubles that every
side forms with the same IEEE operations): it is decided where gt_out is, or where the depth is 0.  With all three x_g equal (no
reads and a no-call row) every side has d_g = 0.0 and q_g = 1 / 3: the tie is structural and broken by the smaller g everywhere.
"""
import numpy as np

import posterior_reference as pr
import tile_reference as tr

LD = np.longdouble
U = tr.U53
C_EXP = pr.C_EXP
C_LOG = 2.0
NONE = 255
DEFAULTS = dict(err=0.01, ambient=0.03, gt_threshold=0.99, prior_floor=0.01)
F = 1.0 + pr.REF_SHARE


def params(**kw):
    p = dict(DEFAULTS)
    assert set(kw) <= set(p), kw
    p.update(kw)
    return p


# ---- step 1 ----------------------------------------------------------------------------------------------------------------------
def tally_reference(TL, coo, assign, D):
    """(cells [D + 1], alt, ref [D + 1, TL]) as plain integers, slot by slot (bincount weights are whole numbers far below 2^53)"""
    lo, ce, al, re = (np.asarray(x, np.int64) for x in coo)
    assign = np.asarray(assign, np.int64)
    slot = np.where(assign == NONE, D, assign)
    assert ((slot >= 0) & (slot <= D)).all()
    es = slot[ce]
    alt, ref = np.zeros((D + 1, TL), np.uint64), np.zeros((D + 1, TL), np.uint64)
    for s in range(D + 1):
        sel = es == s
        alt[s] = np.bincount(lo[sel], weights=al[sel], minlength=TL).astype(np.uint64)
        ref[s] = np.bincount(lo[sel], weights=re[sel], minlength=TL).astype(np.uint64)
    return np.array([(slot == s).sum() for s in range(D + 1)], np.uint64), alt, ref


# ---- step 2 ----------------------------------------------------------------------------------------------------------------------
def theta_double(alt, ref, err, ambient):
    """theta [TL, 3] in double, operation by operation as the header states it"""
    A = np.asarray(alt, np.uint64).sum(axis=0)
    T = A + np.asarray(ref, np.uint64).sum(axis=0)
    soup = (A.astype(np.float64) + 1.0) / (T.astype(np.float64) + 2.0)
    out = np.empty((len(A), 3))
    for g, e in enumerate((err, 0.5, 1.0 - err)):
        out[:, g] = ((1.0 - ambient) * e) + (ambient * soup)
    return out


def tab_reference(alt, ref, err=0.01, ambient=0.03):
    """(tab [TL, 3, 2] in longdouble from the double thetas, its bound)"""
    th = theta_double(alt, ref, err, ambient)
    tab = np.stack([np.log(th.astype(LD)), np.log((1.0 - th).astype(LD))], axis=-1)
    return tab, C_LOG * U * np.abs(tab).astype(np.float64) * F


def _ratio(got, want, bound):
    d = np.abs(np.asarray(got, np.float64).astype(LD) - want).astype(np.float64)
    bound = bound + np.where(bound > 0, 0.5 * np.spacing(np.abs(want.astype(np.float64))), 0.0)
    return float(np.where(bound > 0, d / np.where(bound > 0, bound, 1.0), np.where(d == 0, 0.0, np.inf)).max(initial=0.0))


def compare_tab(alt, ref, err, ambient, tab):
    want, bound = tab_reference(alt, ref, err, ambient)
    return _ratio(tab, want, bound)


# ---- steps 3 and 4 ---------------------------------------------------------------------------------------------------------------
def weights_double(prior, D, TL):
    """(w [D, TL, 3] double, prior_call [D, TL]) with the header's operations; None: every row a no-call"""
    w = np.full((D, TL, 3), 1.0 / 3.0)
    call = np.full((D, TL), 3, np.int64)
    if prior is None:
        return w, call
    p = np.asarray(prior, np.float32)
    assert p.shape == (D, TL, 3)
    for d in range(D):
        x = p[d].astype(np.float64)
        have = ~np.isnan(x).all(axis=1)
        s = (x[have, 0] + x[have, 1]) + x[have, 2]
        w[d, have] = x[have] / s[:, None]
        wd = w[d, have]
        best = np.zeros(len(wd), np.int64)
        for g in (1, 2):  # (the smallest g on ties: only a strictly larger weight moves it)
            best = np.where(wd[:, g] > wd[np.arange(len(wd)), best], g, best)
        call[d, have] = best
    return w, call


def reference(alt, ref, tab, prior=None, **kw):
    """q of every (donor, locus) in longdouble from the planes and DOUBLE tables (the device's, or the twin's), with the bounds of the
    module docstring.  Returns a dict (values longdouble, bounds double)."""
    prm = params(**kw)
    alt, ref = np.asarray(alt, np.uint64), np.asarray(ref, np.uint64)
    D, TL = alt.shape[0] - 1, alt.shape[1]
    w, prior_call = weights_double(prior, D, TL)
    pf = float(prm["prior_floor"])
    v = ((1.0 - pf) * w) + (pf / 3.0)
    part = v != 0.0
    t = np.asarray(tab, np.float64).astype(LD)
    a, r = alt[:D].astype(LD)[..., None], ref[:D].astype(LD)[..., None]
    pa, pb = a * t[None, :, :, 0], r * t[None, :, :, 1]
    lam = pa + pb
    fin = lambda z: np.abs(np.where(np.isfinite(z), z, 0)).astype(np.float64)
    B_lam = U * (fin(pa) + fin(pb)) + U * fin(lam)
    lv = np.log(np.where(part, v, 1.0).astype(LD))
    x = np.where(part, lam + lv, -np.inf)
    B_x = np.where(part, B_lam + C_LOG * U * fin(lv) + U * fin(x), 0.0)
    m = x.max(axis=2)
    d = x - m[..., None]
    ex = np.where(part, np.exp(d), 0)
    den = ex.sum(axis=2)
    q = ex / den[..., None]
    e = B_x + B_x.max(axis=2)[..., None] + U * fin(d)
    rel_g = np.where(part, np.expm1(e) + C_EXP * U, 0.0)
    rel_den = rel_g.max(axis=2) + 3 * U
    rel_q = np.where(part, ((1.0 + rel_g) * (1.0 + U) / (1.0 - rel_den[..., None]) - 1.0) * F, 0.0)
    # decisions
    qf = q.astype(np.float64)
    call = np.zeros((D, TL), np.int64)
    for g in (1, 2):
        call = np.where(q[..., g] > np.take_along_axis(q, call[..., None], 2)[..., 0], g, call)
    top = np.take_along_axis(qf, call[..., None], 2)[..., 0]
    top_rel = np.take_along_axis(rel_q, call[..., None], 2)[..., 0]
    thr = float(prm["gt_threshold"])
    gt_out = np.where(np.take_along_axis(q, call[..., None], 2)[..., 0] > thr, call, 3)
    B_top = top_rel * top + np.spacing(thr)
    off_thr = np.abs(top - thr) > B_top
    others = np.where(np.arange(3)[None, None, :] == call[..., None], -np.inf, qf)
    runner = others.max(axis=2)
    runner_B = np.where(np.arange(3)[None, None, :] == call[..., None], 0.0, rel_q * qf).max(axis=2)
    clear = (top - runner) > (top_rel * top + runner_B)
    depth = alt[:D] + ref[:D]
    gt_ok = off_thr & ((top < thr) | clear)
    kind = np.where(depth == 0, 0, np.where(gt_out == 3, 4, np.where(prior_call == 3, 2, np.where(gt_out == prior_call, 1, 3))))
    return dict(q=q, rel_q=rel_q, lam=lam, B_lam=B_lam * F, x=x, B_x=B_x * F, w=w, v=v, prior_call=prior_call, gt_out=gt_out.astype(np.uint8),
                kind=kind.astype(np.uint8), gt_ok=gt_ok, kind_ok=gt_ok | (depth == 0), depth=depth)


def _rel_ratio(got, want, rel):
    got = np.asarray(got, np.float64)
    seen = want >= pr.OBSERVABLE
    ratio = (np.abs(got.astype(LD) - want) / np.where(seen & (rel > 0), rel * np.where(seen, want, LD(1)), LD(1))).astype(np.float64)
    ratio = np.where(seen & (rel > 0), ratio, np.where(seen, np.where(got == want.astype(np.float64), 0.0, np.inf), 0.0))
    ratio = np.where(seen, ratio, np.where((got >= 0) & (got < pr.UNOBSERVED_BELOW), 0.0, np.inf))
    return float(np.where(np.isfinite(got), ratio, np.inf).max(initial=0.0))


def compare(ref, got):
    """got: the dict of Cellector.donor_genotypes (or the twin's).  Returns ({name: worst observed / bound}, undecided [D, TL] bool):
    q against its bound; gt_out and kind on the decided sites (inf = a difference there)."""
    out = dict(q=_rel_ratio(got["q"], ref["q"], ref["rel_q"]))
    s = np.asarray(got["q"], np.float64).sum(axis=2)
    out["q_sum"] = float((np.abs(s - 1.0) / (ref["rel_q"].max(axis=2) + 3 * U)).max(initial=0.0))
    for name, okname in (("gt_out", "gt_ok"), ("kind", "kind_ok")):
        dec = ref[okname]
        out[name] = 0.0 if np.array_equal(np.asarray(got[name])[dec], ref[name][dec]) else np.inf
    return out, ~ref["kind_ok"]


def site_mp(a, r, la, lb, v):
    """q [3] of one site with mpmath at 50 digits from double la, lb [3] and v [3]"""
    mp = tr._mp()
    x = [None if vg == 0.0 else int(a) * mp.mpf(float(l1)) + int(r) * mp.mpf(float(l2)) + mp.log(mp.mpf(float(vg)))
         for l1, l2, vg in zip(la, lb, v)]
    m = max(z for z in x if z is not None)
    e = [mp.mpf(0) if z is None else mp.exp(z - m) for z in x]
    return [z / sum(e) for z in e]


# ---- the cases -------------------------------------------------------------------------------------------------------------------
DONORS = (1, 2, 33, 64)
PRIORS = ("null", "onehot", "soft")
_case = {}


def case_assign(D, N, seed=0):
    """a draw over the D donors with 15 % of the cells at 255; with D >= 2 the last donor has no cell"""
    rng = np.random.default_rng(500 * D + seed)
    a = rng.integers(0, max(D - 1, 1), N).astype(np.uint8)
    a[rng.random(N) < 0.15] = NONE
    a[0] = 0
    return a


def case_prior(D, TL, kind, seed=0):
    """None; one-hot rows with a tenth blanked; or soft rows (Dirichlet draws, unnormalised, some with a zero weight, a tenth blanked,
    every 7th row one-hot)"""
    if kind == "null":
        return None
    rng = np.random.default_rng(77 * D + TL + seed)
    if kind == "onehot":
        g = rng.choice(3, (D, TL), p=[0.45, 0.3, 0.25])
        p = (g[..., None] == np.arange(3)).astype(np.float32)
    else:
        p = (rng.dirichlet([0.4, 0.4, 0.4], (D, TL)) * rng.choice([1.0, 0.5, 100.0], (D, TL, 1))).astype(np.float32)
        p[rng.random((D, TL)) < 0.15, 0] = 0.0
        p[:, ::7] = np.array([0, 2.5, 0], np.float32)
        p[(p == 0).all(axis=2)] = np.array([1, 0, 0], np.float32)
    p[rng.random((D, TL)) < 0.1] = np.nan
    return np.ascontiguousarray(p)


def edge_matrix():
    """(TL, N, coo) for the GPU tests, locus-major, 600 loci x 900 cells, on the tally kernel's edges (a block takes 4096 entries; its
    window holds 2047 loci at D = 1 and 63 at D = 64):
      locus 0         every cell five times over (4500 entries, the pair (0, c) listed five times): it straddles the first block edge;
                      300 of the entries carry alt = ref = 65535
      loci 1 .. 99    45 entries each at random cells, counts 0 .. 12 with alt = ref = 0 lines among them: the used loci
      loci 100 .. 599 one entry each: a run of 500 single-entry loci, longer than the window for D >= 31; they fail min_alt / min_ref
                      = 4 but hold reads (loci 300 .. 309 hold none: a line of 0, 0)"""
    if "edge" not in _case:
        rng = np.random.default_rng(61)
        N, TL = 900, 600
        lo = [np.zeros(4500, np.int64)]
        ce = [np.tile(np.arange(N), 5)]
        al, re = [rng.integers(0, 4, 4500)], [rng.integers(0, 4, 4500)]
        big = rng.choice(4500, 300, replace=False)
        al[0][big], re[0][big] = 65535, 65535
        for l in range(1, 100):
            lo.append(np.full(45, l)); ce.append(np.sort(rng.choice(N, 45, replace=False)))
            tot = rng.integers(0, 13, 45)
            a = rng.binomial(tot, rng.choice([0.02, 0.5, 0.98], 45))
            al.append(a); re.append(tot - a)
        lo.append(np.arange(100, 600)); ce.append(rng.integers(0, N, 500))
        a1, r1 = rng.integers(0, 3, 500), rng.integers(0, 3, 500)
        a1[200:210], r1[200:210] = 0, 0
        al.append(a1); re.append(r1)
        _case["edge"] = (TL, N, [np.concatenate(x).astype(np.int64) for x in (lo, ce, al, re)])
    return _case["edge"]


def edge_assign(D, N=900, mode="draw"):
    if mode == "none":
        return np.full(N, NONE, np.uint8)
    return case_assign(D, N, seed=3)


def called_matrix(D, seed=0):
    """(TL, N, coo, assign, truth gt [D, TL]) a pool of D donors with planted genotypes: 320 loci x 40 D (at most 640) cells, every
    cell a singlet of donor c % D reading 12 % of the loci at depth 1 + Poisson(1.5); every 9th cell assigned 255.  For the q /
    gt_out / kind comparisons: depth per (donor, locus) around 10 reads, so calls, withdrawals and no-read sites all occur."""
    key = ("called", D, seed)
    if key not in _case:
        rng = np.random.default_rng(900 + D + seed)
        TL, N = 320, min(40 * D, 640)
        gt = rng.choice(3, (D, TL), p=[0.5, 0.3, 0.2])
        donor = np.arange(N) % D
        lo, ce, al, re = [], [], [], []
        for c in range(N):
            l = np.sort(rng.choice(TL, int(0.12 * TL), replace=False))
            tot = 1 + rng.poisson(1.5, len(l))
            th = 0.97 * np.array([0.01, 0.5, 0.99])[gt[donor[c], l]] + 0.03 * 0.4
            a = rng.binomial(tot, th)
            lo.append(l); ce.append(np.full(len(l), c)); al.append(a); re.append(tot - a)
        lo, ce, al, re = (np.concatenate(x).astype(np.int64) for x in (lo, ce, al, re))
        o = np.argsort(lo, kind="stable")
        assign = donor.astype(np.uint8)
        assign[::9] = NONE
        _case[key] = (TL, N, [x[o] for x in (lo, ce, al, re)], assign, gt.astype(np.uint8))
    return _case[key]


def prior_of(gt, kind, seed=0):
    """the three priors of a truth gt [D, TL]: None; its one-hot with 10 % blanked and 5 % flipped; soft rows that lean to it"""
    if kind == "null":
        return None
    gt = np.asarray(gt)
    rng = np.random.default_rng(31 + seed + gt.shape[0])
    g = np.where(rng.random(gt.shape) < 0.05, (gt + 1 + rng.integers(0, 2, gt.shape)) % 3, gt)
    p = (g[..., None] == np.arange(3)).astype(np.float32)
    if kind == "soft":
        p = (0.7 * p + 0.3 * rng.dirichlet([1.0, 1.0, 1.0], gt.shape)).astype(np.float32) * np.float32(3.0)
        p[:, ::5, 2] = 0.0
    p[rng.random(gt.shape) < 0.1] = np.nan
    return np.ascontiguousarray(p, np.float32)


# ---- the planted pools -----------------------------------------------------------------------------------------------------------
FLIP = 0.05


def planted(seed):
    """donor_reference.planted_pool(seed) with its blanking undone and redone on purpose: returns a dict of L, N, coo, truth_cell [N]
    (255: a doublet), full [4, L] (the pool's calls before any blanking; donor 3 is the decoy without cells), gt [4, L] (the pool's:
    10 % blanked), damaged [4, L] (gt with FLIP of the remaining calls of the three real donors moved to another genotype), blanked
    and flipped [4, L] bool.  The blanking is the pool's own draw, repeated here and checked against it."""
    key = ("planted", seed)
    if key not in _case:
        import class_doublet_reference as cdr
        import donor_reference as dr
        from cellector_amd import genotypes as gtw
        L, N, coo, gt, truth, par = dr.planted_pool(seed)
        _, alt, ref = gtw.class_genotype_tallies(L, coo, cdr.doublet_mixture(0.0, seed)[3], 3)
        called, _, _ = gtw.genotype_posteriors(alt, ref)
        full = np.array([3, 2, 1, 0], np.uint8)[called]
        rng = np.random.default_rng(seed + 41)
        full = np.concatenate([full, rng.choice(3, (1, L)).astype(np.uint8)])
        blanked = rng.random(full.shape) < 0.1
        assert np.array_equal(np.where(blanked, 3, full), gt), "the pool's blanking is not the one repeated here"
        blanked &= full != 3
        rng = np.random.default_rng(seed + 97)
        flipped = (rng.random(gt.shape) < FLIP) & (gt != 3)
        flipped[3] = False
        damaged = np.where(flipped, (gt + 1 + rng.integers(0, 2, gt.shape)) % 3, gt).astype(np.uint8)
        _case[key] = dict(L=L, N=N, coo=coo, truth_cell=truth, parents=par, full=full, gt=gt, damaged=damaged, blanked=blanked,
                          flipped=flipped)
    return _case[key]


def onehot(gt):
    """prior [D, TL, 3] float32 of hard calls, three NaN for code 3 (stated here on its own, not the twin's helper)"""
    gt = np.asarray(gt)
    p = (gt[..., None] == np.arange(3)).astype(np.float32)
    p[gt == 3] = np.nan
    return p
