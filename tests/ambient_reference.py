"""80-bit reference of the ambient calls (cellector_ambient_tables / cellector_ambient_profile / cellector_estimate_ambient;
csrc/kernels_ambient.hip), the device's error bounds, the cases the CPU and the GPU tests share and the planted-ambient generator.

A plain helper for the tests (no fixtures, no GPU), independent of cellector_amd/ambient.py: it shares no code with the twin.  The
model is stated once more here, in np.longdouble (u64 = 2^-64).  S sources with genotypes gt [S, L] (0 = 0/0, 1 = 0/1, 2 = 1/1, 3 = no
call), a cell c scored under source assign[c] (255: it takes no part), a grid rho [G]:

  theta_{l,g,j} = ((1 - rho_j) e_g) + (rho_j soup_l),  e = (err, 0.5, 1 - err, soup_l),  soup_l = (A_l + 1) / ((A_l + R_l) + 2)
  tab[l][g][j]  = (log theta, log(1 - theta)), (0, 0) at a masked locus
  ll[c][j]      = the sum over the cell's entries at unmasked loci of alt tab[l][g][j][0] + ref tab[l][g][j][1], g = gt[assign[c], l]
  total[j]      = the sum of ll[c][j] over the cells that take part;  source_total[s][j] = over the cells of source s
  vertex rule   j* = the smallest argmax of y over the grid, jj = min(max(j*, 1), G - 2), the parabola through the three points at
                jj - 1, jj, jj + 1: curvature c = 2 (d1 - d0) / (h0 + h1), d0 = (y1 - y0) / h0, d1 = (y2 - y1) / h1, and c = 0 where
                neither step is resolved (|y1 - y0| and |y2 - y1| both <= 2^-40 |y1|: rounding, not signal); c < 0: rho =
                (x0 + x1) / 2 - d0 / c clamped into [x0, x2], se = 1 / sqrt(-c); else rho = rho[j*], se = +inf
  estimate      round r: the grid of G points over [lo_r, hi_r] (made in double, as the library makes it: the grid is an input of the
                round), j* of total, lo_{r+1}, hi_{r+1} = rho[max(j* - 1, 0)], rho[min(j* + 1, G - 1)]; after the last round the
                vertex rule on total, rho clamped into the parameters' [lo, hi]

Bounds (u = 2^-53; nothing here is fitted to observed errors).  n = the entries of the cell at used, unmasked loci.

  tab    theta is a chain of IEEE operations on doubles (whole-number totals, err, rho_j): the device's theta IS the double theta
         formed here in double, so tab = log(double theta) and log(double (1.0 - theta)) are held to C_LOG u |log| = one ulp of log
         as a relative error (ROCm device-libs documents 1 ulp for the f64 log; donor_reference's tab bound).
  ll     the sums of doubles (the tables the device returned): B = (n + 1) u sum (|alt la| + |ref lb|), as donor_reference's B_s.
  fold   a value passes through at most ceil(N / 256) adds in its thread's chain and 8 more in the pairwise fold of the 256 partial
         sums: B_total = sum_c B_ll[c] + (ceil(N / 256) + 8) u sum_c |ll[c]|; a source's fold likewise over its own cells.

The reference repeats the operations at 2^-64: every bound is widened by posterior_reference.REF_SHARE of itself for it, and a
comparison adds half an ulp of the double the reference is rounded to.

The per-cell and pooled rho of the vertex rule are quotients of differences of nearly equal sums: they are compared with the twin bit
for bit (tests/test_gpu_ambient.py), not with this reference.  The reference's own estimate is what the recovery test holds to the
planted rho.
"""
import math

import numpy as np

import donor_reference as dr

LD = np.longdouble
U = dr.U
C_LOG = dr.C_LOG
F = dr.F
NONE = 255
DEFAULTS = dict(err=0.01, lo=0.0, hi=0.5, grid=16, rounds=3, min_loci=1)
FOLD_THREADS = 256
FLAT = LD(2) ** -40


def params(**kw):
    p = dict(DEFAULTS)
    assert set(kw) <= set(p), kw
    p.update(kw)
    return p


# ---- tables ----------------------------------------------------------------------------------------------------------------------
def theta_double(A, R, rho, err):
    """theta [L, 4, G] in double, operation by operation as the header states it"""
    A, R = np.asarray(A, np.float64), np.asarray(R, np.float64)
    soup = (A + 1.0) / ((A + R) + 2.0)
    out = np.empty((len(A), 4, len(rho)))
    for j, r in enumerate(np.asarray(rho, np.float64)):
        for g, e in enumerate((err, 0.5, 1.0 - err, None)):
            out[:, g, j] = ((1.0 - r) * (soup if e is None else e)) + (r * soup)
    return out


def tab_reference(A, R, rho, err=0.01, mask=None):
    """(tab [L, 4, G, 2] in longdouble from the double thetas, its bound)"""
    th = theta_double(A, R, rho, err)
    tab = np.stack([np.log(th.astype(LD)), np.log((1.0 - th).astype(LD))], axis=-1)
    if mask is not None:
        tab[np.asarray(mask) == 0] = 0
    return tab, C_LOG * U * np.abs(tab).astype(np.float64) * F


def compare_tab(A, R, rho, err, mask, tab):
    want, B = tab_reference(A, R, rho, err, mask)
    return dr._ratio(tab, want, B)


# ---- cell sums and folds ---------------------------------------------------------------------------------------------------------
def cell_reference(N, coo, gt_used, assign, tab, mask=None):
    """The cell sums in longdouble from a DOUBLE table tab [L, 4, G, 2] (the device's, or the twin's): dict of ll [N, G], B_ll,
    n_entries.  Also rows: the entries in row order (locus, cell, alt, ref, genotype) for the wrong-row test."""
    gt_used, assign = np.asarray(gt_used, np.int64), np.asarray(assign, np.int64)
    lo, ce, al, re = dr._rows(coo, mask)
    part = assign[ce] != NONE
    lo, ce, al, re = lo[part], ce[part], al[part], re[part]
    g = gt_used[assign[ce], lo]
    t = np.asarray(tab, np.float64).astype(LD)[lo, g]  # [m, G, 2]
    pa, pb = al.astype(LD)[:, None] * t[:, :, 0], re.astype(LD)[:, None] * t[:, :, 1]
    ll, cnt = dr._seg_sum(ce, pa + pb, N)
    mag, _ = dr._seg_sum(ce, np.abs(pa) + np.abs(pb), N)
    return dict(ll=ll, B_ll=(cnt[:, None] + 1.0) * U * mag.astype(np.float64) * F, n_entries=cnt, rows=(lo, ce, al, re, g))


def fold_reference(ll, B_ll, assign, S):
    """dict of total [G], source_total [S, G] in longdouble, their bounds and source_cells from the reference's cell sums"""
    assign = np.asarray(assign, np.int64)
    depth = (math.ceil(len(assign) / FOLD_THREADS) + 8) * U

    def one(member):
        t = ll[member].sum(axis=0)
        B = B_ll[member].sum(axis=0) + depth * np.abs(ll[member]).sum(axis=0).astype(np.float64) * F
        return t, B

    total, B_total = one(assign != NONE)
    src = [one(assign == s) for s in range(S)]
    return dict(total=total, B_total=B_total, source_total=np.stack([s[0] for s in src]), B_source=np.stack([s[1] for s in src]),
                source_cells=np.array([(assign == s).sum() for s in range(S)], np.uint64))


def compare(N, coo, gt_used, assign, mask, got):
    """got: the dict of Cellector.ambient_profile with tables (or the twin's).  Returns {name: worst observed / bound}."""
    ref = cell_reference(N, coo, gt_used, assign, got["tab"], mask)
    fr = fold_reference(ref["ll"], ref["B_ll"], assign, np.asarray(gt_used).shape[0])
    return dict(ll=dr._ratio(got["ll"], ref["ll"], ref["B_ll"]), total=dr._ratio(got["total"], fr["total"], fr["B_total"]),
                source_total=dr._ratio(got["source_total"], fr["source_total"], fr["B_source"]),
                n_entries=0.0 if np.array_equal(np.asarray(got["n_entries"]).astype(np.int64), ref["n_entries"]) else np.inf,
                source_cells=0.0 if np.array_equal(np.asarray(got["source_cells"]), fr["source_cells"]) else np.inf), ref


# ---- the vertex rule and the estimate ---------------------------------------------------------------------------------------------
def vertex_reference(rho, y):
    """(j*, rho, se, curvature) of one profile y [G] in longdouble"""
    rho, y = np.asarray(rho, np.float64).astype(LD), np.asarray(y).astype(LD)
    G = len(y)
    js = int(np.argmax(y))
    jj = min(max(js, 1), G - 2)
    x0, x1, x2 = rho[jj - 1:jj + 2]
    y0, y1, y2 = y[jj - 1:jj + 2]
    h0, h1 = x1 - x0, x2 - x1
    d0, d1 = (y1 - y0) / h0, (y2 - y1) / h1
    lim = FLAT * abs(y1)
    c = 2 * (d1 - d0) / (h0 + h1) if abs(y1 - y0) > lim or abs(y2 - y1) > lim else LD(0)
    if c < 0:
        v = (x0 + x1) / 2 - d0 / c
        return js, float(min(max(v, x0), x2)), float(1 / np.sqrt(-c)), float(c)
    return js, float(rho[js]), math.inf, float(c)


def estimate_reference(L, N, coo, gt_used, assign, mask=None, **kw):
    """cellector_estimate_ambient in longdouble: dict of rho, se, curvature, at_boundary, lo, hi, j_star, source_rho, source_se,
    source_cells and, per round, grids and totals (for the concavity check)"""
    prm = params(**kw)
    G, S = int(prm["grid"]), np.asarray(gt_used).shape[0]
    A, R = dr.totals(L, coo)
    lo, hi = float(prm["lo"]), float(prm["hi"])
    grids, totals = [], []
    for rnd in range(int(prm["rounds"])):
        if rnd:
            js = int(np.argmax(fr["total"]))
            lo, hi = float(rho[max(js - 1, 0)]), float(rho[min(js + 1, G - 1)])
        step = (hi - lo) / float(G - 1)
        rho = np.array([lo + (float(j) * step) for j in range(G)])
        th = theta_double(A, R, rho, prm["err"])
        tab = np.stack([np.log(th.astype(LD)), np.log((1.0 - th).astype(LD))], axis=-1)
        if mask is not None:
            tab[np.asarray(mask) == 0] = 0
        # (the sums from the longdouble table itself: no rounding of the logarithms to double in between)
        lo_, ce, al, re = dr._rows(coo, mask)
        a = np.asarray(assign, np.int64)
        part = a[ce] != NONE
        lo_, ce, al, re = lo_[part], ce[part], al[part], re[part]
        t = tab[lo_, np.asarray(gt_used, np.int64)[a[ce], lo_]]
        ll, _ = dr._seg_sum(ce, al.astype(LD)[:, None] * t[:, :, 0] + re.astype(LD)[:, None] * t[:, :, 1], N)
        fr = fold_reference(ll, np.zeros(ll.shape), assign, S)
        grids.append(rho); totals.append(fr["total"])
    clamp = lambda x: min(max(x, float(prm["lo"])), float(prm["hi"]))
    js, est, se, c = vertex_reference(rho, fr["total"])
    est = clamp(est)
    src = [vertex_reference(rho, fr["source_total"][s]) if fr["source_cells"][s] else (0, math.nan, math.nan, math.nan) for s in range(S)]
    return dict(rho=est, se=se, curvature=c, j_star=js, lo=lo, hi=hi, at_boundary=int(est <= prm["lo"] or est >= prm["hi"]),
                source_rho=np.array([clamp(s[1]) if s[1] == s[1] else math.nan for s in src]), source_se=np.array([s[2] for s in src]),
                source_curvature=np.array([s[3] for s in src]), source_j=np.array([s[0] for s in src]),
                source_cells=fr["source_cells"], grids=grids, totals=totals, source_total=fr["source_total"])


# ---- the cases -------------------------------------------------------------------------------------------------------------------
GRIDS = (4, 5, 8, 15, 16, 17, 32)   # every lanes-per-cell width of the cell pass (4, 8, 16, 32) and both sides of each
SOURCES = (1, 3, 33, 64)            # one and two packed words


def case_grid(G):
    """a uniform grid over [0, 0.5], made as the library makes it"""
    step = (0.5 - 0.0) / float(G - 1)
    return np.array([0.0 + (float(j) * step) for j in range(G)])


def case_grid_uneven(G=9):
    """a caller's grid: ascending, unequal steps, 0 and a value close to 1 included"""
    return np.array([0.0, 0.001, 0.01, 0.03, 0.05, 0.1, 0.3, 0.7, 0.97][:G])


def case_assign(S, kind="mixed", N=dr.CASE_N):
    """mixed: cell c under source (c mod S), every 7th cell 255; hole: as mixed with source S // 2 emptied (S >= 2); none: all 255"""
    a = (np.arange(N) % S).astype(np.uint8)
    a[::7] = NONE
    if kind == "hole" and S >= 2:
        a[a == S // 2] = NONE
    if kind == "none":
        a[:] = NONE
    return a


# ---- the planted pool ------------------------------------------------------------------------------------------------------------
PLANT_N, PLANT_L = 300, 400
PLANT_RHOS = (0.0, 0.03, 0.08, 0.2)
PLANT_SEEDS = (0, 1, 2, 3)
_plant = {}


def planted(rho, seed, err=0.01):
    """(L, N, coo, gt [3, L], assign [N]): 300 cells x 400 loci; 3 donors at 60 / 30 / 10 % of the cells; genotypes 0 / 1 / 2 at 0.5 /
    0.3 / 0.2; a (locus, cell) entry with probability 0.3; depth 1 + Poisson(1); alt ~ Binomial(depth, (1 - rho) e_g + rho soup_true),
    soup_true = the pool's allele fraction at the locus (the donors' e_g weighted by their shares)"""
    key = (rho, seed)
    if key not in _plant:
        rng = np.random.default_rng(1000 * seed + int(round(rho * 1000)) + 17)
        N, L = PLANT_N, PLANT_L
        share = np.array([0.6, 0.3, 0.1])
        donor = np.repeat(np.arange(3), (share * N).astype(int))
        assert len(donor) == N
        gt = rng.choice(3, (3, L), p=[0.5, 0.3, 0.2]).astype(np.uint8)
        e = np.array([err, 0.5, 1.0 - err])[gt]  # [3, L]
        soup = (share[:, None] * e).sum(axis=0)
        have = rng.random((L, N)) < 0.3
        lo, ce = np.nonzero(have)
        depth = 1 + rng.poisson(1.0, len(lo))
        p = (1.0 - rho) * e[donor[ce], lo] + rho * soup[lo]
        al = rng.binomial(depth, p)
        _plant[key] = (L, N, [lo.astype(np.int64), ce.astype(np.int64), al.astype(np.int64), (depth - al).astype(np.int64)], gt,
                       donor.astype(np.uint8))
    return _plant[key]
