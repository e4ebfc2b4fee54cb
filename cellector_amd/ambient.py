"""Ambient fraction estimation on host arrays: the numpy twin of cellector_ambient_tables / cellector_ambient_profile /
cellector_estimate_ambient (include/cellector_ffi.h states the model; csrc/kernels_ambient.hip runs it).

Every cell is scored under the genotypes of the source it is assigned to at G ambient fractions rho at once; the sums are added
over the cells; the maximum of that profile, found on a grid that zooms in, is the estimate, and the parabola through the last
three points gives its standard error.

The sums are the library's sums in the library's order (a cell's entries in by-cell CSR row order, the cells in the order of the
256-thread fold, one rounded product and one rounded add at a time): fed the DEVICE's tables, cell_sums, fold, the vertex rule's
rho and every field of estimate's summary but the se fields carry the device's bits.  The se fields pass through a square root and
agree to an ulp or two.  log is numpy's, not the device's: the tables made here agree with the device's to a few ulps.
"""
import numpy as np

from .cluster import OBJ_THREADS, Matrix  # noqa: F401  (the matrix in the library's row order; callers build one and pass it in)

NONE = 255
DEFAULTS = dict(err=0.01, lo=0.0, hi=0.5, grid=16, rounds=3, min_loci=1)
FLAT = 2.0 ** -40  # two steps of a profile that both stay within this share of its value are rounding, not signal (AM_FLAT)


def _params(params):
    p = dict(DEFAULTS)
    for k, v in params.items():
        if k not in p:
            raise TypeError(f"unknown parameter {k!r}")
        p[k] = v
    return p


def grid(lo, hi, G):
    """rho [G]: lo + ((double)j ((hi - lo) / (double)(G - 1)))"""
    step = (float(hi) - float(lo)) / float(G - 1)
    return float(lo) + (np.arange(G, dtype=np.float64) * step)


def tables(alt_total, ref_total, rho, err=0.01, mask=None, log=np.log):
    """tab [L, 4, G, 2] = (log theta, log(1 - theta)), theta = ((1 - rho_j) e_g) + (rho_j soup), e = (err, 0.5, 1 - err, soup), soup =
    (A + 1) / ((A + R) + 2); a masked locus carries (0, 0)"""
    A, R = np.asarray(alt_total, np.float64), np.asarray(ref_total, np.float64)
    rho = np.asarray(rho, np.float64)
    soup = (A + 1.0) / ((A + R) + 2.0)
    e = np.stack([np.full_like(soup, err), np.full_like(soup, 0.5), np.full_like(soup, 1.0 - err), soup], axis=1)  # [L, 4]
    keep, amb = 1.0 - rho, rho[None, :] * soup[:, None]  # [G], [L, G]
    th = (keep[None, None, :] * e[:, :, None]) + amb[:, None, :]
    tab = np.stack([log(th), log(1.0 - th)], axis=-1)
    if mask is not None:
        tab[np.asarray(mask) == 0] = 0.0
    return tab


def genotype_rows(gt_used, assign):
    """g_of_cell [cells, L] int64: the genotypes of every cell's source at the used loci, -1 throughout for a cell that takes no part
    (assign 255); gt_used [S, L]"""
    gt_used, assign = np.asarray(gt_used, np.int64), np.asarray(assign, np.int64)
    part = assign != NONE
    out = np.full((len(assign), gt_used.shape[1]), -1, np.int64)
    out[part] = gt_used[assign[part]]
    return out


def cell_sums(mat, tab, g_of_cell):
    """(ll [cells, G], n_entries [cells] uint32): per (cell, j) the sum over the cell's entries in row order of ((alt la) + (ref lb)),
    (la, lb) = tab[l][g_of_cell[c, l]][j]; mat: a cluster.Matrix over the used loci (built with the call's mask); a cell whose row of
    g_of_cell is negative takes no part: a row of 0.0 and 0 entries"""
    tab, g = np.asarray(tab, np.float64), np.asarray(g_of_cell, np.int64)
    part = g.min(axis=1, initial=0) >= 0 if g.shape[1] else np.ones(mat.N, bool)
    ll = np.zeros((mat.N, tab.shape[2]))
    for rows, ent in mat.rows.steps:
        keep = part[rows]
        rows, ent = rows[keep], ent[keep]
        l = mat.r_lo[ent]
        t = tab[l, g[rows, l]]  # [m, G, 2]
        ll[rows] = ll[rows] + ((mat.r_al[ent, None] * t[:, :, 0]) + (mat.r_re[ent, None] * t[:, :, 1]))
    return ll, np.where(part, mat.entries, 0).astype(np.uint32)


def _fold_one(ll, member):
    n, G = ll.shape
    p = np.zeros((OBJ_THREADS, G))
    for i in range(0, n, OBJ_THREADS):
        m = member[i:i + OBJ_THREADS]
        t = np.flatnonzero(m)
        p[t] = p[t] + ll[i:i + OBJ_THREADS][m]
    h = OBJ_THREADS // 2
    while h:
        p[:h] = p[:h] + p[h:2 * h]
        h //= 2
    return p[0].copy()


def fold(ll, assign, S):
    """(total [G], source_total [S, G], source_cells [S]) in the device's order: thread t of 256 adds its cells t, t + 256, ... in
    ascending order, skipping the cells that take no part (for a source: the cells of other sources); the 256 partial sums are
    folded pairwise, h = 128 ... 1"""
    ll, assign = np.asarray(ll, np.float64), np.asarray(assign, np.int64)
    total = _fold_one(ll, assign != NONE)
    src = np.stack([_fold_one(ll, assign == s) for s in range(S)]) if S else np.zeros((0, ll.shape[1]))
    return total, src, np.array([(assign == s).sum() for s in range(S)], np.uint64)


def vertex(rho, y):
    """The vertex rule on y [G] or [n, G] over the grid rho [G]: dict of j_star (the smallest argmax), rho, se, curvature.  jj =
    min(max(j*, 1), G - 2); the parabola through the points jj - 1, jj, jj + 1 in the header's order of operations; the curvature
    is 0 where neither step of y exceeds FLAT |y1|; a curvature that is not negative gives rho[j*] and se = +inf"""
    rho, y = np.asarray(rho, np.float64), np.asarray(y, np.float64)
    one = y.ndim == 1
    y = np.atleast_2d(y)
    n, G = y.shape
    js = np.argmax(y, axis=1)
    jj = np.minimum(np.maximum(js, 1), G - 2)
    r = np.arange(n)
    x0, x1, x2 = rho[jj - 1], rho[jj], rho[jj + 1]
    y0, y1, y2 = y[r, jj - 1], y[r, jj], y[r, jj + 1]
    with np.errstate(all="ignore"):
        h0, h1 = x1 - x0, x2 - x1
        e0, e1 = y1 - y0, y2 - y1
        d0, d1 = e0 / h0, e1 / h1
        lim = FLAT * np.abs(y1)
        c = np.where((np.abs(e0) > lim) | (np.abs(e1) > lim), (2.0 * (d1 - d0)) / (h0 + h1), 0.0)
        v = (0.5 * (x0 + x1)) - (d0 / c)
        v = np.where(v < x0, x0, v)
        v = np.where(v > x2, x2, v)
        se = 1.0 / np.sqrt(-c)
    neg = c < 0.0
    out = dict(j_star=js, rho=np.where(neg, v, rho[js]), se=np.where(neg, se, np.inf), curvature=c)
    return {k: (v[0].item() if one else v) for k, v in out.items()}


def profile(mat, gt_used, assign, rho, alt_total=None, ref_total=None, tab=None, err=0.01, min_loci=1):
    """cellector_ambient_profile on host arrays.  mat: a cluster.Matrix over the used loci, built with the call's mask; gt_used [S, L]
    the sources' genotypes at the used loci; tab: the device's table for the device's bits, None = numpy's from the loci's totals.
    Returns the dict of Cellector.ambient_profile."""
    gt_used, assign = np.asarray(gt_used, np.uint8), np.asarray(assign, np.uint8)
    if tab is None:
        tab = tables(alt_total, ref_total, rho, err, mat.mask)
    ll, cnt = cell_sums(mat, tab, genotype_rows(gt_used, assign))
    total, src, cells = fold(ll, assign, gt_used.shape[0])
    v = vertex(rho, ll) if mat.N else dict(rho=np.zeros(0), se=np.zeros(0))
    out_of = (assign == NONE) | (cnt < int(min_loci))
    return dict(ll=ll, total=total, source_total=src, source_cells=cells, n_entries=cnt, cell_rho=np.where(out_of, np.nan, v["rho"]),
                cell_se=np.where(out_of, np.nan, v["se"]), tab=tab)


def estimate(mat, gt_used, assign, alt_total=None, ref_total=None, tables_of=None, **params):
    """cellector_estimate_ambient on host arrays: the zooming grid search.  tables_of(rho) -> tab [L, 4, G, 2]: the device's tables
    of a grid (Cellector.ambient_tables), for the device's bits; None = numpy's from the loci's totals.  Returns the summary's fields
    as a dict, the per-cell outputs of round 0 (cell_rho, cell_se, n_entries) and the last round's grid, total and source_total."""
    prm = _params(params)
    G, S = int(prm["grid"]), np.asarray(gt_used).shape[0]
    lo, hi = float(prm["lo"]), float(prm["hi"])
    first = None
    for rnd in range(int(prm["rounds"])):
        if rnd:
            js = int(np.argmax(pr["total"]))
            lo, hi = float(rho[max(js - 1, 0)]), float(rho[min(js + 1, G - 1)])
        rho = grid(lo, hi, G)
        tab = tables_of(rho) if tables_of is not None else None
        pr = profile(mat, gt_used, assign, rho, alt_total, ref_total, tab, prm["err"], prm["min_loci"])
        first = first or pr
    clamp = lambda x: min(max(x, float(prm["lo"])), float(prm["hi"]))
    v = vertex(rho, pr["total"])
    est = clamp(v["rho"])
    src_rho, src_se = np.full(64, np.nan), np.full(64, np.nan)
    cells = np.zeros(64, np.uint64)
    cells[:S] = pr["source_cells"]
    for s in range(S):
        if cells[s]:
            vs = vertex(rho, pr["source_total"][s])
            src_rho[s], src_se[s] = clamp(vs["rho"]), vs["se"]
    return dict(rho=est, se=v["se"], curvature=v["curvature"], log_likelihood=float(pr["total"][v["j_star"]]), lo=lo, hi=hi,
                j_star=int(v["j_star"]), at_boundary=int(est <= float(prm["lo"]) or est >= float(prm["hi"])), rounds=int(prm["rounds"]),
                n_cells_used=int((np.asarray(assign) != NONE).sum()), source_rho=src_rho, source_se=src_se, source_cells=cells,
                cell_rho=first["cell_rho"], cell_se=first["cell_se"], n_entries=first["n_entries"], grid=rho, total=pr["total"],
                source_total=pr["source_total"])
