"""Donor pair fractions on host arrays: the numpy twin of cellector_pair_fraction_tables / cellector_donor_pair_fractions
(include/cellector_ffi.h states the model; csrc/kernels_pair_fraction.hip runs it).

Every cell is scored under a pair of donors (a, b) at G values of f, the share of its reads that come from donor a, at once:
theta = (f theta_a) + ((1 - f) theta_b) per (locus, genotype of a, genotype of b, grid point).  The maximum of a cell's profile over
the grid and the parabola through the three points around it (ambient.vertex: the same rule, the same function) give the cell's share
and its standard error; kinds() names what the share says.

The sums are the library's sums in the library's order (a cell's entries in by-cell CSR row order, one rounded product and one
rounded add at a time): fed the DEVICE's tables, cell_sums, and fractions' j_star and cell_frac and kinds carry the device's bits;
cell_se passes through a square root and agrees to an ulp or two.  log is numpy's, not the device's: the tables made here agree with
the device's to a few ulps.
"""
import math
from decimal import Decimal

import numpy as np

from . import ambient, donors
from .cluster import Matrix  # noqa: F401  (the matrix in the library's row order; callers build one and pass it in)

NONE = 255
BALANCED, TOWARD_A, TOWARD_B, FLAT = 0, 1, 2, 3
KIND_NAMES = {BALANCED: "balanced", TOWARD_A: "toward_a", TOWARD_B: "toward_b", FLAT: "flat", NONE: "NA"}
DEFAULTS = dict(min_fraction=0.1, min_loci=1)
DEFAULT_GRID = np.arange(17) / 16.0  # j / 16.0: holds 0, 0.5 and 1 exactly


def _params(params):
    p = dict(DEFAULTS)
    for k, v in dict(params or {}).items():
        if k not in p:
            raise TypeError(f"unknown parameter {k!r}")
        p[k] = v
    return p


def tables(alt_total, ref_total, frac=None, err=0.01, ambient=0.03, mask=None, log=np.log):
    """tab [L, 16, G, 2] = (log theta, log(1 - theta)) at index 4 g_a + g_b, theta = (f_j theta_ga) + ((1 - f_j) theta_gb), theta_g =
    donors.thetas (step 2 of the donor model); a masked locus carries (0, 0)"""
    frac = DEFAULT_GRID if frac is None else np.asarray(frac, np.float64)
    th = donors.thetas(alt_total, ref_total, err, ambient)  # [L, 4]
    wa = frac[None, None, None, :] * th[:, :, None, None]  # [L, ga, 1, G]
    wb = (1.0 - frac)[None, None, None, :] * th[:, None, :, None]  # [L, 1, gb, G]
    t = (wa + wb).reshape(len(th), 16, len(frac))
    tab = np.stack([log(t), log(1.0 - t)], axis=-1)
    if mask is not None:
        tab[np.asarray(mask) == 0] = 0.0
    return tab


def cell_sums(mat, tab, g, pair_a, pair_b):
    """(ll [cells, G], n_entries [cells] uint32): per (cell, j) the sum over the cell's entries in row order of ((alt la) + (ref lb)),
    (la, lb) = tab[l][4 g[l, a_c] + g[l, b_c]][j]; mat: a cluster.Matrix over the used loci (built with the call's mask), g [L, D] the
    donors' genotypes there; a cell whose pair_a is 255 takes no part: a row of 0.0 and 0 entries"""
    tab, g = np.asarray(tab, np.float64), np.asarray(g, np.int64)
    a, b = np.asarray(pair_a, np.int64), np.asarray(pair_b, np.int64)
    part = a != NONE
    a, b = np.where(part, a, 0), np.where(part, b, 0)
    ll = np.zeros((mat.N, tab.shape[2]))
    for rows, ent in mat.rows.steps:
        keep = part[rows]
        rows, ent = rows[keep], ent[keep]
        l = mat.r_lo[ent]
        t = tab[l, 4 * g[l, a[rows]] + g[l, b[rows]]]  # [m, G, 2]
        ll[rows] = ll[rows] + ((mat.r_al[ent, None] * t[:, :, 0]) + (mat.r_re[ent, None] * t[:, :, 1]))
    return ll, np.where(part, mat.entries, 0).astype(np.uint32)


def fractions(frac, ll):
    """The vertex rule of the ambient model on every cell's profile ll [cells, G] over the grid frac [G]: dict of j_star uint8,
    cell_frac, cell_se (before the kinds blank the cells that take no part)"""
    frac = DEFAULT_GRID if frac is None else np.asarray(frac, np.float64)
    ll = np.asarray(ll, np.float64)
    if not len(ll):
        return dict(j_star=np.zeros(0, np.uint8), cell_frac=np.zeros(0), cell_se=np.zeros(0))
    v = ambient.vertex(frac, ll)
    return dict(j_star=v["j_star"].astype(np.uint8), cell_frac=v["rho"], cell_se=v["se"])


def kinds(cell_frac, cell_se, n_entries, pair_a, min_fraction=0.1, min_loci=1):
    """kind [cells] uint8: 255 = pair_a 255 or fewer than min_loci entries, else 3 = flat (se +inf), else 1 = toward a (frac > 1.0 -
    min_fraction), else 2 = toward b (frac < min_fraction), else 0 = balanced"""
    f, se = np.asarray(cell_frac, np.float64), np.asarray(cell_se, np.float64)
    top = 1.0 - float(min_fraction)
    with np.errstate(invalid="ignore"):
        k = np.where(se == np.inf, FLAT, np.where(f > top, TOWARD_A, np.where(f < float(min_fraction), TOWARD_B, BALANCED)))
    out = (np.asarray(pair_a) == NONE) | (np.asarray(n_entries).astype(np.int64) < int(min_loci))
    return np.where(out, NONE, k).astype(np.uint8)


def summary(kind, pair_a, pair_b):
    """the fields of cellector_pair_fraction_summary as a dict"""
    kind, a, b = np.asarray(kind), np.asarray(pair_a, np.int64), np.asarray(pair_b, np.int64)
    cells = np.bincount(a[kind == TOWARD_A], minlength=64) + np.bincount(b[kind == TOWARD_B], minlength=64)
    return dict(n_balanced=int((kind == BALANCED).sum()), n_toward_a=int((kind == TOWARD_A).sum()), n_toward_b=int((kind == TOWARD_B).sum()),
                n_flat=int((kind == FLAT).sum()), n_none=int((kind == NONE).sum()), donor_cells=cells.astype(np.uint64))


def pair_fractions(mat, g, pair_a, pair_b, frac=None, alt_total=None, ref_total=None, tab=None, params=None, err=0.01, ambient=0.03):
    """cellector_donor_pair_fractions on host arrays.  mat: a cluster.Matrix over the used loci, built with the call's mask; g [L, D]
    the donors' genotypes at the used loci; tab: the device's table for the device's bits, None = numpy's from the loci's totals.
    Returns the dict of Cellector.donor_pair_fractions (summary: a dict)."""
    prm = _params(params)
    frac = DEFAULT_GRID if frac is None else np.asarray(frac, np.float64)
    if tab is None:
        tab = tables(alt_total, ref_total, frac, err, ambient, mat.mask)
    ll, cnt = cell_sums(mat, tab, g, pair_a, pair_b)
    v = fractions(frac, ll)
    kind = kinds(v["cell_frac"], v["cell_se"], cnt, pair_a, prm["min_fraction"], prm["min_loci"])
    out = kind == NONE
    return dict(ll=ll, n_entries=cnt, cell_frac=np.where(out, np.nan, v["cell_frac"]), cell_se=np.where(out, np.nan, v["cell_se"]),
                j_star=v["j_star"], kind=kind, frac=frac, tab=tab, summary=summary(kind, pair_a, pair_b))


# ---- the host binary's table -------------------------------------------------------------------------------------------------------
TSV_HEAD = "barcode\tdonor_a\tdonor_b\tn_loci\tfraction\tse\tll_half\tll_max\tkind\n"


def _display(x):
    """a double as the host binary writes it: the shortest digits that read back, positional, a whole value without '.0'"""
    x = float(x)
    if math.isnan(x):
        return "NaN"
    if math.isinf(x):
        return "inf" if x > 0 else "-inf"
    s = format(Decimal(repr(x)), "f")
    return s[:-2] if s.endswith(".0") else s


def render(barcodes, names, res, pair_a, pair_b):
    """cellector_doublet_fractions.tsv as `cellector --doublet_fraction true` writes it, from the dict of pair_fractions (or of
    Cellector.donor_pair_fractions) on a grid that holds 0.5 in its middle: NA throughout for a cell that took no part"""
    G = res["ll"].shape[1]
    out = [TSV_HEAD]
    for c, bc in enumerate(barcodes):
        if pair_a[c] == NONE:
            out.append(bc + "\tNA" * 8 + "\n")
            continue
        k = int(res["kind"][c])
        est = ["NA", "NA"] if k == NONE else [_display(res["cell_frac"][c]), _display(res["cell_se"][c])]
        out.append("\t".join([bc, names[pair_a[c]], names[pair_b[c]], str(int(res["n_entries"][c]))] + est +
                             [_display(res["ll"][c, G // 2]), _display(res["ll"][c, int(res["j_star"][c])]), KIND_NAMES[k]]) + "\n")
    return "".join(out)
