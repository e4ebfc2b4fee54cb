"""80-bit reference of the donor pair fractions (cellector_pair_fraction_tables / cellector_donor_pair_fractions;
csrc/kernels_pair_fraction.hip), the device's error bounds, the cases the CPU and the GPU tests share and the planted-share generator.

A plain helper for the tests (no fixtures, no GPU), independent of cellector_amd/pair_fraction.py: it shares no code with the twin.
The model is stated once more here, in np.longdouble (u64 = 2^-64).  D donors with genotypes gt [D, L] (0 = 0/0, 1 = 0/1, 2 = 1/1, 3 =
no call), a cell c scored under the pair (pair_a[c], pair_b[c]) (pair_a 255: it takes no part), a grid frac [G] of shares of donor a:

  theta_{l,g}       = ((1 - ambient) e_g) + (ambient soup_l),  e = (err, 0.5, 1 - err, soup_l),  soup_l = (A_l + 1) / ((A_l + R_l) + 2)
  theta_{l,ga,gb,j} = (f_j theta_{l,ga}) + ((1 - f_j) theta_{l,gb})
  tab[l][4 ga + gb][j] = (log theta, log(1 - theta)), (0, 0) at a masked locus
  ll[c][j]          = the sum over the cell's entries at unmasked loci of alt tab[..][0] + ref tab[..][1], ga = gt[a_c, l], gb = gt[b_c, l]
  vertex rule       ambient_reference.vertex_reference on (frac, ll[c]): the smallest argmax j*, the parabola through the three points
                    around it, its vertex clamped into their span and se = 1 / sqrt(-curvature); flat or convex: frac[j*], se = +inf
  kind              255 = no part or n_entries < min_loci; 3 = se +inf; 1 = frac > 1 - min_fraction; 2 = frac < min_fraction; else 0

Bounds (u = 2^-53; nothing here is fitted to observed errors; they are donor_reference's and ambient_reference's own).  n = the
entries of the cell at used, unmasked loci.

  tab    theta is a chain of IEEE operations on doubles (whole-number totals, err, ambient, f_j): the device's theta IS the double theta
         formed here in double, so tab = log(double theta) and log(double (1.0 - theta)) are held to C_LOG u |log|.
  ll     the sums of doubles (the tables the device returned): B = (n + 1) u sum (|alt la| + |ref lb|).

The reference repeats the operations at 2^-64: both bounds are widened by posterior_reference.REF_SHARE of themselves for it, and a
comparison adds half an ulp of the double the reference is rounded to.

cell_frac and cell_se are quotients of differences of nearly equal sums: they are compared with the twin bit for bit
(tests/test_gpu_pair_fraction.py), not with this reference.  The reference's own estimate is what the recovery test holds to the
planted share.
"""
import math

import numpy as np

import ambient_reference as ar
import donor_reference as dr

LD = np.longdouble
U = dr.U
C_LOG = dr.C_LOG
F = dr.F
NONE = 255
DEFAULTS = dict(min_fraction=0.1, min_loci=1)
DEFAULT_GRID = np.array([float(j) / 16.0 for j in range(17)])


# ---- tables ----------------------------------------------------------------------------------------------------------------------
def theta_double(A, R, frac, err, ambient):
    """theta [L, 16, G] in double, operation by operation as the header states it"""
    th = dr.theta_double(A, R, err, ambient)  # [L, 4]
    out = np.empty((len(th), 16, len(frac)))
    for j, f in enumerate(np.asarray(frac, np.float64)):
        for a in range(4):
            for b in range(4):
                out[:, 4 * a + b, j] = (f * th[:, a]) + ((1.0 - f) * th[:, b])
    return out


def _logs(th, mask):
    tab = np.stack([np.log(th.astype(LD)), np.log((1.0 - th).astype(LD))], axis=-1)
    if mask is not None:
        tab[np.asarray(mask) == 0] = 0
    return tab


def tab_reference(A, R, frac, err=0.01, ambient=0.03, mask=None):
    """(tab [L, 16, G, 2] in longdouble from the double thetas, its bound)"""
    tab = _logs(theta_double(A, R, frac, err, ambient), mask)
    return tab, C_LOG * U * np.abs(tab).astype(np.float64) * F


def compare_tab(A, R, frac, err, ambient, mask, tab):
    want, B = tab_reference(A, R, frac, err, ambient, mask)
    return dr._ratio(tab, want, B)


# ---- cell sums -------------------------------------------------------------------------------------------------------------------
def _pair_rows(coo, gt_used, pair_a, pair_b, mask):
    """the entries of the cells that take part, in row order, with the two genotypes of each"""
    gt_used = np.asarray(gt_used, np.int64)
    a, b = np.asarray(pair_a, np.int64), np.asarray(pair_b, np.int64)
    lo, ce, al, re = dr._rows(coo, mask)
    part = a[ce] != NONE
    lo, ce, al, re = lo[part], ce[part], al[part], re[part]
    return lo, ce, al, re, gt_used[a[ce], lo], gt_used[b[ce], lo]


def cell_reference(N, coo, gt_used, pair_a, pair_b, tab, mask=None, index=lambda ga, gb: 4 * ga + gb):
    """The cell sums in longdouble from a table tab [L, 16, G, 2] (a DOUBLE one, the device's or the twin's, for the bounds; or the
    reference's own longdouble one): dict of ll [N, G], B_ll, n_entries.  index: the table row of a genotype pair (the sensitivity test
    passes a wrong one)."""
    lo, ce, al, re, ga, gb = _pair_rows(coo, gt_used, pair_a, pair_b, mask)
    tab = np.asarray(tab)
    t = (tab if tab.dtype == LD else tab.astype(np.float64).astype(LD))[lo, index(ga, gb)]  # [m, G, 2]
    pa, pb = al.astype(LD)[:, None] * t[:, :, 0], re.astype(LD)[:, None] * t[:, :, 1]
    ll, cnt = dr._seg_sum(ce, pa + pb, N)
    mag, _ = dr._seg_sum(ce, np.abs(pa) + np.abs(pb), N)
    return dict(ll=ll, B_ll=(cnt[:, None] + 1.0) * U * mag.astype(np.float64) * F, n_entries=cnt)


def informative(N, coo, gt_used, pair_a, pair_b, A, R, err, ambient, mask=None):
    """[N] bool: the cell has an entry with a read at a locus where the two genotypes of its pair differ in theta (two codes that give
    the same theta, or an entry of 0 + 0 reads, tell f nothing)"""
    lo, ce, al, re, ga, gb = _pair_rows(coo, gt_used, pair_a, pair_b, mask)
    th = dr.theta_double(A, R, err, ambient)
    inf = (th[lo, ga] != th[lo, gb]) & (al + re > 0)
    return np.bincount(ce[inf], minlength=N) > 0


def compare(N, coo, gt_used, pair_a, pair_b, mask, got):
    """got: the dict of Cellector.donor_pair_fractions with tables (or the twin's).  Returns ({name: worst observed / bound}, ref)."""
    ref = cell_reference(N, coo, gt_used, pair_a, pair_b, got["tab"], mask)
    return dict(ll=dr._ratio(got["ll"], ref["ll"], ref["B_ll"]),
                n_entries=0.0 if np.array_equal(np.asarray(got["n_entries"]).astype(np.int64), ref["n_entries"]) else np.inf), ref


# ---- the vertex rule and the kinds -----------------------------------------------------------------------------------------------
def fractions_reference(frac, ll, n_entries, pair_a, min_fraction=0.1, min_loci=1):
    """dict of j_star, cell_frac, cell_se, kind from profiles ll [N, G] (longdouble): ambient_reference's vertex rule per cell"""
    N = len(ll)
    js, est, se = np.zeros(N, np.int64), np.full(N, np.nan), np.full(N, np.nan)
    kind = np.full(N, NONE, np.uint8)
    for c in range(N):
        j, e, s, _ = ar.vertex_reference(frac, ll[c])
        js[c] = j
        if pair_a[c] == NONE or n_entries[c] < min_loci:
            continue
        est[c], se[c] = e, s
        kind[c] = 3 if s == math.inf else 1 if e > 1.0 - min_fraction else 2 if e < min_fraction else 0
    return dict(j_star=js, cell_frac=est, cell_se=se, kind=kind)


def estimate_reference(L, N, coo, gt_used, pair_a, pair_b, frac=None, err=0.01, ambient=0.03, mask=None, **kw):
    """cellector_donor_pair_fractions in longdouble, the logarithms never rounded to double: the dict of fractions_reference and ll"""
    frac = DEFAULT_GRID if frac is None else np.asarray(frac, np.float64)
    A, R = dr.totals(L, coo)
    tab = _logs(theta_double(A, R, frac, err, ambient), mask)
    ref = cell_reference(N, coo, gt_used, pair_a, pair_b, tab, mask)
    out = fractions_reference(frac, ref["ll"], ref["n_entries"], np.asarray(pair_a), **dict(DEFAULTS, **kw))
    out.update(ll=ref["ll"], n_entries=ref["n_entries"])
    return out


# ---- the cases -------------------------------------------------------------------------------------------------------------------
DONORS = (2, 3, 33, 64)  # one and two packed words; 2: the one pair there is


_pairs = {}


def case_pairs(D, N=dr.CASE_N, kind="mixed"):
    """(pair_a, pair_b) uint8 for donor_reference.case_matrix() and case_gt(D): a = c % D, b = (a + 1 + (c // D) % (D - 1)) % D: every
    ordered pair in turn; every 7th cell 255 (and its pair_b 255, a value refused elsewhere: it is ignored); none: every cell 255.
    With that rule alone 5.6 % (D = 64; 6.5 % under case_mask()) of the cells that have an entry have none that bears on f (a third
    of all genotype pairs are equal, a tenth of the calls are blank and a tenth of the rows hold one entry), above the 5 % the
    sensitivity test allows.  So a cell without such an entry under case_mask() steps its b on through the rotation, (b + 1) % D
    skipping a, to the first donor that gives it one, if any does."""
    if (D, N) not in _pairs:
        c = np.arange(N)
        a = c % D
        b = (a + 1 + (c // D) % (D - 1)) % D
        L, N_, coo = dr.case_matrix()
        if N == N_:
            A, R = dr.totals(L, coo)
            gt = dr.case_gt(D)
            for _ in range(D - 2):
                dull = ~informative(N, coo, gt, a, b, A, R, 0.01, 0.03, dr.case_mask())
                if not dull.any():
                    break
                nxt = (b + 1) % D
                nxt = np.where(nxt == a, (nxt + 1) % D, nxt)
                b = np.where(dull, nxt, b)
            # (a cell no donor helps has been round the rotation D - 2 times and one step on: any b is as good for it)
        _pairs[(D, N)] = (a, b)
    a, b = (x.astype(np.uint8) for x in _pairs[(D, N)])
    a[::7] = NONE
    b[::7] = NONE
    if kind == "none":
        a[:] = NONE
    return a, b


def case_grid_uneven(G=9):
    """a caller's grid: ascending, unequal steps, 0, 0.5 and 1 included"""
    return np.array([0.0, 0.02, 0.1, 0.25, 0.5, 0.6, 0.9, 0.99, 1.0][:G])


def case_grid(G):
    """a uniform grid over [0, 1] of G points, made by one division per point; an odd G holds 0.5 exactly"""
    return np.array([float(j) / float(G - 1) for j in range(G)])


# ---- the planted pool ------------------------------------------------------------------------------------------------------------
PLANT_FS = (1.0, 0.5, 0.3, 0.15)
PLANT_PER_F = 300
PLANT_SEEDS = (0, 1, 2)
PLANT_RHO = 0.03
PLANT_DEPTH = 2.0  # the Poisson mean of a parent cell's depth above 1 (raised from 1.0: see planted)
_plant = {}


def planted(seed, err=0.01):
    """(L, N, coo, gt [3, L], pair_a, pair_b [N], f [N]): the pool of ambient_reference.planted(0.03, seed) (300 singlets, which take no
    part: pair_a 255, f NaN) and behind it 300 cells at each planted share f = 1, 0.5, 0.3, 0.15 under a random ordered pair of
    distinct donors.  A planted cell has an entry at a locus with probability 0.3; a cell at f = 1 is one cell of depth 1 + Poisson(2),
    a cell at f < 1 two parent cells of that depth each in one droplet (at 1 + Poisson(1), the depth of ambient_reference.planted, the
    reference itself put one of 900 planted singlets at 0.883, below 1 - min_fraction: the depth is raised, the condition stays);
    alt ~ Binomial(depth, (1 - rho) (f e_a + (1 - f) e_b) + rho soup), soup = the pool's allele fraction at the locus as
    ambient_reference.planted forms it."""
    if seed not in _plant:
        L, N0, coo0, gt, _ = ar.planted(PLANT_RHO, seed, err)
        rng = np.random.default_rng(7000 + seed)
        e = np.array([err, 0.5, 1.0 - err])[gt]  # [3, L]
        soup = (np.array([0.6, 0.3, 0.1])[:, None] * e).sum(axis=0)
        M = PLANT_PER_F * len(PLANT_FS)
        f = np.repeat(np.array(PLANT_FS), PLANT_PER_F)
        a = rng.integers(0, 3, M)
        b = (a + 1 + rng.integers(0, 2, M)) % 3
        have = rng.random((L, M)) < 0.3
        lo, ce = np.nonzero(have)
        depth = 1 + rng.poisson(PLANT_DEPTH, len(lo))
        depth = np.where(f[ce] < 1.0, depth + 1 + rng.poisson(PLANT_DEPTH, len(lo)), depth)
        p = (1.0 - PLANT_RHO) * (f[ce] * e[a[ce], lo] + (1.0 - f[ce]) * e[b[ce], lo]) + PLANT_RHO * soup[lo]
        al = rng.binomial(depth, p)
        coo = [np.concatenate([x0, x.astype(np.int64)]) for x0, x in zip(coo0, (lo, ce + N0, al, depth - al))]
        _plant[seed] = (L, N0 + M, coo, gt, np.concatenate([np.full(N0, NONE), a]).astype(np.uint8),
                        np.concatenate([np.full(N0, NONE), b]).astype(np.uint8), np.concatenate([np.full(N0, np.nan), f]))
    return _plant[seed]
