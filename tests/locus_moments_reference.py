"""Reference of the locus moments (cellector_locus_moments, cellector_locus_total_counts): a plain helper for the tests (no
fixtures, no GPU).

Inputs are the entries in the by-cell CSR's order (cell, then locus, a repeated pair in load order): locus, cell, alt, ref; per-locus
alpha / beta; a mask (1 = used, None = all used) and the exclusion flags.  For a used locus l and a class of cells (min: flagged,
maj: the rest) the four sums are, over the class' entries at l,

    exp_c[l] = sum E(alpha_l, beta_l, alt + ref)        var_c[l] = sum V(alpha_l, beta_l, alt + ref)

with E and V the `expected` and `variance` of pmf_reference.records, added here in np.longdouble; a masked locus gives 0.

Bounds (u = 2^-53; nothing fitted).  Every entry's device value is within pmf_reference's b_expected (b_variance) of the
reference, so B = the class' sum of those at the locus.  The device forms s = s + (double)count[n] * T[n] for n = 1..17 and then
adds the locus' entries with a larger total one by one: 17 products, whose roundings are u |term| each and together at most
u (|S| + B) because all terms of a sum have one sign (E <= 0, V >= 0); and m = 17 + (far entries of the class) additions, each
of a partial sum that is at most the whole, u (|S| + B) each.  Plus half an ulp of S for the rounding of the longdouble sum:

    |device - reference| <= B + (m + 1) u (|S| + B) + ulp(S) / 2.

histogram(): the [L][19] integer counts by np.bincount: entries per (locus, total 0..17), slot 18 = the entries above 17.

matrix_c(): the smallest shape at which the far list's segments can go wrong, 40 loci x 200 cells (min_alt = min_ref = 0): far
totals at the first and the last locus; a locus whose four far entries (18, 18, 40, 300) sit in cells 3, 70, 71 and 199
interleaved with entries of total <= 17; a locus with far entries only; loci with none; a far entry at a locus its mask masks; a
far pair listed twice in one cell.
"""
import numpy as np

import pmf_reference as pr

LD = np.longdouble
U = 2.0 ** -53
SMALL = pr.SMALL  # 17
KEYS = ("exp_min", "exp_maj", "var_min", "var_maj")


def csr_order(lo, ce):
    """the by-cell CSR's order: cell, then locus, repeated pairs in load order"""
    return np.lexsort((np.arange(len(lo)), lo, ce))


def histogram(L, lo, ce, n, flags=None):
    """[L][19] uint32: entries of the flagged cells (None: all cells) per locus and total 0..17; slot 18: those above 17"""
    lo, n = np.asarray(lo, np.int64), np.asarray(n, np.int64)
    if flags is not None:
        sel = np.asarray(flags)[np.asarray(ce, np.int64)] != 0
        lo, n = lo[sel], n[sel]
    slot = np.minimum(n, SMALL + 1)
    return np.bincount(lo * (SMALL + 2) + slot, minlength=L * (SMALL + 2)).reshape(L, SMALL + 2).astype(np.uint32)


def _per_locus(L, lo, values):
    s = np.zeros(L, LD)
    np.add.at(s, lo, np.asarray(values).astype(LD))
    return s


def sums(L, lo, ce, n, rec, mask, flags):
    """The four longdouble sums and their bounds.  rec: pmf_reference.records(alpha, beta, lo, alt, ref) of the same entries.
    Returns a dict: KEYS -> longdouble [L]; "b_" + key -> the bound (double) [L]; "far_min" / "far_maj" -> far entries of the class
    at used loci [L]."""
    lo, ce, n = (np.asarray(x, np.int64) for x in (lo, ce, n))
    live = np.ones(len(lo), bool) if mask is None else np.asarray(mask)[lo] != 0
    is_min = np.asarray(flags)[ce] != 0
    out = {}
    for cls, sel in (("min", live & is_min), ("maj", live & ~is_min)):
        far = np.bincount(lo[sel & (n > SMALL)], minlength=L).astype(np.float64)
        out["far_" + cls] = far
        for what, col in (("exp", "expected"), ("var", "variance")):
            s_ld = _per_locus(L, lo[sel], rec[col][sel])
            s = np.abs(s_ld.astype(np.float64))
            b = _per_locus(L, lo[sel], rec["b_" + col][sel]).astype(np.float64)
            out[f"{what}_{cls}"] = s_ld
            out[f"b_{what}_{cls}"] = b + (SMALL + far + 1.0) * U * (s + b) + 0.5 * np.spacing(s)
    return out


def add_bound(far, s_ld):
    """the device's multiply-adds alone on a sum S of values taken as exact: (17 + far + 1) u |S| + ulp(S) / 2"""
    s = np.abs(np.asarray(s_ld).astype(np.float64))
    return (SMALL + np.asarray(far, np.float64) + 1.0) * U * s + 0.5 * np.spacing(s)


# ---- matrix C -------------------------------------------------------------------------------------------------------------------
LC, NC = 40, 200
C_FOUR = (10, ((3, 18), (70, 18), (71, 40), (199, 300)))  # locus, (cell, total) of its four far entries
C_FAR_ONLY = 20
C_MASKED = 30
C_TWICE = (15, 60, (22, 41))  # locus, cell, the totals of the pair listed twice
C_FAR = [(0, 5, 20), (0, 150, 33), (LC - 1, 0, 19), (LC - 1, NC - 1, 64), (C_FAR_ONLY, 7, 18), (C_FAR_ONLY, 8, 25),
         (C_MASKED, 9, 50), (C_TWICE[0], C_TWICE[1], C_TWICE[2][0]), (C_TWICE[0], C_TWICE[1], C_TWICE[2][1])] + \
        [(C_FOUR[0], c, t) for c, t in C_FOUR[1]]  # (locus, cell, total) of every far entry


def matrix_c():
    """(lo, ce, al, re) in load order, locus-major (so that "load order" inside a pair is defined here)"""
    rng = np.random.default_rng(40200)
    small = [1] * 10 + [2] * 4 + [3, 4, 0, 5, 6, 8, 9, 13, 16, 17]
    k = 700
    lo, ce, tot = rng.integers(0, LC, k), rng.integers(0, NC, k), rng.choice(small, k)
    keep = lo != C_FAR_ONLY
    lo, ce, tot = lo[keep], ce[keep], tot[keep]
    # entries of total <= 17 at the locus of the four far entries, in cells around and between theirs (one in a far cell itself)
    extra = [(C_FOUR[0], c, t) for c, t in ((0, 1), (2, 17), (4, 3), (69, 2), (70, 5), (72, 1), (198, 17))]
    extra += [(C_TWICE[0], C_TWICE[1], 2)]
    add = np.array(extra + C_FAR, np.int64)
    lo, ce, tot = np.concatenate([lo, add[:, 0]]), np.concatenate([ce, add[:, 1]]), np.concatenate([tot, add[:, 2]])
    al = (rng.random(len(tot)) * (tot + 1)).astype(np.int64)
    perm = rng.permutation(len(lo))
    perm = perm[np.argsort(lo[perm], kind="stable")]
    return [x[perm] for x in (lo, ce, al, tot - al)]


def matrix_c_mask():
    m = np.ones(LC, np.uint8)
    m[[C_MASKED, 3]] = 0
    return m


def matrix_c_flags():
    """the flag sets of matrix C: empty, all, random 10 %, the cells of the far entries, their complement"""
    rng = np.random.default_rng(7)
    planted = np.zeros(NC, np.uint8)
    planted[sorted({c for _, c, _ in C_FAR})] = 1
    return {"empty": np.zeros(NC, np.uint8), "all": np.ones(NC, np.uint8), "random 10 %": (rng.random(NC) < 0.1).astype(np.uint8),
            "planted": planted, "complement": (1 - planted).astype(np.uint8)}
