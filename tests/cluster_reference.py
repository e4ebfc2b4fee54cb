"""80-bit reference of one E step and one M step of the genotype clustering (cellector_cluster_e_step / cellector_cluster_m_step;
csrc/kernels_cluster.hip) and the device's error bounds.

A plain helper for the tests (no fixtures, no GPU), independent of cellector_amd/cluster.py: it shares no code with the twin and
adds with np.add.reduceat over the COO sorted by segment, in np.longdouble.  Inputs are doubles (the tables of an E step, the weights
of an M step); every product and sum is formed in longdouble, u64 = 2^-64.

Bounds (u = 2^-53; nothing here is fitted to observed errors).  n = the entries of the cell (E) or of the locus (M).

  s      each entry's term rounds three times (two products, their sum): u (|alt la| + |ref lb| + |term|) <= 2 u |term|' with
         |term|' = |alt la| + |ref lb| (both products have one sign, la, lb <= 0).  The accumulator adds n terms one after the
         other: n - 1 further roundings of partial sums, each at most the full sum in size: (n - 1) u sum |term|'.
         B_s = (n + 1) u sum |term|'  (0 for a cell without entries: its sum is exactly 0).
  x      = s / T: B_x = B_s / T + u |x|.
  w      d_k = x_k - m rounds once and carries the errors of both operands: e_k = B_x[k] + max_j B_x[j] + u |d_k|.  exp is good to an
         ulp, at most C_EXP u relative (ROCm device-libs' OCML documents "exp: 1 ulp" and "log: 1 ulp" for f64; posterior_reference
         uses the same constant): rel_k = expm1(e_k) + C_EXP u.  den adds K such terms in order: its relative error is at most the
         w-weighted mean of rel_k, bounded here by its maximum over k, plus (K - 1) u.  The division rounds once:
         rel(w_k) = (1 + rel_k) (1 + u) / (1 - rel_den) - 1.
  o      = m + log(den): B_o = max_j B_x[j] + rel_den / (1 - rel_den) + C_LOG u |log den| + u |o|, C_LOG = 2 (one ulp of log as a
         relative error).
  obj    the sum of o over the cells: sum B_o, plus the additions: ceil(N / 256) - 1 in a thread's chain and 8 in the fold, each at
         most u sum |o|.
  A, T   a product and an add per entry: B_A = u sum w alt + (n - 1) u sum w alt = n u sum w alt; B_T likewise.
  theta  (A + 1) / (T + 2): two additions and a division, rel = (B_A + u (A + 1)) / (A + 1) + (B_T + u (T + 2)) / (T + 2) + u, first
         order, widened by REF_SHARE; the clamp to [floor, 1 - floor] moves no value away from the reference's.
  tab    from the SAME double theta (the M step's theta is compared bit for bit first): la = log(theta) is within C_LOG u |la| of the
         true logarithm, lb = log(1 - theta) with the subtraction done in double on both sides, within C_LOG u |lb|.

The reference repeats the operations at 2^-64: every bound is widened by posterior_reference.REF_SHARE of itself for it, and a
comparison adds half an ulp of the double the reference is rounded to where it is compared as one.
"""
import math

import numpy as np

import posterior_reference as pr
import tile_reference as tr

LD = np.longdouble
U = tr.U53
C_EXP = pr.C_EXP
C_LOG = 2.0
OBJ_THREADS = 256


def _filter(coo, mask):
    lo, ce, al, re = (np.asarray(x, np.int64) for x in coo)
    if mask is not None:
        keep = np.asarray(mask)[lo] != 0
        lo, ce, al, re = lo[keep], ce[keep], al[keep], re[keep]
    return lo, ce, al, re


def _seg_sum(idx, vals, n):
    """out [n, J] longdouble: the rows of vals added per segment idx (sorted by segment, then np.add.reduceat)"""
    out = np.zeros((n, vals.shape[1]), LD)
    if len(idx):
        order = np.argsort(idx, kind="stable")
        cnt = np.bincount(idx, minlength=n)
        starts = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        nz = cnt > 0
        out[nz] = np.add.reduceat(vals[order], starts[nz], axis=0)
    return out


# ---- E step ----------------------------------------------------------------------------------------------------------------------
def e_reference(L, N, coo, tab, K, R, temp=None, mask=None):
    """dict: s, w [N, J] and o [N, R], objective [R] in longdouble, and the bounds B_s [N, J], rel_w [N, J], B_obj [R] in double"""
    lo, ce, al, re = _filter(coo, mask)
    tab = np.asarray(tab, np.float64)
    J = K * R
    assert tab.shape == (L, J, 2)
    la, lb = tab[:, :, 0].astype(LD), tab[:, :, 1].astype(LD)
    pa, pb = al.astype(LD)[:, None] * la[lo], re.astype(LD)[:, None] * lb[lo]
    s, mag = _seg_sum(ce, pa + pb, N), _seg_sum(ce, np.abs(pa) + np.abs(pb), N)
    n = np.bincount(ce, minlength=N).astype(np.float64)
    B_s = (n[:, None] + 1.0) * U * mag.astype(np.float64)
    T = np.ones(N, LD) if temp is None else np.asarray(temp, np.float64).astype(LD)
    x = (s / T[:, None]).reshape(N, R, K)
    B_x = (B_s / T.astype(np.float64)[:, None] + U * np.abs(x.reshape(N, J)).astype(np.float64)).reshape(N, R, K)
    m = x.max(axis=2)
    d = x - m[:, :, None]
    ex = np.exp(d)
    den = ex.sum(axis=2)
    w = ex / den[:, :, None]
    o = m + np.log(den)
    B_m = B_x.max(axis=2)
    e = B_x + B_m[:, :, None] + U * np.abs(d).astype(np.float64)
    rel_k = np.expm1(e) + C_EXP * U
    rel_den = rel_k.max(axis=2) + (K - 1) * U
    rel_w = ((1.0 + rel_k) * (1.0 + U) / (1.0 - rel_den[:, :, None]) - 1.0) * (1.0 + pr.REF_SHARE)
    B_o = B_m + rel_den / (1.0 - rel_den) + C_LOG * U * np.abs(np.log(den)).astype(np.float64) + U * np.abs(o).astype(np.float64)
    adds = max(-(-N // OBJ_THREADS) - 1, 0) + 8
    B_obj = (B_o.sum(axis=0) + adds * U * np.abs(o).sum(axis=0).astype(np.float64)) * (1.0 + pr.REF_SHARE)
    return dict(s=s, w=w.reshape(N, J), o=o, objective=o.sum(axis=0), B_s=B_s * (1.0 + pr.REF_SHARE), rel_w=rel_w.reshape(N, J),
                B_obj=B_obj, entries=n)


def compare_e(ref, got):
    """got: dict of s, w [N, J], objective [R] doubles.  Returns {name: worst observed / bound}; a value <= 1 is inside."""
    out = {}
    s = np.asarray(got["s"], np.float64)
    bound = ref["B_s"] + np.where(ref["B_s"] > 0, 0.5 * np.spacing(np.abs(ref["s"].astype(np.float64))), 0.0)
    d = np.abs(s.astype(LD) - ref["s"]).astype(np.float64)
    out["s"] = float(np.where(bound > 0, d / np.where(bound > 0, bound, 1.0), np.where(d == 0, 0.0, np.inf)).max(initial=0.0))
    w, want = np.asarray(got["w"], np.float64), ref["w"]
    seen = want >= pr.OBSERVABLE
    ratio = (np.abs(w.astype(LD) - want) / (ref["rel_w"] * np.where(seen, want, LD(1)))).astype(np.float64)
    ratio = np.where(seen, ratio, np.where((w >= 0) & (w < pr.UNOBSERVED_BELOW), 0.0, np.inf))
    out["w"] = float(np.where(np.isfinite(w), ratio, np.inf).max(initial=0.0))
    obj = np.asarray(got["objective"], np.float64)
    bound = ref["B_obj"] + 0.5 * np.spacing(np.abs(ref["objective"].astype(np.float64)))
    out["objective"] = float((np.abs(obj.astype(LD) - ref["objective"]).astype(np.float64) / bound).max(initial=0.0))
    return out


# ---- M step ----------------------------------------------------------------------------------------------------------------------
def m_reference(L, N, coo, w, theta_floor=0.01, mask=None):
    """dict: A, T, theta [J, L] in longdouble (a masked locus: 0, 0, 0.5) and the bounds B_A, B_T, B_theta [J, L] in double"""
    lo, ce, al, re = _filter(coo, mask)
    w = np.asarray(w, np.float64)
    J = w.shape[1]
    wl = w.astype(LD)[ce]
    A, T = _seg_sum(lo, wl * al.astype(LD)[:, None], L), _seg_sum(lo, wl * (al + re).astype(LD)[:, None], L)
    n = np.bincount(lo, minlength=L).astype(np.float64)[:, None]
    B_A, B_T = n * U * A.astype(np.float64), n * U * T.astype(np.float64)
    th = (A + 1) / (T + 2)
    rel = (B_A + U * (A.astype(np.float64) + 1.0)) / (A.astype(np.float64) + 1.0) \
        + (B_T + U * (T.astype(np.float64) + 2.0)) / (T.astype(np.float64) + 2.0) + U
    B_th = rel * th.astype(np.float64) * (1.0 + pr.REF_SHARE)
    th = np.minimum(np.maximum(th, LD(theta_floor)), LD(1.0 - theta_floor))
    if mask is not None:
        th[np.asarray(mask) == 0] = 0.5
    f = 1.0 + pr.REF_SHARE
    return dict(A=A.T.copy(), T=T.T.copy(), theta=th.T.copy(), B_A=(B_A * f).T.copy(), B_T=(B_T * f).T.copy(), B_theta=B_th.T.copy(),
                entries=n[:, 0])


def tab_reference(theta, mask=None):
    """(tab [L, J, 2] longdouble, bound [L, J, 2]) of a double theta [J, L]: log(theta) and log of the DOUBLE 1.0 - theta"""
    th = np.asarray(theta, np.float64).T
    tab = np.stack([np.log(th.astype(LD)), np.log((1.0 - th).astype(LD))], axis=-1)
    if mask is not None:
        tab[np.asarray(mask) == 0] = 0
    return tab, C_LOG * U * np.abs(tab).astype(np.float64) * (1.0 + pr.REF_SHARE)


def _ratio(got, want, bound):
    d = np.abs(np.asarray(got, np.float64).astype(LD) - want).astype(np.float64)
    bound = bound + np.where(bound > 0, 0.5 * np.spacing(np.abs(want.astype(np.float64))), 0.0)
    return float(np.where(bound > 0, d / np.where(bound > 0, bound, 1.0), np.where(d == 0, 0.0, np.inf)).max(initial=0.0))


def compare_m(ref, got):
    """got: dict of A, T, theta [J, L].  Returns {name: worst observed / bound}"""
    return dict(A=_ratio(got["A"], ref["A"], ref["B_A"]), T=_ratio(got["T"], ref["T"], ref["B_T"]),
                theta=_ratio(got["theta"], ref["theta"], ref["B_theta"]))


def compare_tab(theta, mask, got_tab):
    want, bound = tab_reference(theta, mask)
    d = np.abs(np.asarray(got_tab, np.float64).astype(LD) - want).astype(np.float64)
    return float(np.where(bound > 0, d / np.where(bound > 0, bound, 1.0), np.where(d == 0, 0.0, np.inf)).max(initial=0.0))


# ---- the cases -------------------------------------------------------------------------------------------------------------------
COLUMNS = ((2, 1), (3, 1), (5, 1), (4, 3), (8, 3), (16, 3), (4, 16))  # (K, R): J = 2, 3, 5, 12, 24, 48, 64: every lane width 2 ... 64
_hand = {}


def hand_matrix():
    """(L, N, coo) in file order (locus-major, cells NOT ascending inside a locus): 1101 cells x 1231 loci, neither a multiple of 64.
    Cells 0, 7 and the last: no entry; cell 1: one entry; cells 2, 3, 4: 63, 64, 65 entries; cell 5: 1100 entries (> 1024); locus
    0: no entry; locus 1: an entry of every cell from 8 on (1094 with the repeats, > 1024); (locus 1, cell 200) three times with different
    counts; counts of 0 (also both) and 65535."""
    if not _hand:
        L, N = 1231, 1101
        rng = np.random.default_rng(11)
        lo, ce = [], []
        for cell, k in ((1, 1), (2, 63), (3, 64), (4, 65), (5, 1100)):
            lo.append(2 + rng.choice(L - 2, k, replace=False)); ce.append(np.full(k, cell))
        for cell in range(8, N - 1):
            k = int(rng.integers(1, 12))
            lo.append(2 + rng.choice(L - 2, k, replace=False)); ce.append(np.full(k, cell))
        many = np.arange(8, N - 1)
        lo.append(np.ones(len(many), np.int64)); ce.append(many)
        lo.append(np.array([1, 1])); ce.append(np.array([200, 200]))
        lo, ce = np.concatenate(lo), np.concatenate(ce)
        tot = rng.geometric(0.4, len(lo))
        al = rng.binomial(tot, rng.choice([0.05, 0.5, 0.95], len(lo)))
        re = tot - al
        al[:3], re[:3] = [0, 65535, 65535], [65535, 0, 65535]
        al[5], re[5] = 0, 0
        al[7], re[7] = 0, 3
        perm = rng.permutation(len(lo))  # file order: shuffled inside a locus, then locus-major (stable)
        order = perm[np.argsort(lo[perm], kind="stable")]
        _hand["m"] = (L, N, [np.asarray(x, np.int64)[order] for x in (lo, ce, al, re)])
    return _hand["m"]


def matrices():
    """name -> (L, N, coo): posterior_reference's row-length and tier-2 matrices and the hand-built one"""
    out = {}
    for name in ("row-lengths", "tier2"):
        L, N, coo, _ = pr.matrix(name)
        out[name] = (L, N, coo)
    out["hand"] = hand_matrix()
    return out


def case_mask(L):
    return (np.random.default_rng(977 + L).random(L) < 0.8).astype(np.uint8)


def case_tab(L, J, seed=3):
    """tables of a theta drawn in [0.01, 0.99], as doubles"""
    th = 0.01 + 0.98 * np.random.default_rng(seed + 31 * J + L).random((L, J))
    return np.stack([np.log(th), np.log(1.0 - th)], axis=-1)


def case_temp(N, seed=5):
    """temperatures from 1 to 10^4, a few next to 1"""
    rng = np.random.default_rng(seed + N)
    t = 10.0 ** rng.uniform(0.0, 4.0, N)
    t[::7] = 1.0
    t[1::7] = np.nextafter(1.0, 2.0)
    t[2::7] = 1.0 + 1e-9
    return t


def case_w(N, K, R, seed=9):
    """weights as an E step leaves them: per (cell, restart) a draw that sums to 1 to rounding, some of them one-hot, some tiny"""
    rng = np.random.default_rng(seed + N + 64 * K + R)
    g = rng.gamma(0.3, 1.0, (N, R, K)) + 1e-300
    g[::5] = np.eye(K)[rng.integers(0, K, (len(g[::5]), R))]
    return (g / g.sum(axis=2, keepdims=True)).reshape(N, R * K)
