"""Genotype clusters without labels on host arrays: the numpy twin of cellector_cluster / cellector_cluster_e_step /
cellector_cluster_m_step (include/cellector_ffi.h states the model; csrc/kernels_cluster.hip runs it).

A mixture of per-locus binomials over allele fractions, fitted by soft EM from random starts; a depth-dependent temperature is
annealed away over a few stages; R restarts run as columns j = r K + k of one pass and the best is kept.

The start draw is the library's bit for bit (integer hash, one product, one sum).  The sums are the library's sums in the library's
order: an E-step sum walks a cell's entries in by-cell CSR row order, an M-step tally a locus' entries in ascending cell order, one
rounded product and one rounded add at a time, so s, A, T and theta carry the device's bits whenever the tables (E step) or the
weights (M step) do.  log and exp are numpy's, not the device's: tables, weights and objectives agree to a few ulps, and a whole fit
may end a stage an iteration apart from the device's.

sums="dense" replaces the ordered sums by matrix products over a dense copy of the matrix (any order, BLAS): the same model to
rounding, hundreds of times faster on a small matrix, for checks of the partition and not of the bits.
"""
import itertools
import math

import numpy as np

UNLABELLED = 255
GOLD = 0x9E3779B97F4A7C15
_M64 = (1 << 64) - 1
DEFAULTS = dict(theta_floor=0.01, anneal_base=20.0, tol=0.01, anneal_steps=9, max_iter=50, min_loci=1)
OBJ_THREADS = 256


# ---- the start draw ------------------------------------------------------------------------------------------------------------
def mix64(z):
    """the splitmix64 finaliser (csrc/mix64.h) on uint64 arrays"""
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def start_theta(seed, L, J, theta_floor=0.01):
    """theta [L, J]: floor + (1 - 2 floor) u, u(l, j) = (mix64(mix64(seed GOLD + GOLD) + (l J + j + 1) GOLD) >> 11) 2^-53"""
    sm = mix64(np.uint64((int(seed) * GOLD + GOLD) & _M64))
    with np.errstate(over="ignore"):
        i = np.arange(1, L * J + 1, dtype=np.uint64) * np.uint64(GOLD) + sm
    u = (mix64(i) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return (theta_floor + (1.0 - 2.0 * theta_floor) * u).reshape(L, J)


def tables(theta, mask=None):
    """tab [L, J, 2] = (log theta, log(1 - theta)); a masked locus carries (0, 0)"""
    theta = np.asarray(theta, np.float64)
    tab = np.stack([np.log(theta), np.log(1.0 - theta)], axis=-1)
    if mask is not None:
        tab[np.asarray(mask) == 0] = 0.0
    return tab


# ---- the matrix in the library's two orders ----------------------------------------------------------------------------------------
class _Ordered:
    """the entries of every segment (a cell's, a locus') in order, regrouped by position inside the segment: step p holds the
    p-th entry of every segment that has one, so that a strictly sequential sum per segment is one vector add per step"""

    def __init__(self, seg, n_seg):
        cnt = np.bincount(seg, minlength=n_seg)
        start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        by_len = np.argsort(-cnt, kind="stable")
        n_at = np.searchsorted(-cnt[by_len], -np.arange(1, cnt.max(initial=0) + 1), side="right")  # segments longer than p
        self.steps = [(by_len[:m], start[by_len[:m]] + p) for p, m in enumerate(n_at)]
        self.count = cnt


class Matrix:
    """COO arrays (locus, cell, alt, ref) over the used loci in file order, as the library holds them: the by-cell CSR (a stable
    sort by locus, then a stable sort by cell) and the by-locus list in ascending cell order (a stable sort of the CSR by locus)"""

    def __init__(self, n_loci, n_cells, coo, mask=None):
        lo, ce, al, re = (np.asarray(x, np.int64) for x in coo)
        self.L, self.N = int(n_loci), int(n_cells)
        self.mask = None if mask is None else (np.asarray(mask) != 0)
        if self.mask is not None:
            keep = self.mask[lo]
            lo, ce, al, re = lo[keep], ce[keep], al[keep], re[keep]
        o = np.argsort(lo, kind="stable")
        o = o[np.argsort(ce[o], kind="stable")]
        self.r_lo, self.r_ce, self.r_al, self.r_re = lo[o], ce[o], al[o].astype(np.float64), re[o].astype(np.float64)
        o2 = np.argsort(self.r_lo, kind="stable")
        self.c_ce, self.c_al, self.c_tot = self.r_ce[o2], self.r_al[o2], self.r_al[o2] + self.r_re[o2]
        self.rows = _Ordered(self.r_ce, self.N)
        self.cols = _Ordered(self.r_lo[o2], self.L)
        self.depth = np.bincount(ce, weights=(al + re).astype(np.float64), minlength=self.N)  # exact: whole numbers below 2^53
        self.entries = self.rows.count
        self._dense = None

    def dense(self):
        if self._dense is None:
            a, t = np.zeros((self.N, self.L)), np.zeros((self.N, self.L))
            np.add.at(a, (self.r_ce, self.r_lo), self.r_al)
            np.add.at(t, (self.r_ce, self.r_lo), self.r_al + self.r_re)
            self._dense = (a, t - a, t)
        return self._dense


# ---- the two steps -------------------------------------------------------------------------------------------------------------
def objective_sum(o):
    """obj [R] from o [cells, R] in the device's order: thread t of 256 adds the cells t, t + 256, ... in ascending order, then the
    256 partial sums are folded pairwise"""
    n, R = o.shape
    rows = -(-n // OBJ_THREADS)
    pad = np.zeros((max(rows, 1) * OBJ_THREADS, R))
    pad[:n] = o
    pad = pad.reshape(-1, OBJ_THREADS, R)
    p = np.zeros((OBJ_THREADS, R))
    for i in range(pad.shape[0]):
        p = p + pad[i]
    h = OBJ_THREADS // 2
    while h:
        p[:h] = p[:h] + p[h:2 * h]
        h //= 2
    return p[0].copy()


def softmax(s, K, R, temp=None):
    """(w [cells, J], o [cells, R]) from the sums s [cells, J]: per restart x_k = s_k / T, m = max, den = sum exp(x_k - m) in ascending
    k, w = exp(x - m) / den, o = m + log(den)"""
    n = s.shape[0]
    x = s if temp is None else s / np.asarray(temp, np.float64)[:, None]
    x = x.reshape(n, R, K)
    m = x.max(axis=2)
    den = np.zeros((n, R))
    for k in range(K):
        den = den + np.exp(x[:, :, k] - m)
    w = np.exp(x - m[:, :, None]) / den[:, :, None]
    return w.reshape(n, R * K), m + np.log(den)


def e_sums(mat, tab, sums="ordered"):
    """s [cells, J]: per (cell, column) the sum over the cell's entries in row order of ((alt la) + (ref lb))"""
    tab = np.asarray(tab, np.float64)
    la, lb = tab[:, :, 0], tab[:, :, 1]
    if sums == "dense":
        a, r, _ = mat.dense()
        return a @ la + r @ lb
    s = np.zeros((mat.N, la.shape[1]))
    for rows, ent in mat.rows.steps:
        l = mat.r_lo[ent]
        s[rows] = s[rows] + ((mat.r_al[ent, None] * la[l]) + (mat.r_re[ent, None] * lb[l]))
    return s


def e_step(mat, tab, K, R, temp=None, sums="ordered"):
    """dict of s, w [cells, J], objective [R] (and o [cells, R])"""
    s = e_sums(mat, tab, sums)
    w, o = softmax(s, K, R, temp)
    return dict(s=s, w=w, o=o, objective=objective_sum(o))


def m_step(mat, w, theta_floor=0.01, sums="ordered"):
    """dict of A, T, theta [J, L] and tab [L, J, 2] from weights w [cells, J]: A = sum w alt, T = sum w (alt + ref) over the locus'
    entries in ascending cell order, theta = min(max((A + 1) / (T + 2), floor), 1 - floor); a masked locus: A = T = 0, theta = 0.5"""
    w = np.asarray(w, np.float64)
    J = w.shape[1]
    if sums == "dense":
        a, _, t = mat.dense()
        A, T = a.T @ w, t.T @ w
    else:
        A, T = np.zeros((mat.L, J)), np.zeros((mat.L, J))
        for loci, ent in mat.cols.steps:
            wv = w[mat.c_ce[ent]]
            A[loci] = A[loci] + wv * mat.c_al[ent, None]
            T[loci] = T[loci] + wv * mat.c_tot[ent, None]
    theta = np.minimum(np.maximum((A + 1.0) / (T + 2.0), theta_floor), 1.0 - theta_floor)
    if mat.mask is not None:
        theta[~mat.mask] = 0.5
    return dict(A=A.T.copy(), T=T.T.copy(), theta=theta.T.copy(), tab=tables(theta, mat.mask))


# ---- the whole fit -------------------------------------------------------------------------------------------------------------
def fit(n_loci, n_cells, coo, n_clusters, n_restarts=None, seed=4, mask=None, sums="ordered", **params):
    """cellector_cluster on host arrays.  Returns a dict: labels, ll [K, cells], posterior [K, cells], theta [K, L], objective [R],
    best_restart, iterations, iterations_per_stage, stages, cluster_cells [K], n_unlabelled."""
    K = int(n_clusters)
    R = min(16, 64 // K) if n_restarts is None else int(n_restarts)
    p = dict(DEFAULTS)
    for k, v in params.items():
        if k not in p:
            raise TypeError(f"unknown parameter {k!r}")
        p[k] = v
    if not 2 <= K <= 16 or R < 1 or K * R > 64:
        raise ValueError(f"{K} clusters x {R} restarts: 2..16 clusters, at least one restart, at most 64 columns")
    mat = coo if isinstance(coo, Matrix) else Matrix(n_loci, n_cells, coo, mask)
    J, floor, S = K * R, float(p["theta_floor"]), int(p["anneal_steps"])
    theta = start_theta(seed, mat.L, J, floor)
    per_stage = []
    for stage in range(S):
        temp = np.maximum(1.0, mat.depth / (float(p["anneal_base"]) * 2.0 ** stage)) if stage + 1 < S else None
        prev, it = None, 0
        while it < int(p["max_iter"]):
            e = e_step(mat, tables(theta, mat.mask), K, R, temp, sums)
            theta = m_step(mat, e["w"], floor, sums)["theta"].T
            it += 1
            still = prev is not None and bool((np.abs(e["objective"] - prev) < p["tol"]).all())
            prev = e["objective"]
            if still:
                break
        per_stage.append(it)
    e = e_step(mat, tables(theta, mat.mask), K, R, None, sums)
    obj = e["objective"] - float(mat.N) * math.log(float(K))
    best = int(np.argmax(obj))  # (the first index attaining the maximum)
    s = e["s"][:, best * K:(best + 1) * K]
    labels = np.argmax(s, axis=1).astype(np.uint8)
    labels[mat.entries < int(p["min_loci"])] = UNLABELLED
    return dict(labels=labels, ll=s.T.copy(), posterior=e["w"][:, best * K:(best + 1) * K].T.copy(),
                theta=theta[:, best * K:(best + 1) * K].T.copy(), objective=obj, best_restart=best, iterations=sum(per_stage),
                iterations_per_stage=per_stage, stages=S, cluster_cells=np.bincount(labels[labels != UNLABELLED], minlength=K),
                n_unlabelled=int((labels == UNLABELLED).sum()))


def best_permutation(labels, truth, n_clusters):
    """(perm, n_agree): the relabelling perm[cluster] = truth class under which the most cells (255 left out on either side) carry
    their true class, and how many do.  Exhaustive up to 8 clusters, greedy on the confusion matrix above."""
    labels, truth, K = np.asarray(labels).astype(np.int64), np.asarray(truth).astype(np.int64), int(n_clusters)
    ok = (labels != UNLABELLED) & (truth != UNLABELLED)
    conf = np.zeros((K, K), np.int64)
    np.add.at(conf, (labels[ok], truth[ok]), 1)
    if K <= 8:
        best = max(itertools.permutations(range(K)), key=lambda q: sum(conf[k, q[k]] for k in range(K)))
        return list(best), int(sum(conf[k, best[k]] for k in range(K)))
    perm, c = [-1] * K, conf.astype(np.float64)
    for _ in range(K):
        k, t = np.unravel_index(np.argmax(c), c.shape)
        perm[k] = int(t)
        c[k, :], c[:, t] = -1.0, -1.0
    return perm, int(sum(conf[k, perm[k]] for k in range(K)))
