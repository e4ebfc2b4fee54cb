"""K-genotype class scoring on host arrays: the numpy twin of cellector_class_tallies / _class_alpha_betas /
_class_posteriors / cellector_refine_classes (include/cellector_ffi.h states the model; csrc/kernels_classes.hip runs it).

The integer tallies and the alpha / beta bits are the library's own.  The posterior chain repeats the device's operations in the
same order in numpy doubles; exp and log are numpy's, not the device's, so its last bits need not be the device's.  The per-cell
sums are not formed here: refine() and posteriors() take any function ll(alpha, beta, mask) -> (ll [cells], loci_used [cells]),
e.g. Cellector.cell_log_likelihoods or an extended-precision reference.

Doublet classes are not formed: they would need K (K - 1) / 2 further distributions and a prior nobody has argued for.
"""
import math

import numpy as np

UNLABELLED = 255
MAX_CLASSES = 16


def check_labels(labels, n_classes):
    labels = np.ascontiguousarray(labels, dtype=np.uint8)
    if not 1 <= n_classes <= MAX_CLASSES:
        raise ValueError(f"{n_classes} classes, 1..{MAX_CLASSES} are supported")
    bad = np.nonzero((labels >= n_classes) & (labels != UNLABELLED))[0]
    if bad.size:
        raise ValueError(f"cell {bad[0]} has label {labels[bad[0]]}, neither below the {n_classes} classes nor 255 (unlabelled)")
    if not (labels != UNLABELLED).any():
        raise ValueError(f"every cell is unlabelled: all {n_classes} classes are dead")
    return labels


def class_sizes(labels, n_classes):
    """cells per class [K] (unlabelled cells are in none)"""
    labels = np.asarray(labels)
    return np.bincount(labels[labels != UNLABELLED], minlength=n_classes).astype(np.uint64)


def class_tallies(n_loci, coo, labels, n_classes):
    """(cells [K], alt [K, L], ref [K, L]) uint64 from COO arrays (locus, cell, alt, ref) over the used loci: per class the sums
    of the allele counts of its cells' entries; a repeated (locus, cell) pair counts each time"""
    lo, ce, al, re = (np.asarray(x, np.int64) for x in coo)
    labels = np.asarray(labels)
    alt = np.zeros((n_classes, n_loci), np.uint64)
    ref = np.zeros((n_classes, n_loci), np.uint64)
    lab = labels[ce].astype(np.int64)
    for k in range(n_classes):
        sel = lab == k
        np.add.at(alt[k], lo[sel], al[sel].astype(np.uint64))
        np.add.at(ref[k], lo[sel], re[sel].astype(np.uint64))
    return class_sizes(labels, n_classes), alt, ref


def class_alpha_betas(alt, ref, scale=None):
    """alpha_k = (double)alt_k * scale_k + 1.0, beta_k likewise: a rounded product and a rounded sum"""
    alt, ref = np.asarray(alt), np.asarray(ref)
    s = np.ones(alt.shape[0]) if scale is None else np.asarray(scale, np.float64)
    return alt.astype(np.float64) * s[:, None] + 1.0, ref.astype(np.float64) * s[:, None] + 1.0


def default_log_priors(cells):
    """lp_k = log((n_k + 1) / (N_lab + K_live)) with the C library's log; a dead class (n_k == 0) takes no part: -inf here"""
    cells = [int(x) for x in cells]
    n_lab, k_live = sum(cells), sum(1 for x in cells if x)
    return np.array([math.log((x + 1.0) / (float(n_lab) + float(k_live))) if x else -math.inf for x in cells])


def reference_scales(n_excluded, n_cells):
    """(scale [2], log_prior [2]) that make K = 2 with class 0 = the exclusion set the reference's two-class posterior without
    the doublet term: the majority's counts scaled by max(mf0, 0.01) (main.rs:250-253), priors log(mf), log(1 - mf) (main.rs:264-265)"""
    mf = max((n_excluded + 1.0) / (n_cells + 1.0), 0.01)
    return np.array([1.0, mf]), np.array([math.log(mf), math.log(1.0 - mf) if mf < 1.0 else -math.inf])


def posterior_chain(ll, log_prior, live):
    """Step 6 in the device's operation order.  ll [K, cells], log_prior [K], live [K] bool.  Returns a dict: posterior [K, cells]
    (0 in a dead class' row), best [cells] uint8, qual [cells] uint64, x [K, cells] (nan in a dead row), den, rest."""
    ll = np.asarray(ll, np.float64)
    K, n = ll.shape
    live = np.asarray(live, bool)
    ks = [k for k in range(K) if live[k]]
    x = np.full((K, n), np.nan)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = np.full(n, -np.inf)
        best = np.zeros(n, np.uint8)
        for j, k in enumerate(ks):
            x[k] = log_prior[k] + ll[k]
            take = (x[k] > m) if j else np.ones(n, bool)
            m = np.where(take, x[k], m)
            best = np.where(take, k, best).astype(np.uint8)
        s = np.zeros(n)
        for k in ks:
            s = s + np.exp(x[k] - m)
        den = m + np.log(s)
        post = np.zeros((K, n))
        rest = np.zeros(n)
        for k in ks:
            post[k] = np.exp(x[k] - den)
            rest = rest + np.where(best == k, 0.0, post[k])
        q = np.fmin(-10.0 * np.log10(rest), 255.0)
        qual = np.where(q > 0.0, q, 0.0).astype(np.uint64)
    return dict(posterior=post, best=best, qual=qual, x=x, den=den, rest=rest)


def _recount_rule(step, class_delta, n_moved, sizes_with_unlabelled):
    """a step counts its tallies from scratch on the first step, with class_delta off, and when more cells moved than a recount
    would walk (every cell outside the largest slot)"""
    return step == 0 or not class_delta or n_moved > int(sizes_with_unlabelled.sum()) - int(sizes_with_unlabelled.max())


def posteriors(n_loci, coo, labels, n_classes, ll_fn, scale=None, log_prior=None, mask=None):
    """Steps 1-6 for one labelling: dict with cells, alt, ref, alpha, beta, log_prior (as used), live, ll [K, cells], loci_used
    and the outputs of posterior_chain"""
    labels = check_labels(labels, n_classes)
    cells, alt, ref = class_tallies(n_loci, coo, labels, n_classes)
    alpha, beta = class_alpha_betas(alt, ref, scale)
    live = cells > 0
    lp = default_log_priors(cells) if log_prior is None else np.asarray(log_prior, np.float64)
    n = len(labels)
    ll = np.full((n_classes, n), -np.inf)
    loci_used = np.zeros(n)
    for k in range(n_classes):
        if live[k]:
            ll[k], loci_used = (np.asarray(v, np.float64) for v in ll_fn(alpha[k], beta[k], mask)[:2])
    out = posterior_chain(ll, lp, live)
    out.update(cells=cells, alt=alt, ref=ref, alpha=alpha, beta=beta, log_prior=lp, live=live, ll=ll, loci_used=loci_used)
    return out


def refine(n_loci, coo, labels, n_classes, ll_fn, scale=None, log_prior=None, mask=None, max_iter=100, min_loci=1,
           class_delta=True):
    """The hard-EM loop of cellector_refine_classes.  Returns a dict: labels (the result), summary (iterations, converged,
    n_moved_last, n_moved_total, n_recounts, class_cells [16]), steps (the posteriors() dict of every step run, each with
    labels_in / labels_out / n_moved) and ll / posterior / qual of the last step."""
    if min_loci < 1:
        raise ValueError("min_loci must be at least 1")
    labels = check_labels(labels, n_classes).copy()
    summ = dict(iterations=0, converged=0, n_moved_last=0, n_moved_total=0, n_recounts=0)
    steps, n_moved = [], 0
    while True:
        sizes = np.bincount(np.where(labels == UNLABELLED, n_classes, labels), minlength=n_classes + 1)
        if _recount_rule(len(steps), class_delta, n_moved, sizes):
            summ["n_recounts"] += 1
        st = posteriors(n_loci, coo, labels, n_classes, ll_fn, scale, log_prior, mask)
        st["labels_in"] = labels.copy()
        steps.append(st)
        if max_iter == 0:
            st["labels_out"], st["n_moved"] = labels.copy(), 0
            break
        move = (labels != UNLABELLED) & (st["loci_used"].astype(np.uint64) >= np.uint64(min_loci))
        new = np.where(move, st["best"], labels).astype(np.uint8)
        n_moved = int((new != labels).sum())
        labels = new
        st["labels_out"], st["n_moved"] = labels.copy(), n_moved
        summ["iterations"] += 1
        summ["n_moved_last"] = n_moved
        summ["n_moved_total"] += n_moved
        if n_moved == 0:
            summ["converged"] = 1
            break
        if summ["iterations"] == max_iter:
            break
    cc = np.zeros(16, np.uint64)
    cc[:n_classes] = class_sizes(labels, n_classes)
    summ["class_cells"] = cc
    last = steps[-1]
    return dict(labels=labels, summary=summ, steps=steps, ll=last["ll"], posterior=last["posterior"], qual=last["qual"])
