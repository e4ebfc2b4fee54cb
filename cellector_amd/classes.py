"""K-genotype class scoring on host arrays: the numpy twin of cellector_class_tallies / _class_alpha_betas /
_class_posteriors / cellector_refine_classes (include/cellector_ffi.h states the model; csrc/kernels_classes.hip runs it).

The integer tallies and the alpha / beta bits are the library's own.  The posterior chain repeats the device's operations in the
same order in numpy doubles; exp and log are numpy's, not the device's, so its last bits need not be the device's.  The per-cell
sums are not formed here: refine() and posteriors() take any function ll(alpha, beta, mask) -> (ll [cells], loci_used [cells]),
e.g. Cellector.cell_log_likelihoods or an extended-precision reference.

The second half is the twin of the doublet calls (cellector_class_pair_alpha_betas / _class_doublets /
cellector_refine_class_doublets): the K (K - 1) / 2 pair distributions, the chain over singlets and pairs, the call, and the
held-out refine with its effective-class recount rule.
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


# ---- doublet classes over the K classes ------------------------------------------------------------------------------------------
def n_pairs(n_classes):
    return n_classes * (n_classes - 1) // 2


def pair_index(n_classes, a, b):
    """p(a, b) = a (2K - a - 1) / 2 + (b - a - 1) for 0 <= a < b < K: the pairs in lexicographic order"""
    if not 0 <= a < b < n_classes:
        raise ValueError(f"({a}, {b}) is no pair a < b of {n_classes} classes")
    return a * (2 * n_classes - a - 1) // 2 + (b - a - 1)


def pairs(n_classes):
    """the (a, b) in ascending p"""
    return [(a, b) for a in range(n_classes) for b in range(a + 1, n_classes)]


def effective_labels(labels, held, n_classes):
    """the tally slot of every cell: its label, or K for an unlabelled or a held cell"""
    labels = np.asarray(labels)
    out = np.where(labels == UNLABELLED, n_classes, labels).astype(np.int64)
    if held is not None:
        out = np.where(np.asarray(held) != 0, n_classes, out)
    return out


def _unheld(labels, held):
    labels = np.asarray(labels, np.uint8)
    return labels if held is None else np.where(np.asarray(held) != 0, UNLABELLED, labels).astype(np.uint8)


def balanced_pair_scales(cells):
    """ps_k = (double)n_min / (double)n_k, n_min the smallest live n_k; a dead class: 0"""
    cells = [int(x) for x in cells]
    live = [x for x in cells if x]
    n_min = min(live) if live else 0
    return np.array([float(n_min) / float(x) if x else 0.0 for x in cells])


def class_fractions(cells):
    """f_k = (n_k + 1) / (N_lab + K_live), the fraction inside the default singlet prior (formed for dead classes too)"""
    cells = [int(x) for x in cells]
    n_lab, k_live = sum(cells), sum(1 for x in cells if x)
    return np.array([(x + 1.0) / (float(n_lab) + float(k_live)) for x in cells])


def default_log_pair_priors(cells, n_cells):
    """lpp_ab = log((N / 1000 / 100) * max(min(f_a, f_b), 0.1)) in ascending p, N = all cells of the matrix (main.rs:259 with the
    smaller class of the pair in the place of the minority); not normalised"""
    f = class_fractions(cells)
    return np.array([math.log((float(n_cells) / 1000.0 / 100.0) * max(min(f[a], f[b]), 0.1)) for a, b in pairs(len(f))])


def class_pair_alpha_betas(alt, ref, pair_scale):
    """(alpha [P, L], beta [P, L]): ((double)alt_a * ps_a + (double)alt_b * ps_b) + 1.0 — two rounded products, a rounded sum, + 1"""
    alt, ref = np.asarray(alt).astype(np.float64), np.asarray(ref).astype(np.float64)
    ps = np.asarray(pair_scale, np.float64)
    K = alt.shape[0]
    a = np.zeros((n_pairs(K), alt.shape[1]))
    b = np.zeros_like(a)
    for p, (i, j) in enumerate(pairs(K)):
        a[p] = (alt[i] * ps[i] + alt[j] * ps[j]) + 1.0
        b[p] = (ref[i] * ps[i] + ref[j] * ps[j]) + 1.0
    return a, b


def reference_doublet_scales(n_excluded, n_cells):
    """(pair_scale [2], log_pair_prior [1]) that make K = 2 with class 0 = the exclusion set the reference's three-way posterior
    (with reference_scales for the singlets): the majority's counts at the unclamped mf0 (main.rs:245-246), the doublet prior
    log(N / 1000 / 100 * max(mf, 0.1)) (main.rs:259; max(max(mf0, 0.01), 0.1) = max(mf0, 0.1))"""
    mf0 = (n_excluded + 1.0) / (n_cells + 1.0)
    return np.array([1.0, mf0]), np.array([math.log(n_cells / 1000.0 / 100.0 * max(max(mf0, 0.01), 0.1))])


def doublet_chain(ll, ll_pair, log_prior, log_pair_prior, live):
    """Step 6 of the doublet model in the device's operation order.  ll [K, cells], ll_pair [P, cells], live [K] bool.  Returns a
    dict: posterior [K, cells], doublet_posterior, best, best_pair [cells, 2], call, qual, rest, den, x [K, cells] and y [P, cells]
    (nan in dead rows), pair_live [P]."""
    ll = np.asarray(ll, np.float64)
    K, n = ll.shape
    P = n_pairs(K)
    ll_pair = np.asarray(ll_pair, np.float64).reshape(P, n)
    live = np.asarray(live, bool)
    ks = [k for k in range(K) if live[k]]
    pl = np.array([live[a] and live[b] for a, b in pairs(K)], bool)
    ps = [p for p in range(P) if pl[p]]
    ab = pairs(K)
    x, y = np.full((K, n), np.nan), np.full((P, n), np.nan)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = np.full(n, -np.inf)
        best = np.zeros(n, np.uint8)
        for j, k in enumerate(ks):
            x[k] = log_prior[k] + ll[k]
            take = (x[k] > m) if j else np.ones(n, bool)
            m = np.where(take, x[k], m)
            best = np.where(take, k, best).astype(np.uint8)
        mp = np.full(n, -np.inf)
        bp = np.full((n, 2), UNLABELLED, np.uint8)
        for j, p in enumerate(ps):
            y[p] = log_pair_prior[p] + ll_pair[p]
            take = (y[p] > mp) if j else np.ones(n, bool)
            mp = np.where(take, y[p], mp)
            bp[take] = ab[p]
        if ps:
            m = np.where(mp > m, mp, m)
        s = np.zeros(n)
        for k in ks:
            s = s + np.exp(x[k] - m)
        for p in ps:
            s = s + np.exp(y[p] - m)
        den = m + np.log(s)
        post = np.zeros((K, n))
        others, every = np.zeros(n), np.zeros(n)
        for k in ks:
            post[k] = np.exp(x[k] - den)
            every = every + post[k]
            others = others + np.where(best == k, 0.0, post[k])
        dp = np.zeros(n)
        for p in ps:
            dp = dp + np.exp(y[p] - den)
        call = (dp > 0.5).astype(np.uint8)
        rest = np.where(call == 1, every, others + dp)
        q = np.fmin(-10.0 * np.log10(rest), 255.0)
        qual = np.where(q > 0.0, q, 0.0).astype(np.uint64)
    return dict(posterior=post, doublet_posterior=dp, best=best, best_pair=bp, call=call, qual=qual, rest=rest, den=den, x=x, y=y,
                pair_live=pl)


def doublet_posteriors(n_loci, coo, labels, n_classes, ll_fn, held=None, scale=None, pair_scale=None, log_prior=None,
                       log_pair_prior=None, mask=None):
    """Steps 1-6 of the doublet model for one (labels, held): dict with cells (unheld, [K]), alt, ref, alpha, beta, pair_alpha,
    pair_beta, pair_scale / log_prior / log_pair_prior (as used), live, ll, ll_pair, loci_used and the outputs of doublet_chain"""
    labels = check_labels(labels, n_classes)
    if not (_unheld(labels, held) != UNLABELLED).any():
        raise ValueError(f"every labelled cell is held: all {n_classes} classes are dead")
    cells, alt, ref = class_tallies(n_loci, coo, _unheld(labels, held), n_classes)
    alpha, beta = class_alpha_betas(alt, ref, scale)
    ps = balanced_pair_scales(cells) if pair_scale is None else np.asarray(pair_scale, np.float64)
    pa, pb = class_pair_alpha_betas(alt, ref, ps)
    live = cells > 0
    n = len(labels)
    lp = default_log_priors(cells) if log_prior is None else np.asarray(log_prior, np.float64)
    lpp = default_log_pair_priors(cells, n) if log_pair_prior is None else np.asarray(log_pair_prior, np.float64)
    ll = np.full((n_classes, n), -np.inf)
    llp = np.full((n_pairs(n_classes), n), -np.inf)
    loci_used = np.zeros(n)
    for k in range(n_classes):
        if live[k]:
            ll[k], loci_used = (np.asarray(v, np.float64) for v in ll_fn(alpha[k], beta[k], mask)[:2])
    for p, (a, b) in enumerate(pairs(n_classes)):
        if live[a] and live[b]:
            llp[p] = np.asarray(ll_fn(pa[p], pb[p], mask)[0], np.float64)
    out = doublet_chain(ll, llp, lp, lpp, live)
    out.update(cells=cells, alt=alt, ref=ref, alpha=alpha, beta=beta, pair_alpha=pa, pair_beta=pb, pair_scale=ps, log_prior=lp,
               log_pair_prior=lpp, live=live, ll=ll, ll_pair=llp, loci_used=loci_used)
    return out


def refine_doublets(n_loci, coo, labels, n_classes, ll_fn, held=None, scale=None, pair_scale=None, log_prior=None,
                    log_pair_prior=None, mask=None, doublet_threshold=0.5, max_iter=100, min_loci=1, class_delta=True):
    """The held-out refine of cellector_refine_class_doublets.  Returns a dict: labels, held (the result), summary (the fields of
    refine()'s, class_cells the unheld sizes, and n_held), steps (the doublet_posteriors() dict of every step run, each with
    labels_in / held_in / labels_out / held_out / n_moved) and the last step's outputs.  The recount rule is refine()'s over the
    effective classes: n_moved counts the cells whose label or held flag changed."""
    if min_loci < 1:
        raise ValueError("min_loci must be at least 1")
    if not 0.0 <= doublet_threshold <= 1.0:
        raise ValueError("doublet_threshold must lie within [0, 1]")
    labels = check_labels(labels, n_classes).copy()
    held = np.zeros(len(labels), np.uint8) if held is None else (np.asarray(held) != 0).astype(np.uint8)
    summ = dict(iterations=0, converged=0, n_moved_last=0, n_moved_total=0, n_recounts=0)
    steps, n_moved = [], 0
    while True:
        sizes = np.bincount(effective_labels(labels, held, n_classes), minlength=n_classes + 1)
        if _recount_rule(len(steps), class_delta, n_moved, sizes):
            summ["n_recounts"] += 1
        st = doublet_posteriors(n_loci, coo, labels, n_classes, ll_fn, held, scale, pair_scale, log_prior, log_pair_prior, mask)
        st["labels_in"], st["held_in"] = labels.copy(), held.copy()
        steps.append(st)
        if max_iter == 0:
            st["labels_out"], st["held_out"], st["n_moved"] = labels.copy(), held.copy(), 0
            break
        move = (labels != UNLABELLED) & (st["loci_used"].astype(np.uint64) >= np.uint64(min_loci))
        new = np.where(move, st["best"], labels).astype(np.uint8)
        new_held = np.where(move, st["doublet_posterior"] > doublet_threshold, held != 0).astype(np.uint8)
        n_moved = int(((new != labels) | (new_held != held)).sum())
        labels, held = new, new_held
        st["labels_out"], st["held_out"], st["n_moved"] = labels.copy(), held.copy(), n_moved
        summ["iterations"] += 1
        summ["n_moved_last"] = n_moved
        summ["n_moved_total"] += n_moved
        if n_moved == 0:
            summ["converged"] = 1
            break
        if summ["iterations"] == max_iter:
            break
    cc = np.zeros(16, np.uint64)
    cc[:n_classes] = class_sizes(_unheld(labels, held), n_classes)
    summ["class_cells"] = cc
    summ["n_held"] = int(((held != 0) & (labels != UNLABELLED)).sum())
    last = steps[-1]
    out = dict(labels=labels, held=held, summary=summ, steps=steps)
    out.update({k: last[k] for k in ("ll", "ll_pair", "posterior", "doublet_posterior", "best", "best_pair", "call", "qual")})
    return out
