"""Donor genotype refinement on host arrays: the numpy twin of cellector_donor_genotypes (include/cellector_ffi.h states the model;
csrc/kernels_donor_genotypes.hip runs it).

The reads of the cells called for a donor, tallied over ALL loci of the matrix, say what that donor's genotype is at every covered
locus: per (donor, locus) a posterior over the three genotypes from the binomial terms of the donor model and the floored prior of
the donor's own VCF row, a call above gt_threshold, and a kind (confirmed, filled, changed, withdrawn) against the prior's call.

The tallies are integer sums and equal the device's exactly.  Every operation of the model that is not a log or an exp is one rounded
IEEE operation and is repeated here in the model's order: fed the DEVICE's tab (la, lb) the terms lam_g carry the device's bits, and
q differs from the device's only through numpy's log(v_g) and exp, by a few ulps.  gt_out and kind follow exactly from q.

Helpers: prior_from_gt (one-hot rows of hard calls), to_gp (q as the float32 rows cellector_donor_posteriors_gp takes), render_vcf /
render_tsv (the host binary's two files).
"""
import numpy as np

NO_CALL = 3
NONE = 255
KIND_NONE, CONFIRMED, FILLED, CHANGED, WITHDRAWN = 0, 1, 2, 3, 4
KIND_NAMES = {KIND_NONE: "no_reads", CONFIRMED: "confirmed", FILLED: "filled", CHANGED: "changed", WITHDRAWN: "withdrawn"}
DEFAULTS = dict(err=0.01, ambient=0.03, gt_threshold=0.99, prior_floor=0.01)
GT_STRINGS = {0: "0/0", 1: "0/1", 2: "1/1", 3: "./."}


def _params(params):
    p = dict(DEFAULTS)
    for k, v in params.items():
        if k not in p:
            raise TypeError(f"unknown parameter {k!r}")
        p[k] = float(v)
    return p


def prior_from_gt(gt):
    """prior [D, total_loci, 3] float32 from hard calls gt [D, total_loci] (0 = 0/0, 1 = 0/1, 2 = 1/1, 3 = no call): one-hot rows, three
    NaN for code 3"""
    gt = np.asarray(gt)
    if gt.ndim != 2 or (gt > 3).any():
        raise ValueError("gt: shape (D, total_loci) with codes 0..3 expected")
    out = np.zeros(gt.shape + (3,), np.float32)
    for g in range(3):
        out[..., g] = gt == g
    out[gt == NO_CALL] = np.nan
    return out


def to_gp(q):
    """q [D, total_loci, 3] as the float32 rows cellector_donor_posteriors_gp takes.  A q_g below float32's range rounds to 0 and the
    genotype leaves the row's support, as a one-hot row's other genotypes do; every row keeps its largest weight (>= 1/3)."""
    return np.ascontiguousarray(q, dtype=np.float32)


def tallies(total_loci, coo, assign, n_donors):
    """(cells [D + 1], alt [D + 1, total_loci], ref [D + 1, total_loci]) uint64 from the entries coo = (locus, cell, alt, ref) of the
    staged matrix in any order: slot D holds the cells assigned 255"""
    lo, ce, al, re = (np.asarray(x) for x in coo)
    assign = np.asarray(assign, np.uint8)
    D, TL = int(n_donors), int(total_loci)
    slot = np.where(assign == NONE, D, assign).astype(np.int64)
    if (slot > D).any():
        raise ValueError(f"assign: a value that is neither below the {D} donors nor 255")
    alt, ref = np.zeros((D + 1, TL), np.uint64), np.zeros((D + 1, TL), np.uint64)
    s = slot[ce.astype(np.int64)]
    np.add.at(alt, (s, lo.astype(np.int64)), al.astype(np.uint64))
    np.add.at(ref, (s, lo.astype(np.int64)), re.astype(np.uint64))
    return np.bincount(slot, minlength=D + 1).astype(np.uint64), alt, ref


def tables(alt, ref, err=0.01, ambient=0.03, log=np.log):
    """tab [total_loci, 3, 2] = (log theta_g, log(1 - theta_g)) from the planes alt, ref [D + 1, total_loci]: step 2 of the model"""
    A, R = np.asarray(alt, np.uint64).sum(axis=0), np.asarray(ref, np.uint64).sum(axis=0)
    soup = (A.astype(np.float64) + 1.0) / ((A + R).astype(np.float64) + 2.0)
    keep, amb = 1.0 - ambient, ambient * soup
    e = np.array([err, 0.5, 1.0 - err])
    th = (keep * e)[None, :] + amb[:, None]
    return np.stack([log(th), log(1.0 - th)], axis=-1)


def weights(prior, D, total_loci):
    """(w [D, total_loci, 3] float64, prior_call [D, total_loci] uint8) from prior [D, total_loci, 3] or None: a no-call row has 1/3
    each and prior_call 3"""
    third = 1.0 / 3.0
    if prior is None:
        return np.full((D, total_loci, 3), third), np.full((D, total_loci), NO_CALL, np.uint8)
    p = np.asarray(prior, np.float32)
    if p.shape != (D, total_loci, 3):
        raise ValueError(f"prior: shape ({D}, {total_loci}, 3) expected, got {p.shape}")
    none = np.isnan(p).all(axis=2)
    fine = np.isfinite(p).all(axis=2) & (p >= 0).all(axis=2) & (p > 0).any(axis=2)
    if (~(none | fine)).any():
        d, t = np.argwhere(~(none | fine))[0]
        raise ValueError(f"prior of donor {d} at locus {t}: three NaN (no call), or three finite weights >= 0 that are not all zero")
    x = np.where(none[..., None], 1.0, p.astype(np.float64))
    w = x / ((x[..., 0] + x[..., 1]) + x[..., 2])[..., None]
    w = np.where(none[..., None], third, w)
    call = np.where(none, NO_CALL, _argmax_first(w)).astype(np.uint8)
    return w, call


def _argmax_first(v):
    return np.argmax(v, axis=-1)  # (numpy returns the first of equal maxima)


def posterior(alt, ref, tab, prior=None, log=np.log, exp=np.exp, **params):
    """dict of q [D, total_loci, 3], gt_out, kind [D, total_loci] uint8 and lam, x (the terms) from the planes alt, ref [D + 1,
    total_loci], tab [total_loci, 3, 2] (the device's, for its bits in lam) and the prior: steps 3 and 4 of the model"""
    prm = _params(params)
    alt, ref = np.asarray(alt, np.uint64), np.asarray(ref, np.uint64)
    D, TL = alt.shape[0] - 1, alt.shape[1]
    tab = np.asarray(tab, np.float64)
    w, prior_call = weights(prior, D, TL)
    a, r = alt[:D].astype(np.float64), ref[:D].astype(np.float64)
    lam = (a[..., None] * tab[None, :, :, 0]) + (r[..., None] * tab[None, :, :, 1])
    v = ((1.0 - prm["prior_floor"]) * w) + (prm["prior_floor"] / 3.0)
    part = v != 0.0
    with np.errstate(divide="ignore"):
        x = np.where(part, lam + log(np.where(part, v, 1.0)), -np.inf)
    m = x.max(axis=2)
    e = np.where(part, exp(x - m[..., None]), 0.0)
    den = np.zeros_like(m)
    for g in range(3):
        den = den + e[..., g]
    q = e / den[..., None]
    gt_out, kind = calls(q, alt[:D] + ref[:D], prior_call, prm["gt_threshold"])
    return dict(q=q, gt_out=gt_out, kind=kind, lam=lam, x=x, w=w, v=v, prior_call=prior_call)


def calls(q, depth, prior_call, gt_threshold=0.99):
    """(gt_out, kind) uint8 from q, the depth a + r and the prior's call: the rule of steps 3 and 4, exact given its inputs"""
    call = _argmax_first(q)
    top = np.take_along_axis(q, call[..., None], axis=2)[..., 0]
    gt_out = np.where(top > gt_threshold, call, NO_CALL).astype(np.uint8)
    kind = np.where(np.asarray(depth) == 0, KIND_NONE,
                    np.where(gt_out == NO_CALL, WITHDRAWN,
                             np.where(prior_call == NO_CALL, FILLED, np.where(gt_out == prior_call, CONFIRMED, CHANGED)))).astype(np.uint8)
    return gt_out, kind


def summary(cells, kind):
    """the per-donor counts of step 5 as a dict of [D] arrays"""
    kind = np.asarray(kind)
    D = kind.shape[0]
    out = dict(cells=np.asarray(cells, np.uint64)[:D].copy(), loci_with_reads=(kind != KIND_NONE).sum(axis=1).astype(np.uint64))
    for name, k in (("confirmed", CONFIRMED), ("filled", FILLED), ("changed", CHANGED), ("withdrawn", WITHDRAWN)):
        out[name] = (kind == k).sum(axis=1).astype(np.uint64)
    return out


def donor_genotypes(total_loci, coo, assign, n_donors, prior=None, tab=None, **params):
    """cellector_donor_genotypes on host arrays; tab: the device's table for its bits in lam, None = numpy's.  Returns the dict of
    Cellector.donor_genotypes (summary: a dict)."""
    prm = _params(params)
    cells, alt, ref = tallies(total_loci, coo, assign, n_donors)
    if tab is None:
        tab = tables(alt, ref, prm["err"], prm["ambient"])
    out = posterior(alt, ref, tab, prior, **prm)
    out.update(cells=cells, alt=alt, ref=ref, tab=tab, summary=summary(cells, out["kind"]))
    return out


# ---- the host binary's two files ----------------------------------------------------------------------------------------------
def _num(x):
    """a probability as the host binary prints it: the shortest digits that read back, positional, whole values without '.0'"""
    from decimal import Decimal
    s = format(Decimal(repr(float(x))), "f")
    return s[:-2] if s.endswith(".0") else s


def render_vcf_columns(gt_out, q, alt, ref, fmt=_num):
    """per locus the D sample columns GT:GP:AO:RO of cellector_donor_genotypes.vcf, as a list of lists of strings"""
    D, TL = gt_out.shape
    return [["%s:%s,%s,%s:%d:%d" % (GT_STRINGS[int(gt_out[d, t])], fmt(float(q[d, t, 0])), fmt(float(q[d, t, 1])), fmt(float(q[d, t, 2])),
                                    int(alt[d, t]), int(ref[d, t])) for d in range(D)] for t in range(TL)]


def render_tsv(names, s):
    """cellector_donor_genotypes.tsv from the summary dict: one row per donor"""
    cols = ("cells", "loci_with_reads", "confirmed", "filled", "changed", "withdrawn")
    lines = ["donor\t" + "\t".join(cols)]
    for d, name in enumerate(names):
        lines.append(name + "\t" + "\t".join(str(int(s[c][d])) for c in cols))
    return "\n".join(lines) + "\n"
