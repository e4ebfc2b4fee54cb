"""Class genotypes on host arrays: the numpy twin of cellector_class_genotypes (include/cellector_ffi.h states the model;
csrc/kernels_genotypes.hip counts, csrc/genotype_host.h calls).

The tallies are integers and the library's own.  The genotype rule repeats genotype_host.h operation by operation in Python
floats (IEEE doubles, no contraction) on math.exp / math.log, the C library's as in the header, so gt, gp and gp3 are the
header's bits, NaN where it gives NaN.
"""
import math

import numpy as np

from .classes import UNLABELLED, class_sizes

GT_STRINGS = ("./.", "1/1", "0/1", "0/0")  # by the code in gt

_DK = (2.48574089138753565546e-5, 1.05142378581721974210, -3.45687097222016235469, 4.51227709466894823700, -2.98285225323576655721,
       1.05639711577126713077, -1.95428773191645869583e-1, 1.70970543404441224307e-2, -5.71926117404305781283e-4,
       4.63399473359905636708e-6, -2.71994908488607703910e-9)
_FCACHE = [1.0]
for _i in range(1, 171):
    _FCACHE.append(_FCACHE[-1] * float(_i))


def donor_codes(gt):
    """the codes of cellector_class_genotypes' gt (1 = 1/1, 2 = 0/1, 3 = 0/0, 0 = ./.) in the coding of the donor and the ambient calls
    (2 = 1/1, 1 = 0/1, 0 = 0/0, 3 = no call), uint8 of the same shape"""
    return np.array([3, 2, 1, 0], np.uint8)[np.asarray(gt, np.int64)]


def class_genotype_tallies(total_loci, coo, labels, n_classes):
    """(cells [K + 1], alt [K + 1, total_loci], ref [K + 1, total_loci]) uint64 from the all-loci COO arrays (locus, cell, alt,
    ref), e.g. Cellector.staged_coo(): per slot the sums of the allele counts of its cells' entries; slot K = the cells labelled
    255; a repeated (locus, cell) pair counts each time"""
    lo, ce, al, re = (np.asarray(x, np.int64) for x in coo)
    labels = np.asarray(labels)
    K = int(n_classes)
    slot = np.where(labels == UNLABELLED, K, labels).astype(np.int64)
    alt = np.zeros((K + 1, total_loci), np.uint64)
    ref = np.zeros((K + 1, total_loci), np.uint64)
    s = slot[ce]
    np.add.at(alt, (s, lo), al.astype(np.uint64))
    np.add.at(ref, (s, lo), re.astype(np.uint64))
    cells = np.concatenate([class_sizes(labels, K), np.array([(labels == UNLABELLED).sum()], np.uint64)]).astype(np.uint64)
    return cells, alt, ref


def ln_gamma(x):
    s = _DK[0]
    for i in range(1, 11):
        s += _DK[i] / (x + float(i) - 1.0)
    return math.log(s) + 0.6207822376352452223455184457816472122518527279025978 + \
        (x - 0.5) * math.log((x - 0.5 + 10.900511) / 2.71828182845904523536028747135266250)


def ln_factorial(x):
    return math.log(_FCACHE[x]) if x <= 170 else ln_gamma(float(x) + 1.0)


def binomial_pmf(p, n, k):
    if k > n:
        return 0.0
    if p == 0.0:
        return 1.0 if k == 0 else 0.0
    if abs(p - 1.0) <= 4 * 2.220446049250313e-16:
        return 1.0 if k == n else 0.0
    lnb = ln_factorial(n) - ln_factorial(k) - ln_factorial(n - k)
    return math.exp(lnb + float(k) * math.log(p) + float(n - k) * math.log(1.0 - p))


def _div(x, y):  # IEEE division of a non-negative x (Python raises on a zero divisor)
    if y == 0.0:
        return math.nan if (x == 0.0 or x != x) else math.inf
    return x / y


def _fmax(a, b):  # C's fmax: a NaN loses against a number
    if a != a:
        return b
    if b != b:
        return a
    return max(a, b)


def locus_probabilities(total_alt, total_ref, ambient=0.03):
    """(p_hom_alt, p_het, p_hom_ref): a read's alt probability under each genotype with `ambient` of the reads from the soup"""
    total_alt, total_ref = int(total_alt), int(total_ref)
    soup = float(total_alt) / float(total_alt + total_ref) if total_alt + total_ref > 0 else 0.5
    return ((1.0 - ambient) * 0.99 + ambient * soup, (1.0 - ambient) * 0.5 + ambient * soup, (1.0 - ambient) * 0.01 + ambient * soup)


def genotype_call(p3, alt, ref, gt_threshold=0.99):
    """(gt, gp, (q_alt, q_het, q_ref)) of one class at one locus under the locus' p3 = locus_probabilities(...)"""
    alt, ref = int(alt), int(ref)
    l_alt, l_het, l_ref = (binomial_pmf(p, alt + ref, alt) for p in p3)
    den = 1.0 / 3.0 * l_alt + 1.0 / 3.0 * l_het + 1.0 / 3.0 * l_ref
    q = (_div(l_alt * 1.0 / 3.0, den), _div(l_het * 1.0 / 3.0, den), _div(l_ref * 1.0 / 3.0, den))
    gp = _fmax(_fmax(q[0], q[1]), q[2])
    gt = 1 if q[0] > gt_threshold else 2 if q[1] > gt_threshold else 3 if q[2] > gt_threshold else 0
    return gt, gp, q


def genotype_posteriors(alt, ref, ambient=0.03, gt_threshold=0.99):
    """(gt [K, T] uint8, gp [K, T], gp3 [K, T, 3]) from the tallies alt / ref [K + 1, T] of class_genotype_tallies: the soup of a
    locus is formed over all K + 1 slots, the calls are those of the first K"""
    alt, ref = np.asarray(alt, np.uint64), np.asarray(ref, np.uint64)
    K, T = alt.shape[0] - 1, alt.shape[1]
    gt, gp, gp3 = np.zeros((K, T), np.uint8), np.zeros((K, T), np.float64), np.zeros((K, T, 3), np.float64)
    tot_a, tot_r = alt.sum(axis=0, dtype=np.uint64), ref.sum(axis=0, dtype=np.uint64)
    for t in range(T):
        p3 = locus_probabilities(tot_a[t], tot_r[t], ambient)
        for k in range(K):
            gt[k, t], gp[k, t], gp3[k, t] = genotype_call(p3, alt[k, t], ref[k, t], gt_threshold)
    return gt, gp, gp3


def concordance(gt):
    """(both_called [K, K], discordant [K, K]) int64 from gt [K, T]: per pair of classes the loci where both have a call
    (gt != 0), and of those the loci where the calls differ"""
    gt = np.asarray(gt)
    called = gt != 0
    both = (called[:, None, :] & called[None, :, :])
    diff = both & (gt[:, None, :] != gt[None, :, :])
    return both.sum(axis=2).astype(np.int64), diff.sum(axis=2).astype(np.int64)
