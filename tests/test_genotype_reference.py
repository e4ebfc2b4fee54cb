"""CPU checks behind cellector_class_genotypes: genotype_host.h compiled as plain C++ on the host, its numpy twin
(cellector_amd.genotypes) and the oracle's orc_vcf_genotype.

Header and twin are compared with == (NaN equal to NaN) for gt, gp and gp3 at every setting; at the reference's ambient = 0.03,
threshold = 0.99 both are compared with the oracle's minority output for vcf_genotype(a, r, A - a, R - r).  The twin's tallies are
compared with classes.class_tallies at the used loci and, for K = 2, with the oracle's final_tallies_coo.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from cellector_amd import classes as cl
from cellector_amd import genotypes as gn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cellector_amd", "csrc")

DRIVER = r"""
#include <cstdint>
#include "genotype_host.h"

// (a, r) = the class' tallies, (A, R) = the locus' totals over all slots
extern "C" void genotype_batch(const uint64_t *a, const uint64_t *r, const uint64_t *A, const uint64_t *R, int64_t n, double ambient,
                               double threshold, uint8_t *gt, double *gp, double *gp3)
{
    for (int64_t i = 0; i < n; i++) {
        const GenotypeLocus g = genotype_locus(A[i], R[i], ambient);
        const GenotypeCall q = genotype_call(g, a[i], r[i], threshold);
        gt[i] = q.gt;
        gp[i] = q.gp;
        for (int j = 0; j < 3; j++) gp3[3 * i + j] = q.q[j];
    }
}
extern "C" const char *genotype_name(uint8_t gt) { return genotype_string(gt); }
"""


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    if not cxx:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("genotype_reference")
    src, so = d / "driver.cpp", d / "libdrv.so"
    src.write_text(DRIVER)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fno-fast-math", "-ffp-contract=off", "-fPIC", "-shared", "-I", CSRC, str(src),
                           "-o", str(so), "-lm"])
    L = C.CDLL(str(so))
    vp = C.c_void_p
    L.genotype_batch.restype = None
    L.genotype_batch.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_double, C.c_double, vp, vp, vp]
    L.genotype_name.restype = C.c_char_p
    L.genotype_name.argtypes = [C.c_uint8]
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _header(drv, cases, ambient, thr):
    a, r, A, R = (np.ascontiguousarray([c[j] for c in cases], np.uint64) for j in range(4))
    n = len(cases)
    gt, gp, gp3 = np.zeros(n, np.uint8), np.zeros(n), np.zeros((n, 3))
    drv.genotype_batch(_p(a), _p(r), _p(A), _p(R), n, ambient, thr, _p(gt), _p(gp), _p(gp3))
    return gt, gp, gp3


def _twin(cases, ambient, thr):
    n = len(cases)
    gt, gp, gp3 = np.zeros(n, np.uint8), np.zeros(n), np.zeros((n, 3))
    for i, (a, r, A, R) in enumerate(cases):
        gt[i], gp[i], gp3[i] = gn.genotype_call(gn.locus_probabilities(A, R, ambient), a, r, thr)
    return gt, gp, gp3


def _same(x, y):
    return np.array_equal(x, y, equal_nan=True)


DEPTHS = (0, 1, 170, 171, 172, 1000, 10_000, 100_000, 1_000_000, 3_000_000)
RESTS = ((0, 0), (5_000_000, 5_000_000), (10_000_000, 0), (0, 10_000_000), (3, 1_000_000))
UNDERFLOW = (750_000, 2_250_000, 750_000, 2_250_000)  # a quarter alt at depth 3e6: far from all three genotypes
NO_READS = (0, 0, 1234, 4321)


def _grid():
    cases = []
    for n in DEPTHS:
        for a in sorted({0, n, n // 2, n // 4, n // 100}):
            for ra, rr in RESTS:
                cases.append((a, n - a, a + ra, n - a + rr))
    return cases + [UNDERFLOW, NO_READS]


def test_header_twin_and_oracle_at_the_reference_settings(drv, oracle_lib):
    cases = _grid()
    hg, hp, h3 = _header(drv, cases, 0.03, 0.99)
    tg, tp, t3 = _twin(cases, 0.03, 0.99)
    assert _same(hg, tg) and _same(hp, tp) and _same(h3, t3)
    for i, (a, r, A, R) in enumerate(cases):
        _, _, og, op = oracle_lib.vcf_genotype(a, r, A - a, R - r)
        assert og == hg[i] and (op == hp[i] or (op != op and hp[i] != hp[i])), (cases[i], og, op, hg[i], hp[i])
    # the reference's quirk: all three pmfs underflow, den = 0, every q is 0 / 0
    u = cases.index(UNDERFLOW)
    assert np.isnan(hp[u]) and np.isnan(h3[u]).all() and hg[u] == 0
    # a class without reads: three pmfs of 1
    z = cases.index(NO_READS)
    assert hp[z] == 1.0 / 3.0 and hg[z] == 0 and (h3[z] == 1.0 / 3.0).all()
    # the grid reaches every call
    assert set(hg.tolist()) == {0, 1, 2, 3}
    assert [drv.genotype_name(g).decode() for g in range(4)] == list(gn.GT_STRINGS)


@pytest.mark.parametrize("ambient,thr", [(0.0, 0.99), (1.0, 0.99), (0.03, 0.5), (0.03, 1.0), (0.5, 0.0)])
def test_header_equals_twin_at_other_settings(drv, ambient, thr):
    cases = _grid()
    if ambient == 1.0:  # p = soup: soup 0 is the p == 0 branch, soup 1 the p ~ 1 branch of the pmf
        cases += [(0, 5, 0, 40), (2, 3, 0, 40), (5, 0, 40, 0), (2, 3, 40, 0), (0, 0, 0, 9), (0, 0, 9, 0)]
    hg, hp, h3 = _header(drv, cases, ambient, thr)
    tg, tp, t3 = _twin(cases, ambient, thr)
    assert _same(hg, tg) and _same(hp, tp) and _same(h3, t3)
    # (thr = 1 still calls: l / 3 / (1/3 * l) can round to the double above 1, in the reference as here)


def test_genotype_posteriors_is_the_rule_per_slot():
    alt = np.array([[3, 0, 40], [0, 0, 1], [9, 0, 2]], np.uint64)  # K = 2 and the unlabelled slot
    ref = np.array([[0, 0, 41], [30, 0, 0], [1, 0, 5]], np.uint64)
    gt, gp, gp3 = gn.genotype_posteriors(alt, ref)
    assert gt.shape == (2, 3) and gp3.shape == (2, 3, 3)
    for k in range(2):
        for t in range(3):
            p3 = gn.locus_probabilities(alt[:, t].sum(), ref[:, t].sum())
            g, p, q = gn.genotype_call(p3, alt[k, t], ref[k, t])
            assert gt[k, t] == g and gp[k, t] == p and tuple(gp3[k, t]) == q
    assert gp[0, 1] == 1.0 / 3.0 and gt[1, 0] == 3 and gt[0, 2] == 2


def _matrix():
    rng = np.random.default_rng(5)
    TL, N, n = 60, 50, 900
    lo, ce = rng.integers(0, TL, n), rng.integers(0, N, n)  # (repeated pairs included)
    al, re = rng.integers(0, 4, n), rng.integers(0, 4, n)
    al[lo < 12] = 0                     # loci that fail min_alt ...
    re[(lo >= 12) & (lo < 20)] = 0      # ... and min_ref, with reads of the other allele
    return TL, N, (lo.astype(np.uint32), ce.astype(np.uint32), al.astype(np.uint32), re.astype(np.uint32))


def test_twin_tallies_against_class_tallies_and_the_oracle(oracle_lib):
    TL, N, coo = _matrix()
    rng = np.random.default_rng(6)
    orc = oracle_lib.Oracle.from_coo(TL, N, *coo, 4, 4)
    tot_a, tot_r = np.bincount(coo[0], coo[2], TL), np.bincount(coo[0], coo[3], TL)
    used = np.nonzero((tot_a >= 4) & (tot_r >= 4))[0]
    assert orc.locus_ids().tolist() == used.tolist()
    assert 0 < len(used) < TL - 15
    for K in (1, 3, 16):
        lab = rng.integers(0, K, N).astype(np.uint8)
        lab[rng.random(N) < 0.2] = 255
        lab[0] = 0
        cells, alt, ref = gn.class_genotype_tallies(TL, coo, lab, K)
        assert cells.dtype == np.uint64 and alt.shape == (K + 1, TL)
        assert cells[:K].tolist() == cl.class_sizes(lab, K).tolist() and cells[K] == (lab == 255).sum()
        assert (alt.sum(axis=0) == tot_a).all() and (ref.sum(axis=0) == tot_r).all()
        assert alt[:, :20].any() and ref[:, :20].any()  # the loci that failed the filter carry their reads
        # the used-locus COO of the same matrix
        idx = np.full(TL, -1)
        idx[used] = np.arange(len(used))
        sel = idx[coo[0]] >= 0
        ucoo = (idx[coo[0]][sel], coo[1][sel], coo[2][sel], coo[3][sel])
        c2, a2, r2 = cl.class_tallies(len(used), ucoo, lab, K)
        assert (alt[:K, used] == a2).all() and (ref[:K, used] == r2).all() and (cells[:K] == c2).all()
    # K = 2 by an exclusion set: the oracle's load_mtx_final
    excl = (rng.random(N) < 0.3).astype(np.uint8)
    cells, alt, ref = gn.class_genotype_tallies(TL, coo, 1 - excl, 2)
    want = oracle_lib.final_tallies_coo(TL, *coo, excl)
    assert (alt[0] == want["alt_min"]).all() and (ref[0] == want["ref_min"]).all()
    assert (alt[1] == want["alt_maj"]).all() and (ref[1] == want["ref_maj"]).all() and not alt[2].any() and not ref[2].any()


def test_concordance_on_a_hand_written_gt():
    gt = np.array([[1, 2, 0, 3, 3, 0],
                   [1, 3, 2, 3, 0, 0],
                   [0, 0, 0, 0, 0, 0]], np.uint8)
    both, disc = gn.concordance(gt)
    assert both.dtype.kind == "i" and both.shape == (3, 3)
    assert both.tolist() == [[4, 3, 0], [3, 4, 0], [0, 0, 0]]
    assert disc.tolist() == [[0, 1, 0], [1, 0, 0], [0, 0, 0]]
