"""CPU: the doublet bindings exist with the header's signatures, and the doublet half of cellector_amd.classes (the numpy twin) on
its own: pair_index, K = 1, a dead pair, ties go to the lowest p, a doublet posterior of exactly 0.5 is no call, rest == 0 gives
qual 255, a held cell is in no tally and is still scored, the default scales and priors, the effective-class recount rule."""
import ctypes
import math

import numpy as np
import pytest

from cellector_amd import classes as cl
from cellector_amd import ffi


def test_bindings(hip_lib_path):
    lib = ffi.load_library(hip_lib_path)
    for name, nargs in (("cellector_class_pair_alpha_betas", 7), ("cellector_class_doublets", 17), ("cellector_refine_class_doublets", 19)):
        assert hasattr(lib, name) and len(ffi.SIGNATURES[name][1]) == nargs
    for m in ("class_pair_alpha_betas", "class_doublets", "refine_class_doublets"):
        assert callable(getattr(ffi.Cellector, m))
    S = ffi.RefineDoubletsSummary
    assert ctypes.sizeof(S) == ctypes.sizeof(ffi.RefineSummary) + 8 == 8 + 3 * 8 + 16 * 8 + 8
    assert S.class_cells.offset == ffi.RefineSummary.class_cells.offset == 32 and S.n_held.offset == 160
    for f in ("iterations", "converged", "n_moved_last", "n_moved_total", "n_recounts"):
        assert getattr(S, f).offset == getattr(ffi.RefineSummary, f).offset
    assert ffi.SIGNATURES["cellector_refine_class_doublets"][1][9] is ctypes.c_double
    # a null ctx is refused without touching anything
    assert lib.cellector_class_pair_alpha_betas(None, None, None, 2, None, None, None) == 1
    assert lib.cellector_class_doublets(None, None, None, 2, *([None] * 13)) == 1
    assert lib.cellector_refine_class_doublets(None, None, None, 2, None, None, None, None, None, 0.5, 1, 1, *([None] * 7)) == 1


def test_pair_index():
    for K in (2, 3, 16):
        ps = cl.pairs(K)
        assert len(ps) == cl.n_pairs(K) == K * (K - 1) // 2
        assert [cl.pair_index(K, a, b) for a, b in ps] == list(range(len(ps)))
        assert ps == sorted(ps)
    assert cl.pair_index(2, 0, 1) == 0 and cl.pair_index(3, 1, 2) == 2 and cl.pair_index(16, 14, 15) == 119 and cl.pair_index(16, 1, 2) == 15
    assert cl.n_pairs(1) == 0 and cl.pairs(1) == []
    for bad in ((1, 1), (2, 1), (0, 3), (-1, 2)):
        with pytest.raises(ValueError):
            cl.pair_index(3, *bad)


COO = (np.array([0, 0, 1, 1, 2, 2, 2]), np.array([0, 1, 0, 2, 1, 2, 2]), np.array([3, 0, 1, 2, 0, 5, 1]), np.array([0, 2, 1, 0, 4, 0, 1]))


def _flat(alpha, beta, mask):
    return np.zeros(4), np.array([2.0, 2.0, 3.0, 0.0])


def test_k1_has_no_pair():
    one = cl.doublet_chain(np.array([[-3.0, 0.0, -700.0]]), np.zeros((0, 3)), [0.0], [], [True])
    assert (one["posterior"] == 1.0).all() and (one["doublet_posterior"] == 0.0).all() and (one["call"] == 0).all()
    assert (one["best_pair"] == 255).all() and (one["qual"] == 255).all() and (one["best"] == 0).all()
    out = cl.doublet_posteriors(3, COO, [0, 0, 0, 255], 1, _flat)
    assert out["ll_pair"].shape == (0, 4) and (out["doublet_posterior"] == 0).all() and (out["best_pair"] == 255).all()


def test_dead_pair_ties_and_the_strict_call():
    # class 1 is dead: pairs (0, 1) and (1, 2) are dead whatever their columns hold, (0, 2) is the one live pair
    ll = np.array([[0.0, -4.0], [9.0, 9.0], [-2.0, 0.0]])
    llp = np.array([[50.0, 50.0], [-1.0, -3.0], [50.0, 50.0]])
    out = cl.doublet_chain(ll, llp, [0.0] * 3, [0.0] * 3, [True, False, True])
    assert out["pair_live"].tolist() == [False, True, False] and (out["best_pair"] == [0, 2]).all()
    assert (out["posterior"][1] == 0).all() and out["best"].tolist() == [0, 2]
    want = math.exp(-1.0) / (1.0 + math.exp(-2.0) + math.exp(-1.0))
    assert abs(out["doublet_posterior"][0] - want) <= 4e-16 and out["call"].tolist() == [0, 0]
    # ties: the lowest k and the lowest p
    tie = cl.doublet_chain(np.zeros((3, 1)), np.full((3, 1), -1.0), [0.0] * 3, [0.0] * 3, [True] * 3)
    assert tie["best"][0] == 0 and tie["best_pair"][0].tolist() == [0, 1]
    tie = cl.doublet_chain(np.zeros((3, 1)), np.array([[-2.0], [-1.0], [-1.0]]), [0.0] * 3, [0.0] * 3, [True] * 3)
    assert tie["best_pair"][0].tolist() == [0, 2]
    # one singlet and one pair of equal weight: doublet_posterior is exactly 0.5, which is no call (main.rs:150 is strict)
    half = cl.doublet_chain(np.array([[0.0], [-800.0]]), np.array([[0.0]]), [0.0, 0.0], [0.0], [True, True])
    assert half["doublet_posterior"][0] == 0.5 and half["call"][0] == 0 and half["qual"][0] == 3
    over = cl.doublet_chain(np.array([[0.0], [-800.0]]), np.array([[1e-9]]), [0.0, 0.0], [0.0], [True, True])
    assert over["doublet_posterior"][0] > 0.5 and over["call"][0] == 1 and over["qual"][0] == 3  # (rest = the singlets' sum)
    # rest == 0: a singlet that takes everything, and a doublet that does
    sat = cl.doublet_chain(np.array([[0.0], [-800.0]]), np.array([[-900.0]]), [0.0, 0.0], [0.0], [True, True])
    assert sat["rest"][0] == 0.0 and sat["qual"][0] == 255 and sat["call"][0] == 0 and sat["posterior"][0, 0] == 1.0
    dbl = cl.doublet_chain(np.array([[-800.0], [-900.0]]), np.array([[0.0]]), [0.0, 0.0], [0.0], [True, True])
    assert dbl["rest"][0] == 0.0 and dbl["qual"][0] == 255 and dbl["call"][0] == 1 and dbl["doublet_posterior"][0] == 1.0


def test_a_held_cell_is_in_no_tally_and_is_scored():
    lab = np.array([0, 2, 2, 255], np.uint8)
    held = np.array([0, 0, 1, 0], np.uint8)
    out = cl.doublet_posteriors(3, COO, lab, 3, _flat, held=held)
    assert out["cells"].tolist() == [1, 0, 1]
    # cell 2's entries (locus 1: 2 / 0; locus 2: 5 / 0 and 1 / 1) are in no class
    assert out["alt"].tolist() == [[3, 1, 0], [0, 0, 0], [0, 0, 0]] and out["ref"].tolist() == [[0, 1, 0], [0, 0, 0], [2, 0, 4]]
    assert np.isfinite(out["posterior"][:, 2]).all() and abs(out["posterior"][:, 2].sum() + out["doublet_posterior"][2] - 1.0) < 1e-15
    assert cl.effective_labels(lab, held, 3).tolist() == [0, 2, 3, 3]
    with pytest.raises(ValueError, match="every labelled cell is held"):
        cl.doublet_posteriors(3, COO, lab, 3, _flat, held=[1, 1, 1, 0])
    # pair distributions: two rounded products, a rounded sum, + 1
    a, b = cl.class_pair_alpha_betas(out["alt"], out["ref"], [0.3, 1.0, 0.7])
    assert a[cl.pair_index(3, 0, 2)].tolist() == [(3 * 0.3 + 0 * 0.7) + 1.0, (1 * 0.3 + 0.0) + 1.0, 1.0]
    assert b[cl.pair_index(3, 0, 2)].tolist() == [(0 * 0.3 + 2 * 0.7) + 1.0, (1 * 0.3 + 0 * 0.7) + 1.0, (0 * 0.3 + 4 * 0.7) + 1.0]


def test_default_scales_and_priors():
    assert cl.balanced_pair_scales([700, 200, 0, 100]).tolist() == [100.0 / 700.0, 100.0 / 200.0, 0.0, 1.0]
    f = cl.class_fractions([700, 200, 100])
    assert f.tolist() == [701.0 / 1003.0, 201.0 / 1003.0, 101.0 / 1003.0]
    lpp = cl.default_log_pair_priors([700, 200, 100], 1060)
    rate = 1060.0 / 1000.0 / 100.0
    assert lpp.tolist() == [math.log(rate * f[1]), math.log(rate * f[2]), math.log(rate * f[2])]
    # the floor of main.rs:259: a class below 10 % counts as 10 %
    assert cl.default_log_pair_priors([950, 50], 1000)[0] == math.log(1000.0 / 1000.0 / 100.0 * 0.1)
    ps, lpp = cl.reference_doublet_scales(69, 999)
    assert ps.tolist() == [1.0, 0.07] and lpp.tolist() == [math.log(999 / 1000.0 / 100.0 * 0.1)]
    ps, lpp = cl.reference_doublet_scales(0, 999)
    assert ps[1] == 1.0 / 1000.0  # (unclamped, unlike reference_scales)
    ps, lpp = cl.reference_doublet_scales(499, 999)
    assert lpp[0] == math.log(999 / 1000.0 / 100.0 * 0.5)


def test_refine_driver():
    with pytest.raises(ValueError):
        cl.refine_doublets(3, COO, [0, 1, 1, 255], 2, _flat, min_loci=0)
    with pytest.raises(ValueError):
        cl.refine_doublets(3, COO, [0, 1, 1, 255], 2, _flat, doublet_threshold=1.5)
    # the pair's distribution is the one whose beta at locus 2 is (0 * 1 + 5 * 0.5) + 1: every cell scores as a doublet under it
    def fn(a, b, m):
        pair = b[2] == 3.5
        return (np.full(4, 50.0) if pair else np.zeros(4)), np.array([2.0, 2.0, 3.0, 0.0])
    r0 = cl.refine_doublets(3, COO, [0, 1, 1, 255], 2, fn, max_iter=0)
    assert r0["labels"].tolist() == [0, 1, 1, 255] and not r0["held"].any() and r0["summary"]["iterations"] == 0
    assert r0["call"].tolist() == [1, 1, 1, 1] and r0["summary"]["n_held"] == 0 and r0["summary"]["n_recounts"] == 1
    r = cl.refine_doublets(3, COO, [0, 1, 1, 255], 2, fn, max_iter=1)
    # cell 3 is unlabelled (and has no entry): it keeps label and flag; the others are held
    assert r["held"].tolist() == [1, 1, 1, 0] and r["labels"][3] == 255 and r["summary"]["n_held"] == 3 and r["summary"]["n_moved_last"] == 3
    assert r["summary"]["class_cells"][:2].tolist() == [0, 0]
    with pytest.raises(ValueError, match="every labelled cell is held"):
        cl.refine_doublets(3, COO, [0, 1, 1, 255], 2, fn, max_iter=2)
    # threshold 1.0: nothing exceeds it, nobody is held
    r1 = cl.refine_doublets(3, COO, [0, 1, 1, 255], 2, fn, max_iter=1, doublet_threshold=1.0)
    assert not r1["held"].any()
    # a held cell comes back when its doublet posterior falls
    back = cl.refine_doublets(3, COO, [0, 1, 1, 255], 2, _flat, held=[0, 0, 1, 0], max_iter=3, log_pair_prior=[-50.0])
    assert not back["held"].any() and back["summary"]["n_moved_total"] >= 1
    # the recount rule looks at the effective classes: held cells count in the slot of the unlabelled
    sizes = np.bincount(cl.effective_labels([0, 0, 1, 1, 255], [0, 1, 0, 0, 0], 2), minlength=3)
    assert sizes.tolist() == [1, 2, 2]
