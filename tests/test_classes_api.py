"""CPU: the class bindings exist with the header's signatures, and cellector_amd.classes (the numpy twin) on its own: a dead class,
K = 1, ties go to the lowest k, rest == 0 gives qual 255, the recount rule, reference_scales."""
import ctypes
import math

import numpy as np
import pytest

from cellector_amd import classes as cl
from cellector_amd import ffi


def test_bindings(hip_lib_path):
    lib = ffi.load_library(hip_lib_path)
    for name, nargs in (("cellector_class_tallies", 6), ("cellector_class_alpha_betas", 6), ("cellector_class_posteriors", 10),
                        ("cellector_refine_classes", 12)):
        assert hasattr(lib, name) and len(ffi.SIGNATURES[name][1]) == nargs
    for m in ("class_tallies", "class_alpha_betas", "class_posteriors", "refine_classes"):
        assert callable(getattr(ffi.Cellector, m))
    assert ctypes.sizeof(ffi.RefineSummary) == 8 + 3 * 8 + 16 * 8
    assert ffi.RefineSummary.class_cells.offset == 32 and ffi.RefineSummary.n_moved_last.offset == 8
    # a null ctx is refused without touching anything
    assert lib.cellector_class_tallies(None, None, 2, None, None, None) == 1
    assert lib.cellector_refine_classes(None, None, 2, None, None, None, 1, 1, None, None, None, None) == 1


COO = (np.array([0, 0, 1, 1, 2, 2, 2]), np.array([0, 1, 0, 2, 1, 2, 2]), np.array([3, 0, 1, 2, 0, 5, 1]), np.array([0, 2, 1, 0, 4, 0, 1]))


def _flat(alpha, beta, mask):
    return np.zeros(4), np.array([2.0, 2.0, 3.0, 0.0])


def test_tallies_dead_class_and_repeated_pair():
    lab = np.array([0, 2, 2, 255], np.uint8)
    cells, alt, ref = cl.class_tallies(3, COO, lab, 3)
    assert cells.tolist() == [1, 0, 2]
    assert alt.tolist() == [[3, 1, 0], [0, 0, 0], [0, 2, 6]] and ref.tolist() == [[0, 1, 0], [0, 0, 0], [2, 0, 5]]
    a, b = cl.class_alpha_betas(alt, ref, [1.0, 0.01, 0.07])
    assert a[2].tolist() == [1.0, 2.0 * 0.07 + 1.0, 6.0 * 0.07 + 1.0] and b[1].tolist() == [1.0, 1.0, 1.0]
    out = cl.posteriors(3, COO, lab, 3, _flat)
    assert np.isneginf(out["ll"][1]).all() and (out["posterior"][1] == 0).all() and not (out["best"] == 1).any()
    # no entry information at all (ll = 0 everywhere): the posterior is the prior
    lp = out["log_prior"]
    assert lp[0] == math.log(2.0 / 5.0) and lp[2] == math.log(3.0 / 5.0) and lp[1] == -math.inf
    assert np.allclose(out["posterior"][0], 0.4, rtol=1e-15) and (out["best"] == 2).all()


def test_k1_ties_and_saturation():
    one = cl.posterior_chain(np.array([[-3.0, 0.0, -700.0]]), [0.0], [True])
    assert (one["posterior"] == 1.0).all() and (one["qual"] == 255).all() and (one["best"] == 0).all()
    tie = cl.posterior_chain(np.array([[-5.0, -1.0], [-2.0, -1.0], [-2.0, -1.0]]), [0.0, 0.0, 0.0], [True, True, True])
    assert tie["best"].tolist() == [1, 0]
    sat = cl.posterior_chain(np.array([[0.0], [-800.0]]), [0.0, 0.0], [True, True])
    assert sat["rest"][0] == 0.0 and sat["qual"][0] == 255 and sat["posterior"][0, 0] == 1.0
    half = cl.posterior_chain(np.array([[0.0], [0.0]]), [0.0, 0.0], [True, True])
    assert half["qual"][0] == 3 and half["best"][0] == 0  # -10 log10(0.5) = 3.01
    dead = cl.posterior_chain(np.array([[0.0], [5.0], [0.0]]), [0.0, 0.0, 0.0], [True, False, True])
    assert dead["posterior"][1, 0] == 0.0 and dead["best"][0] == 0


def test_refusals_and_refine_driver():
    with pytest.raises(ValueError, match="cell 1 has label 3"):
        cl.check_labels([0, 3, 255], 3)
    with pytest.raises(ValueError, match="every cell is unlabelled"):
        cl.check_labels([255, 255], 2)
    with pytest.raises(ValueError):
        cl.check_labels([0], 17)
    with pytest.raises(ValueError):
        cl.refine(3, COO, [0, 1, 1, 255], 2, _flat, min_loci=0)
    # ll prefers class 1 for every cell; cell 3 has no entry (min_loci) and is unlabelled: both keep theirs
    fn = lambda a, b, m: ((np.zeros(4), np.array([2.0, 2.0, 3.0, 0.0])) if a[2] == 1.0 else (np.full(4, 50.0), np.array([2.0, 2.0, 3.0, 0.0])))
    r = cl.refine(3, COO, [0, 0, 1, 255], 2, fn, max_iter=5)
    assert r["labels"].tolist()[3] == 255 and r["summary"]["iterations"] >= 1
    assert r["summary"]["n_recounts"] >= 1 and r["summary"]["class_cells"][:2].sum() == 3
    r0 = cl.refine(3, COO, [0, 0, 1, 255], 2, fn, max_iter=0)
    assert r0["labels"].tolist() == [0, 0, 1, 255] and r0["summary"]["iterations"] == 0 and r0["summary"]["n_recounts"] == 1
    assert cl._recount_rule(0, True, 0, np.array([5, 3, 1])) and not cl._recount_rule(1, True, 4, np.array([5, 3, 1]))
    assert cl._recount_rule(1, True, 5, np.array([5, 3, 1])) and cl._recount_rule(1, False, 0, np.array([5, 3, 1]))


def test_reference_scales():
    sc, lp = cl.reference_scales(69, 999)
    assert sc.tolist() == [1.0, 0.07] and lp.tolist() == [math.log(0.07), math.log(1.0 - 0.07)]
    sc, lp = cl.reference_scales(0, 999)
    assert sc[1] == 0.01
