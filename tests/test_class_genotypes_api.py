"""CPU: cellector_class_genotypes is declared after the class-doublet calls, exported and bound with the header's signature; what the
binding and the twin refuse before any device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest

from cellector_amd import ffi
from cellector_amd import genotypes as gn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_exported_and_bound(hip_lib_path):
    text = open(os.path.join(ROOT, "include", "cellector_ffi.h")).read()
    at = text.index("cellector_status cellector_class_genotypes(")
    assert text.index("cellector_status cellector_refine_class_doublets(") < at < text.index("cellector_status cellector_final_allele_tallies(")
    decl = re.sub(r"/\*.*?\*/", "", text[at:text.index(";", at)], flags=re.S)
    assert [a.split()[-1].lstrip("*") for a in decl[decl.index("(") + 1:decl.rindex(")")].split(",")] == [
        "ctx", "labels", "n_classes", "ambient", "gt_threshold", "cells", "alt", "ref", "gt", "gp", "gp3"]
    lib = ffi.load_library(hip_lib_path)
    assert hasattr(lib, "cellector_class_genotypes")
    res, args = ffi.SIGNATURES["cellector_class_genotypes"]
    assert res is ctypes.c_int and len(args) == 11 and args[2] is ctypes.c_uint32 and args[3] is args[4] is ctypes.c_double
    assert all(a is ctypes.c_void_p for a in args[:2] + args[5:])
    assert callable(ffi.Cellector.class_genotypes)
    # a null ctx is refused without touching anything
    assert lib.cellector_class_genotypes(None, None, 2, 0.03, 0.99, *([None] * 6)) == 1
    # no kernel id was added: the enum ends where it did
    assert re.search(r"CELLECTOR_K_COUNT\s*=\s*7\b", text)


def test_the_header_states_the_model():
    text = open(os.path.join(ROOT, "include", "cellector_ffi.h")).read()
    block = text[text.index("---- class genotypes"):text.index("cellector_status cellector_class_genotypes(")]
    for word in ("soup", "ambient", "gt_threshold", "keep_coo", "total_loci", "NaN", "255", "CELLECTOR_ENOMEM", "one host thread"):
        assert word in block, word


def test_twin_constants_and_shapes():
    assert gn.GT_STRINGS == ("./.", "1/1", "0/1", "0/0")
    coo = (np.array([0, 2, 2]), np.array([0, 1, 2]), np.array([1, 2, 3]), np.array([4, 5, 6]))
    cells, alt, ref = gn.class_genotype_tallies(4, coo, np.array([1, 255, 1], np.uint8), 2)
    assert cells.tolist() == [0, 2, 1] and alt.tolist() == [[0, 0, 0, 0], [1, 0, 3, 0], [0, 0, 2, 0]]
    assert ref.tolist() == [[0, 0, 0, 0], [4, 0, 6, 0], [0, 0, 5, 0]]
    gt, gp, gp3 = gn.genotype_posteriors(alt, ref)
    assert gt.shape == gp.shape == (2, 4) and gp3.shape == (2, 4, 3) and (gp[0] == 1.0 / 3.0).all() and not gt[0].any()
