"""CPU: cellector_donor_genotypes is declared behind the donor pair fractions, exported and bound with the header's argument names;
the header states the model; the struct layouts and the defaults; a null ctx is refused; the binding's argument checks; the twin's
functions and helpers."""
import ctypes
import os
import re

import numpy as np
import pytest

from cellector_amd import donor_genotypes as dg, ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "cellector_ffi.h")).read()

ARGS = {
    "cellector_donor_genotypes_default_params": ["out"],
    "cellector_donor_genotypes": ["ctx", "assign", "prior", "n_donors", "params", "cells", "alt", "ref", "q", "gt_out", "kind", "summary", "tab",
                                  "pass_ms"],
}


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    m = re.search(r"cellector_status\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared"
    return [a.strip() for a in m.group(1).split(",")]


def test_declared_exported_and_bound(hip_lib_path):
    lib = ffi.load_library(hip_lib_path)
    for name, args in ARGS.items():
        decl = _declared(name)
        assert [re.findall(r"[A-Za-z_][A-Za-z_0-9]*", a)[-1] for a in decl] == args, name
        res, argtypes = ffi.SIGNATURES[name]
        assert hasattr(lib, name) and res is ctypes.c_int and len(argtypes) == len(args), name
        for a, t in zip(decl, argtypes):
            want = ctypes.c_void_p if "*" in a else ctypes.c_uint32 if a.startswith("uint32_t") else ctypes.c_double
            assert t is want, (name, a, t)
    for m in ("donor_genotypes_default_params", "donor_genotypes", "refine_donors"):
        assert callable(getattr(ffi.Cellector, m))
    at = [HEADER.index(s) for s in ("cellector_status cellector_donor_pair_fractions(", "cellector_status cellector_donor_genotypes_default_params(",
                                    "cellector_status cellector_donor_genotypes(", "cellector_status cellector_final_allele_tallies(")]
    assert at == sorted(at)
    for f in ("tallies", "tables", "weights", "posterior", "calls", "summary", "donor_genotypes", "prior_from_gt", "to_gp", "render_vcf_columns",
              "render_tsv"):
        assert callable(getattr(dg, f)), f
    src = open(os.path.join(ROOT, "cellector_amd", "csrc", "kernels_donor_genotypes.hip")).read()
    for k in ("k_dg_tallies", "k_dg_tables", "k_dg_posterior"):
        assert "__global__" in src and k in src
    assert "kernels_donor_genotypes.hip" in open(os.path.join(ROOT, "cellector_amd", "csrc", "Makefile")).read()


def test_struct_layouts_and_defaults(hip_lib_path):
    lib = ffi.load_library(hip_lib_path)
    P, S = ffi.DonorGenotypesParams, ffi.DonorGenotypesSummary
    assert ctypes.sizeof(P) == 32 and [getattr(P, k).offset for k, _ in P._fields_] == [0, 8, 16, 24]
    assert [k for k, _ in P._fields_] == ["err", "ambient", "gt_threshold", "prior_floor"]
    assert ctypes.sizeof(S) == 6 * 64 * 8 and [getattr(S, k).offset for k, _ in S._fields_] == [512 * i for i in range(6)]
    assert [k for k, _ in S._fields_] == ["cells", "loci_with_reads", "confirmed", "filled", "changed", "withdrawn"]
    p = P()
    assert lib.cellector_donor_genotypes_default_params(ctypes.byref(p)) == 0
    assert {k: getattr(p, k) for k, _ in P._fields_} == dg.DEFAULTS == dict(err=0.01, ambient=0.03, gt_threshold=0.99, prior_floor=0.01)
    assert lib.cellector_donor_genotypes_default_params(None) == 1
    assert dg.KIND_NAMES == {0: "no_reads", 1: "confirmed", 2: "filled", 3: "changed", 4: "withdrawn"}


def test_null_ctx_is_refused(hip_lib_path):
    lib = ffi.load_library(hip_lib_path)
    assert lib.cellector_donor_genotypes(None, None, None, 3, *([None] * 10)) == 1


def test_header_states_the_model():
    beg = HEADER.index("donor genotype refinement")
    block = HEADER[beg:HEADER.index("cellector_status cellector_donor_genotypes_default_params(")]
    for word in ("assign [cells] u8", "255", "three NaN", "NULL = every row is a no-call", "1 <= D <= 64", "gt_threshold", "prior_floor",
                 "main.rs:93-124", "never be\n *   overturned", "ALL total_loci loci", "slot D", "Exact in any entry order", "counts each time",
                 "((double)A + 1.0) / ((double)(A + R) + 2.0)", "tab1[l][g]", "lam_g", "1.0 / 3.0", "(prior_floor / 3.0)", "v_g == 0",
                 "ascending g from 0.0", "smallest g on ties", "q_call > gt_threshold", "withdrawn", "filled", "confirmed", "changed",
                 "lean toward it", "few cells", "Doublets must stay out", "keep_coo", "no iteration in flight", "single-device ctx",
                 "CELLECTOR_EINVAL", "CELLECTOR_ENOMEM", "before the first launch", "EM\n * state is never touched", "without contraction"):
        assert word in block, word


class _Dims:
    total_cells, total_loci, loci_used, cell_begin, cell_end = 5, 7, 6, 0, 5


def test_binding_argument_checks():
    """the checks the binding makes before the library is called, on an object that holds no ctx"""
    g = object.__new__(ffi.Cellector)
    g.dims = lambda: _Dims
    g.donor_genotypes_default_params = lambda: ffi.DonorGenotypesParams()
    a, prior = np.zeros(5, np.uint8), np.zeros((3, 7, 3), np.float32)
    with pytest.raises(ValueError, match="assign: 5 values"):
        g.donor_genotypes(a[:4], prior)
    with pytest.raises(ValueError, match=r"prior: shape \(D, 7, 3\)"):
        g.donor_genotypes(a, prior[:, :6])
    with pytest.raises(ValueError, match=r"prior: shape \(D, 7, 3\)"):
        g.donor_genotypes(a, np.zeros((3, 7), np.float32))
    with pytest.raises(ValueError, match="n_donors: needed"):
        g.donor_genotypes(a)
    with pytest.raises(ValueError, match="n_donors = 2, but prior holds 3"):
        g.donor_genotypes(a, prior, n_donors=2)
    with pytest.raises(TypeError, match="unknown parameter 'floor'"):
        g.donor_genotypes(a, prior, floor=0.2)
    with pytest.raises(TypeError, match="unknown parameter"):
        dg.donor_genotypes(7, [np.zeros(0, np.int64)] * 4, a, 3, floor=0.2)


def test_helpers():
    gt = np.array([[0, 1, 2, 3], [3, 3, 0, 2]], np.uint8)
    p = dg.prior_from_gt(gt)
    assert p.dtype == np.float32 and p.shape == (2, 4, 3)
    assert p[0, :3].tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 1]] and np.isnan(p[0, 3]).all() and np.isnan(p[1, :2]).all()
    with pytest.raises(ValueError):
        dg.prior_from_gt(np.array([[4]]))
    w, call = dg.weights(p, 2, 4)
    assert np.array_equal(call, gt) and (w[1, 0] == 1.0 / 3.0).all() and w[0, 1].tolist() == [0.0, 1.0, 0.0]
    q = np.array([[[1.0, 1e-60, 0.0], [0.25, 0.5, 0.25]]])
    f = dg.to_gp(q)
    assert f.dtype == np.float32 and f.flags["C_CONTIGUOUS"] and f[0, 0].tolist() == [1.0, 0.0, 0.0] and f[0, 1].tolist() == [0.25, 0.5, 0.25]
    # the rule on hand-made numbers: threshold strict, ties to the smaller g, the five kinds
    q = np.array([[[0.99, 0.01, 0.0], [0.995, 0.005, 0.0], [0.4, 0.4, 0.2], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [1 / 3, 1 / 3, 1 / 3]]])
    gt_out, kind = dg.calls(q, np.array([[5, 5, 5, 5, 5, 0]]), np.array([[0, 3, 1, 2, 0, 3]]), 0.99)
    assert gt_out.tolist() == [[3, 0, 3, 2, 1, 3]] and kind.tolist() == [[4, 2, 4, 1, 3, 0]]
    s = dg.summary(np.array([9, 4], np.uint64), kind)
    assert {k: v.tolist() for k, v in s.items()} == dict(cells=[9], loci_with_reads=[5], confirmed=[1], filled=[1], changed=[1], withdrawn=[2])
    assert dg.render_tsv(["a"], s) == "donor\tcells\tloci_with_reads\tconfirmed\tfilled\tchanged\twithdrawn\na\t9\t5\t1\t1\t1\t2\n"
