"""cellector_locus_moments, cellector_locus_total_counts and cellector_iter_locus_moments are declared in the header, bound in
cellector_amd.ffi and reachable as Cellector methods; Cellector.locus_zscore is the rule of main.rs:317-322 (no GPU needed)."""
import ctypes as C
import inspect
import os
import re

import numpy as np

from cellector_amd import ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"cellector_locus_moments": 9, "cellector_locus_total_counts": 3, "cellector_iter_locus_moments": 5}  # name -> arguments


def _header():
    return open(os.path.join(ROOT, "include", "cellector_ffi.h")).read()


def test_declared_in_the_header_with_their_reference_seams():
    text = _header()
    for name, n_args in NAMES.items():
        m = re.search(r"cellector_status\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"{name} is not declared in cellector_ffi.h"
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert len(args.split(",")) == n_args, name
    section = text.split("locus moments: the per-locus expected log-likelihood and its variance", 1)[1].split("calculate_posteriors", 1)[0]
    for name in NAMES:
        assert name in section, name
    for cite in ("main.rs:368-420", "main.rs:394", "stats.rs:19-22", "stats.rs:23-28", "main.rs:556", "main.rs:343"):
        assert cite in section, cite
    # the option is documented with its scope; the timer id exists and the count moved
    options = text.split("cellector_status cellector_set_option", 1)[0]
    assert '"locus_moments"' in options
    tail = options.split('"locus_moments"', 1)[1]
    for word in ("cellector_em_threshold", "cellector_iter_locus_moments", "multi-device", "communicator", "cellector_set_shard",
                 "no launches, no allocations"):
        assert word in tail, word
    assert re.search(r"CELLECTOR_K_LOCUS_MOM\s*=\s*6\b", text) and re.search(r"CELLECTOR_K_COUNT\s*=\s*7\b", text)


def test_bound_in_signatures_with_the_right_argument_counts():
    for name, n_args in NAMES.items():
        assert name in ffi.SIGNATURES, name
        res, args = ffi.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args and args[0] is C.c_void_p, name
    assert ffi.K_LOCUS_MOM == 6 and ffi.K_CELL_VAR == 5


def test_exported_by_the_library(hip_lib_path):
    lib = ffi.load_library(hip_lib_path)
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is not exported"
    # a null ctx is an argument error, never a crash
    assert lib.cellector_locus_moments(None, None, None, None, None, None, None, None, None) == 1
    assert lib.cellector_locus_total_counts(None, None, None) == 1
    assert lib.cellector_iter_locus_moments(None, None, None, None, None) == 1


def test_cellector_methods():
    for name, params in (("locus_moments", ["self", "alpha", "beta", "mask", "flags"]), ("iter_locus_moments", ["self"]),
                         ("locus_total_counts", ["self", "flags"])):
        fn = getattr(ffi.Cellector, name, None)
        assert callable(fn), f"Cellector.{name} is missing"
        assert list(inspect.signature(fn).parameters) == params, name
    assert inspect.signature(ffi.Cellector.locus_total_counts).parameters["flags"].default is None
    assert isinstance(inspect.getattr_static(ffi.Cellector, "locus_zscore"), staticmethod)
    assert list(inspect.signature(ffi.Cellector.locus_zscore).parameters) == ["contrib", "exp", "var", "cells"]


def test_locus_zscore_rule():
    contrib = np.array([-10.0, -10.0, -10.0, 0.0, -3.0])
    exp = np.array([-4.0, -4.0, -4.0, 0.0, -3.0])
    var = np.array([9.0, 9.0, 0.0, 0.0, 4.0])
    cells = np.array([2, 0, 5, 0, 1], np.uint64)
    z = ffi.Cellector.locus_zscore(contrib, exp, var, cells)
    assert z.dtype == np.float64 and z.tolist() == [-2.0, 0.0, 0.0, 0.0, 0.0]
    with np.errstate(all="raise"):  # no division by zero, no sqrt of a negative on the way
        ffi.Cellector.locus_zscore(contrib, exp, np.array([9.0, -1.0, 0.0, 0.0, 4.0]), cells)
