"""The three calls that place the EM state — cellector_set_excluded, cellector_set_loci_mask, cellector_em_reset — are declared in
the header, bound in cellector_amd.ffi and reachable as Cellector methods (no GPU needed)."""
import ctypes as C
import inspect
import os
import re

from cellector_amd import ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"cellector_set_excluded": 2, "cellector_set_loci_mask": 2, "cellector_em_reset": 1}  # name -> number of arguments


def _header():
    return open(os.path.join(ROOT, "include", "cellector_ffi.h")).read()


def test_declared_in_the_header_with_their_reference_seams():
    text = _header()
    for name, n_args in NAMES.items():
        m = re.search(r"cellector_status\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in cellector_ffi.h"
        assert len(m.group(1).split(",")) == n_args, name
    # the header comments cite the seams the calls replace
    section = text.split("placing the EM state", 1)[1].split("cellector_iter_resolution", 1)[0]
    for cite in ("main.rs:37", "main.rs:43", "load_data.rs:176-179", "main.rs:444-447"):
        assert cite in section, cite


def test_bound_in_signatures_with_the_right_argument_counts():
    for name, n_args in NAMES.items():
        assert name in ffi.SIGNATURES, name
        res, args = ffi.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args and args[0] is C.c_void_p, name


def test_exported_by_the_library(hip_lib_path):
    lib = ffi.load_library(hip_lib_path)
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is not exported"
    # a null ctx is an argument error, never a crash
    assert lib.cellector_set_excluded(None, None) == 1 and lib.cellector_set_loci_mask(None, None) == 1
    assert lib.cellector_em_reset(None) == 1


def test_cellector_methods():
    for name, params in (("set_excluded", ["self", "flags"]), ("set_loci_mask", ["self", "used"]), ("em_reset", ["self"])):
        fn = getattr(ffi.Cellector, name, None)
        assert callable(fn), f"Cellector.{name} is missing"
        assert list(inspect.signature(fn).parameters) == params, name
    assert list(inspect.signature(ffi.Cellector.run).parameters) == ["self", "iqr_multiple", "max_iter"]  # unchanged
