"""cellector_cell_log_variances and cellector_iter_cell_variances are declared in the header, bound in cellector_amd.ffi and
reachable as Cellector methods (no GPU needed)."""
import ctypes as C
import inspect
import os
import re

from cellector_amd import ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"cellector_cell_log_variances": 5, "cellector_iter_cell_variances": 2}  # name -> number of arguments


def _header():
    return open(os.path.join(ROOT, "include", "cellector_ffi.h")).read()


def test_declared_in_the_header_with_their_reference_seams():
    text = _header()
    for name, n_args in NAMES.items():
        m = re.search(r"cellector_status\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"{name} is not declared in cellector_ffi.h"
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert len(args.split(",")) == n_args, name
    section = text.split("the fourth per-cell vector: expected_log_variances", 1)[1].split("calculate_posteriors", 1)[0]
    for name in NAMES:
        assert name in section, name
    for cite in ("main.rs:541-591", "main.rs:316-318", "stats.rs:23-28"):
        assert cite in section, cite
    # the two options are documented with the pairs they refuse and the two notes the z-score mode needs
    options = text.split("cellector_status cellector_set_option", 1)[0]
    assert '"cell_variance"' in options
    tail = options.split('"cell_variance"', 1)[1]
    for word in ('"normalization"', "resolve_ties", "compute_expected", "n_near_threshold", "main.rs:317-318", "default of 5"):
        assert word in tail, word


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
    assert lib.cellector_cell_log_variances(None, None, None, None, None) == 1
    assert lib.cellector_iter_cell_variances(None, None) == 1


def test_cellector_methods():
    for name, params in (("cell_log_variances", ["self", "alpha", "beta", "mask"]), ("cell_variances", ["self"])):
        fn = getattr(ffi.Cellector, name, None)
        assert callable(fn), f"Cellector.{name} is missing"
        assert list(inspect.signature(fn).parameters) == params, name
    assert inspect.signature(ffi.Cellector.cell_log_variances).parameters["mask"].default is None
    # unchanged
    assert list(inspect.signature(ffi.Cellector.cell_log_likelihoods).parameters) == ["self", "alpha", "beta", "mask"]
    assert ffi.K_CELL_VAR == 5
