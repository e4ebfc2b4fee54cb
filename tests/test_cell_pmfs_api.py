"""cellector_cell_pmfs and cellector_posterior_alpha_betas are declared in the header, bound in cellector_amd.ffi and reachable as
Cellector methods (no GPU needed)."""
import ctypes as C
import inspect
import os
import re

from cellector_amd import ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"cellector_cell_pmfs": 14, "cellector_posterior_alpha_betas": 4}  # name -> number of arguments


def _header():
    return open(os.path.join(ROOT, "include", "cellector_ffi.h")).read()


def test_declared_in_the_header_with_their_reference_seams():
    text = _header()
    for name, n_args in NAMES.items():
        m = re.search(r"cellector_status\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"{name} is not declared in cellector_ffi.h"
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert len(args.split(",")) == n_args, name
    section = text.split("the per-entry records behind those sums", 1)[1].split("cellector_posteriors", 1)[0]
    for cite in ("main.rs:527-539", "main.rs:556-575", "stats.rs:19-22", "stats.rs:23-28", "main.rs:239-254"):
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
    assert lib.cellector_cell_pmfs(None, None, None, None, None, 0, None, 0, None, None, None, None, None, None) == 1
    assert lib.cellector_posterior_alpha_betas(None, 0, None, None) == 1


def test_cellector_methods():
    for name, params in (("cell_pmfs", ["self", "cells", "alpha", "beta", "mask"]), ("posterior_alpha_betas", ["self", "which"])):
        fn = getattr(ffi.Cellector, name, None)
        assert callable(fn), f"Cellector.{name} is missing"
        assert list(inspect.signature(fn).parameters) == params, name
    # unchanged
    assert list(inspect.signature(ffi.Cellector.cell_log_likelihoods).parameters) == ["self", "alpha", "beta", "mask"]
