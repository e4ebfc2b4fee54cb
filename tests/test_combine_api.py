"""cellector_combine and cellector_cell_source are declared in the header, bound in cellector_amd.ffi, exported by the library and
reachable as Cellector methods; combine.TILE is the kernel file's COMBINE_TILE (no GPU needed)."""
import ctypes as C
import inspect
import os
import re

from cellector_amd import combine, ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"cellector_combine": 7, "cellector_cell_source": 2}  # name -> number of arguments


def test_declared_in_the_header_with_their_reference_seams():
    text = open(os.path.join(ROOT, "include", "cellector_ffi.h")).read()
    for name, n_args in NAMES.items():
        m = re.search(r"cellector_status\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in cellector_ffi.h"
        assert len(m.group(1).split(",")) == n_args, name
    section = text.split("merging a second staged matrix in", 1)[1].split("exchange buffers (device memory", 1)[0]
    for cite in ("main.rs:197-231", "main.rs:161-186", "main.rs:111"):
        assert cite in section, cite
    for phrase in ("(locus, cell, ref, alt)", "BOTH ctxs untouched", "CELLECTOR_ENOMEM", "OLD entries", "B per"):
        assert phrase in section, phrase


def test_bound_in_signatures_with_the_right_argument_counts():
    for name, n_args in NAMES.items():
        assert name in ffi.SIGNATURES, name
        res, args = ffi.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args and args[0] is C.c_void_p, name
    args = ffi.SIGNATURES["cellector_combine"][1]
    assert args[4] is C.c_uint64 and args[5] is C.c_double and args[6] is C.c_uint64


def test_exported_by_the_library(hip_lib_path):
    lib = ffi.load_library(hip_lib_path)
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is not exported"
    # a null ctx is an argument error, never a crash
    assert lib.cellector_combine(None, None, None, None, 0, 0.0, 4) == 1
    assert lib.cellector_cell_source(None, None) == 1


def test_cellector_methods():
    for name, params in (("combine", ["self", "src", "keep", "locus_map", "total_loci", "downsample_rate", "seed"]),
                         ("cell_source", ["self"])):
        fn = getattr(ffi.Cellector, name, None)
        assert callable(fn), f"Cellector.{name} is missing"
        assert list(inspect.signature(fn).parameters) == params, name
    sig = inspect.signature(ffi.Cellector.combine).parameters
    assert [sig[k].default for k in ("keep", "locus_map", "total_loci", "downsample_rate", "seed")] == [None, None, None, 0.0, 4]
    sig = inspect.signature(combine.combine_coo).parameters
    assert list(sig)[:9] == ["dst_coo", "n_dst", "src_coo", "n_src", "keep", "locus_map", "total_loci_out", "rate", "seed"]
    assert callable(combine.locus_map_from_vcfs)


def test_tile_is_the_kernel_files_define():
    src = open(os.path.join(ROOT, "cellector_amd", "csrc", "kernels_combine.hip")).read()
    m = re.search(r"^#define\s+COMBINE_TILE\s+(\d+)\s*$", src, flags=re.M)
    assert m, "COMBINE_TILE is not a #define of kernels_combine.hip"
    assert int(m.group(1)) == combine.TILE
    assert "kernels_combine.hip" in open(os.path.join(ROOT, "cellector_amd", "csrc", "Makefile")).read()
