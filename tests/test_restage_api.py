"""cellector_restage, cellector_cell_origin and cellector_staged_coo are declared in the header, bound in cellector_amd.ffi,
exported by the library and reachable as Cellector methods; restage.TILE is the kernel file's RESTAGE_TILE (no GPU needed)."""
import ctypes as C
import inspect
import os
import re

from cellector_amd import ffi, restage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"cellector_restage": 4, "cellector_cell_origin": 2, "cellector_staged_coo": 7}  # name -> number of arguments


def _header():
    return open(os.path.join(ROOT, "include", "cellector_ffi.h")).read()


def test_declared_in_the_header_with_their_reference_seams():
    text = _header()
    for name, n_args in NAMES.items():
        m = re.search(r"cellector_status\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in cellector_ffi.h"
        assert len(m.group(1).split(",")) == n_args, name
    section = text.split("re-staging the resident matrix", 1)[1].split("exchange buffers (device memory", 1)[0]
    for cite in ("load_barcodes", "main.rs:246-255", "main.rs:257-280", "main.rs:83-88", "main.rs:102-107"):
        assert cite in section, cite
    # the two rules a caller must know: the order a finished ingest leaves, and what a memory failure leaves
    for phrase in ("stable sort by locus", "CELLECTOR_ENOMEM", "OLD entries"):
        assert phrase in section, phrase


def test_bound_in_signatures_with_the_right_argument_counts():
    for name, n_args in NAMES.items():
        assert name in ffi.SIGNATURES, name
        res, args = ffi.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args and args[0] is C.c_void_p, name
    assert ffi.SIGNATURES["cellector_restage"][1][2] is C.c_double and ffi.SIGNATURES["cellector_restage"][1][3] is C.c_uint64


def test_exported_by_the_library(hip_lib_path):
    lib = ffi.load_library(hip_lib_path)
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is not exported"
    # a null ctx is an argument error, never a crash
    assert lib.cellector_restage(None, None, 0.0, 4) == 1
    assert lib.cellector_cell_origin(None, None) == 1
    assert lib.cellector_staged_coo(None, None, None, None, None, None, 0) == 1


def test_cellector_methods():
    for name, params in (("restage", ["self", "keep", "downsample_rate", "seed"]), ("cell_origin", ["self"]), ("staged_coo", ["self"])):
        fn = getattr(ffi.Cellector, name, None)
        assert callable(fn), f"Cellector.{name} is missing"
        assert list(inspect.signature(fn).parameters) == params, name
    sig = inspect.signature(ffi.Cellector.restage).parameters
    assert (sig["keep"].default, sig["downsample_rate"].default, sig["seed"].default) == (None, 0.0, 4)
    sig = inspect.signature(restage.restage_coo).parameters
    assert list(sig) == ["locus0", "cell0", "alt", "ref", "total_cells", "keep", "downsample_rate", "seed"]
    assert (sig["keep"].default, sig["downsample_rate"].default, sig["seed"].default) == (None, 0.0, 4)


def test_tile_is_the_kernel_files_define():
    src = open(os.path.join(ROOT, "cellector_amd", "csrc", "kernels_restage.hip")).read()
    m = re.search(r"^#define\s+RESTAGE_TILE\s+(\d+)\s*$", src, flags=re.M)
    assert m, "RESTAGE_TILE is not a #define of kernels_restage.hip"
    assert int(m.group(1)) == restage.TILE
    assert "kernels_restage.hip" in open(os.path.join(ROOT, "cellector_amd", "csrc", "Makefile")).read()
