"""cellector_add_doublets is declared in the header, bound in cellector_amd.ffi, exported by the library and reachable as a
Cellector method; doublets.TILE / BLOCK are the kernel file's defines; the twin refuses what the device call refuses (no GPU
needed)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from cellector_amd import doublets, ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, N_ARGS = "cellector_add_doublets", 6


def test_declared_in_the_header_with_its_reference_seams():
    text = open(os.path.join(ROOT, "include", "cellector_ffi.h")).read()
    m = re.search(r"cellector_status\s+" + NAME + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{NAME} is not declared in cellector_ffi.h"
    assert len(re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")) == N_ARGS
    section = text.split("synthetic doublets from resident cells", 1)[1].split("exchange buffers (device memory", 1)[0]
    for cite in ("main.rs:43", "main.rs:239-276"):
        assert cite in section, cite
    for phrase in ("(locus, cell, ref, alt)", "the ctx untouched", "CELLECTOR_ENOMEM", "OLD entries", "B per", "(2 j + s + 1) * GOLD",
                   "before and after cellector_ingest_finish", "65535"):
        assert phrase in section, phrase


def test_bound_in_signatures():
    assert NAME in ffi.SIGNATURES
    res, args = ffi.SIGNATURES[NAME]
    assert res is C.c_int and len(args) == N_ARGS and args[0] is C.c_void_p
    assert args[3] is C.c_uint64 and args[4] is C.c_double and args[5] is C.c_uint64


def test_exported_by_the_library(hip_lib_path):
    lib = ffi.load_library(hip_lib_path)
    assert hasattr(lib, NAME), f"{NAME} is not exported"
    assert lib.cellector_add_doublets(None, None, None, 0, 0.0, 4) == 1  # a null ctx is an argument error, never a crash


def test_cellector_method_and_twin_signatures():
    fn = getattr(ffi.Cellector, "add_doublets", None)
    assert callable(fn), "Cellector.add_doublets is missing"
    sig = inspect.signature(fn).parameters
    assert list(sig) == ["self", "cell_a", "cell_b", "downsample_rate", "seed"]
    assert [sig[k].default for k in ("downsample_rate", "seed")] == [0.0, 4]
    sig = inspect.signature(doublets.add_doublets_coo).parameters
    assert list(sig) == ["coo", "n_cells", "cell_a", "cell_b", "rate", "seed", "origin", "source", "k"]
    assert [sig[k].default for k in ("rate", "seed", "origin", "source", "k")] == [0.0, 4, None, None, 1]


def test_tile_and_block_are_the_kernel_files_defines():
    src = open(os.path.join(ROOT, "cellector_amd", "csrc", "kernels_doublets.hip")).read()
    for define, value in (("DOUBLETS_TILE", doublets.TILE), ("DB_BLOCK", doublets.BLOCK)):
        m = re.search(r"^#define\s+" + define + r"\s+(\d+)\s*$", src, flags=re.M)
        assert m, f"{define} is not a #define of kernels_doublets.hip"
        assert int(m.group(1)) == value
    assert "kernels_doublets.hip" in open(os.path.join(ROOT, "cellector_amd", "csrc", "Makefile")).read()


COO = [np.array([0, 0, 1, 2], np.uint32), np.array([0, 1, 2, 0], np.uint32), np.array([1, 2, 3, 4], np.uint32),
       np.array([5, 6, 7, 8], np.uint32)]


@pytest.mark.parametrize("kw,word", [
    (dict(cell_a=[], cell_b=[]), "no pairs"),
    (dict(cell_a=None, cell_b=[1]), "None"),
    (dict(cell_a=[0], cell_b=None), "None"),
    (dict(cell_a=[0, 1], cell_b=[1]), "cells"),
    (dict(cell_a=[0, 1, 3], cell_b=[1, 2, 0]), "pair 2"),
    (dict(cell_a=[0, 1], cell_b=[1, 3]), "pair 1"),
    (dict(cell_a=[0, -1], cell_b=[1, 2]), "pair 1"),
    (dict(cell_a=[0, 2, 1], cell_b=[1, 2, 1]), "pair 1 names cell 2 twice"),
    (dict(cell_a=[0], cell_b=[1], rate=1.5), "downsample_rate"),
    (dict(cell_a=[0], cell_b=[1], rate=-0.1), "downsample_rate"),
    (dict(cell_a=[0], cell_b=[1], rate=float("nan")), "downsample_rate"),
    (dict(cell_a=[0], cell_b=[1], k=256), "255"),
    (dict(cell_a=[0.5], cell_b=[1.0]), "indices"),
])
def test_the_twin_refuses_what_the_device_refuses(kw, word):
    with pytest.raises(ValueError) as e:
        doublets.add_doublets_coo(COO, 3, **kw)
    assert word in str(e.value), str(e.value)


def test_the_twin_refuses_more_cells_than_32_bits_hold():
    none = [np.zeros(0, np.uint32)] * 4
    with pytest.raises(ValueError) as e:
        doublets.add_doublets_coo(none, 2 ** 32 - 2, [0, 1], [1, 0])
    assert "32-bit" in str(e.value)
