"""cellector_write_mtx / cellector_format_mtx are declared in the header with their contract, bound in cellector_amd.ffi, exported by
the library and reachable as Cellector methods; the mode / flag constants and cellector_write_summary's layout; the twin's constants
are the kernel file's; the CLI's --write_matrices (no GPU needed)."""
import ctypes as C
import inspect
import os
import re
import subprocess

from cellector_amd import ffi, mtx_write
from test_host_cli import host_bin  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"cellector_write_mtx": 6, "cellector_format_mtx": 10}  # name -> arguments
BASE = ["-a", "a", "-r", "r", "-b", "b", "--output_directory", "o"]
FIELDS = ["n_entries", "lines_first", "lines_second", "bytes_first", "bytes_second", "n_dropped_keys", "n_windows"]


def _header():
    return open(os.path.join(ROOT, "include", "cellector_ffi.h")).read()


def test_declared_in_the_header_with_the_contract():
    text = _header()
    for name, n_args in NAMES.items():
        m = re.search(r"cellector_status\s+" + name + r"\s*\(([^)]*)\)\s*;", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
        assert m, f"{name} is not declared in cellector_ffi.h"
        assert len(m.group(1).split(",")) == n_args, name
    for name, value in (("CELLECTOR_WRITE_ALIGNED", "0"), ("CELLECTOR_WRITE_SPARSE", "1"), ("CELLECTOR_WRITE_DEPTH", "2"),
                        ("CELLECTOR_MTX_SPACE", "1u"), ("CELLECTOR_MTX_HEADER_ZERO", "2u")):
        assert re.search(r"#define\s+" + name + r"\s+" + value + r"\b", text), name
    section = text.split("the staged matrix as mtx text, made on the device", 1)[1].split("exchange buffers", 1)[0]
    for phrase in ("main.rs:52-116", "main.rs:67-69", "STAGED order", "formed in 64 bits", "131070", "n_dropped_keys", "cellector_restage",
                   "only read the ctx", "CELLECTOR_EINVAL", "CELLECTOR_EIO", "REMOVES NOTHING", "never unlinks", "write_window", "pinned",
                   "are still returned", "out == NULL", "CELLECTOR_JOIN_REF", "CELLECTOR_JOIN_DEPTH"):
        assert phrase in section, phrase
    assert '"write_window"' in text.split("cellector_status cellector_set_option", 1)[0]


def test_bound_in_signatures():
    for name, n_args in NAMES.items():
        assert name in ffi.SIGNATURES, name
        res, args = ffi.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args and args[0] is C.c_void_p, name
    assert ffi.SIGNATURES["cellector_write_mtx"][1][1:5] == [C.c_char_p, C.c_char_p, C.c_int, C.c_uint32]
    args = ffi.SIGNATURES["cellector_format_mtx"][1]
    assert args[1:6] == [C.c_int, C.c_int, C.c_uint32, C.c_uint64, C.c_uint64] and args[7] is C.c_uint64


def test_summary_layout_and_constants():
    s = ffi.WriteSummary
    assert C.sizeof(s) == 56
    assert [name for name, _ in s._fields_] == FIELDS and all(t is C.c_uint64 for _, t in s._fields_)
    body = re.search(r"typedef struct \{([^}]*)\} cellector_write_summary;", _header()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(n_entries|lines_\w+|bytes_\w+|n_dropped_keys|n_windows)\b", body) == FIELDS
    assert "uint32_t" not in body
    assert ffi.WRITE_MODES == {"aligned": 0, "sparse": 1, "depth": 2, 0: 0, 1: 1, 2: 2} == mtx_write.MODES
    assert (ffi.MTX_SPACE, ffi.MTX_HEADER_ZERO) == (1, 2) == (mtx_write.FLAG_SPACE, mtx_write.FLAG_HEADER_ZERO)
    assert mtx_write.flags(" ", True) == 3 and mtx_write.flags("\t") == 0
    assert sorted(mtx_write.summary(3, 3, [0], [0], [1], [0]).keys()) == sorted(FIELDS)


def test_exported_by_the_library(hip_lib_path):
    lib = ffi.load_library(hip_lib_path)
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is not exported"
    # a null ctx is an argument error, never a crash
    assert lib.cellector_write_mtx(None, b"a", b"b", 0, 0, None) == 1
    assert lib.cellector_format_mtx(None, 0, 0, 0, 0, 0, None, 0, None, None) == 1


def test_cellector_methods_and_the_twin():
    for name, params in (("write_mtx", ["self", "first", "second", "mode", "sep", "header_zero"]),
                         ("format_mtx", ["self", "which", "mode", "first_entry", "n_entries", "sep"])):
        fn = getattr(ffi.Cellector, name, None)
        assert callable(fn), f"Cellector.{name} is missing"
        assert list(inspect.signature(fn).parameters) == params, name
    sig = inspect.signature(ffi.Cellector.write_mtx).parameters
    assert (sig["mode"].default, sig["sep"].default, sig["header_zero"].default) == ("aligned", "\t", False)
    assert list(inspect.signature(mtx_write.format_lines).parameters) == ["locus0", "cell0", "alt", "ref", "which", "mode", "sep"]
    assert callable(mtx_write.header) and callable(mtx_write.write_pair)


def test_the_twins_constants_are_the_kernel_files():
    src = open(os.path.join(ROOT, "cellector_amd", "csrc", "kernels_mtx_write.hip")).read()
    m = re.search(r"^#define\s+MW_WINDOW_DEFAULT\s+\(1ull << (\d+)\)", src, flags=re.M)
    assert m and 1 << int(m.group(1)) == mtx_write.WINDOW
    assert '#include "mtx_format.h"' in src
    assert "kernels_mtx_write.hip" in open(os.path.join(ROOT, "cellector_amd", "csrc", "Makefile")).read()
    code = re.sub(r"//.*", "", src)
    kernels = code.split("struct MwScratch")[0]
    assert "asm" not in code and "printf" not in kernels  # no printf in a kernel
    assert not re.search(r"[^/*]/\s*[a-z_]\w*\b(?!\s*\()", kernels.replace("MW_BLOCK / 64", ""))  # no division by a variable in a kernel
    assert "unlink" not in src and "remove(" not in src


def test_cli_help_has_the_paragraph(host_bin):  # noqa: F811
    r = subprocess.run([host_bin, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--write_matrices <aligned|sparse|depth>" in r.stdout
    para = " ".join(r.stdout.split("--write_matrices <aligned|sparse|depth>", 1)[1].split())
    for phrase in ("alt.mtx and ref.mtx", "ad.mtx and dp.mtx", "barcodes.tsv", "--matrix_pair join", "--matrix_pair depth", "one GPU"):
        assert phrase in para, phrase


def test_cli_refuses_a_bad_word_and_more_than_one_gpu(host_bin):  # noqa: F811
    r = subprocess.run([host_bin] + BASE + ["--write_matrices", "bogus"], capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.startswith("error: Invalid value 'bogus' for '--write_matrices <aligned|sparse|depth>'"), r.stderr
    assert "expected aligned, sparse or depth" in r.stderr
    for word in ("aligned", "sparse", "depth"):
        r = subprocess.run([host_bin] + BASE + ["--write_matrices", word, "--devices", "0,0"], capture_output=True, text=True)
        assert r.returncode == 1, r.stderr
        assert r.stderr.startswith(f"error: The argument '--write_matrices {word}' works on one GPU and cannot be used with '--devices <a,b,...>'")
