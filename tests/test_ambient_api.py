"""CPU: the ambient calls are declared behind the donor block, exported and bound with the header's argument names; the header states
the model; the struct layouts and the defaults; a null ctx is refused; genotypes.donor_codes; the host binary's usage errors and help
text for --estimate_ambient."""
import ctypes
import os
import re
import subprocess

import numpy as np

from cellector_amd import ambient, ffi, genotypes
from test_host_cli import host_bin  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "cellector_ffi.h")).read()

ARGS = {
    "cellector_ambient_default_params": ["out"],
    "cellector_ambient_tables": ["ctx", "rho", "n_grid", "err", "mask", "tab"],
    "cellector_ambient_profile": ["ctx", "gt", "n_sources", "assign", "rho", "n_grid", "err", "min_loci", "mask", "ll", "total",
                                  "source_total", "source_cells", "n_entries", "cell_rho", "cell_se", "tab"],
    "cellector_estimate_ambient": ["ctx", "gt", "n_sources", "assign", "params", "mask", "summary", "cell_rho", "cell_se", "n_entries"],
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
            want = ctypes.c_void_p if "*" in a else ctypes.c_uint32 if a.startswith("uint32_t") else ctypes.c_uint64 if \
                a.startswith("uint64_t") else ctypes.c_double
            assert t is want, (name, a, t)
    for m in ("ambient_default_params", "ambient_tables", "ambient_profile", "estimate_ambient"):
        assert callable(getattr(ffi.Cellector, m))
    # next to the donor block, in front of what followed it
    at = [HEADER.index(s) for s in ("cellector_status cellector_match_donors(", "cellector_status cellector_ambient_default_params(",
                                    "cellector_status cellector_ambient_tables(", "cellector_status cellector_ambient_profile(",
                                    "cellector_status cellector_estimate_ambient(", "cellector_status cellector_final_allele_tallies(")]
    assert at == sorted(at)
    for f in ("grid", "tables", "cell_sums", "fold", "vertex", "estimate"):
        assert callable(getattr(ambient, f)), f


def test_struct_layouts_and_defaults(hip_lib_path):
    lib = ffi.load_library(hip_lib_path)
    assert ctypes.sizeof(ffi.AmbientParams) == 40 and ffi.AmbientParams.grid.offset == 24 and ffi.AmbientParams.min_loci.offset == 32
    assert ctypes.sizeof(ffi.AmbientSummary) == 6 * 8 + 4 * 4 + 8 + 3 * 64 * 8
    assert ffi.AmbientSummary.j_star.offset == 48 and ffi.AmbientSummary.n_cells_used.offset == 64
    assert ffi.AmbientSummary.source_rho.offset == 72 and ffi.AmbientSummary.source_cells.offset == 72 + 1024
    p = ffi.AmbientParams()
    assert lib.cellector_ambient_default_params(ctypes.byref(p)) == 0
    assert {k: getattr(p, k) for k, _ in ffi.AmbientParams._fields_} == ambient.DEFAULTS == dict(err=0.01, lo=0.0, hi=0.5, grid=16, rounds=3,
                                                                                                 min_loci=1)
    assert lib.cellector_ambient_default_params(None) == 1


def test_null_ctx_is_refused(hip_lib_path):
    lib = ffi.load_library(hip_lib_path)
    assert lib.cellector_ambient_tables(None, None, 8, 0.01, None, None) == 1
    assert lib.cellector_ambient_profile(None, None, 3, None, None, 8, 0.01, 1, *([None] * 9)) == 1
    assert lib.cellector_estimate_ambient(None, None, 3, *([None] * 7)) == 1


def test_header_states_the_model():
    beg = HEADER.index("ambient fraction estimation")
    block = HEADER[beg:HEADER.index("cellector_status cellector_ambient_default_params(")]
    for word in ("soup", "source_total", "source_cells", "at_boundary", "CELLECTOR_ENOMEM", "CELLECTOR_EINVAL", "255", "row order", "h = 128",
                 "sqrt", "2^-40", "unresolved", "min_loci", "ROUND 0", "log_likelihood", "tab1[l][g]", "ambient = rho_j", "64 G", "8 G + 21",
                 "cellector_cell_log_likelihoods invalidates"):
        assert word in block, word


def test_donor_codes():
    gt = np.array([[0, 1, 2, 3], [3, 3, 0, 1]], np.uint8)
    out = genotypes.donor_codes(gt)
    assert out.dtype == np.uint8 and out.tolist() == [[3, 2, 1, 0], [0, 0, 3, 2]]
    assert [genotypes.GT_STRINGS[c] for c in (1, 2, 3, 0)] == ["1/1", "0/1", "0/0", "./."]  # ... which donor_codes maps to 2, 1, 0, 3


def test_estimate_ambient_usage_errors_and_help(host_bin, tmp_path):
    base = [host_bin, "-a", "a.mtx", "-r", "r.mtx", "--barcodes", "b.tsv", "--output_directory", str(tmp_path / "o")]
    r = subprocess.run(base + ["--vcf", "v.vcf", "--estimate_ambient", "true"], capture_output=True, text=True)
    assert r.returncode == 1 and "'--estimate_ambient <true|apply>' requires '--donors <vcf>'" in r.stderr
    r = subprocess.run(base + ["--donors", "d.vcf", "--estimate_ambient", "apply"], capture_output=True, text=True)
    assert r.returncode == 1 and "'--donors <vcf>' requires '--vcf <vcf>'" in r.stderr
    r = subprocess.run(base + ["--vcf", "v.vcf", "--donors", "d.vcf", "--donor_ambient", "0.1", "--estimate_ambient", "apply"],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "'--estimate_ambient apply' cannot be used with '--donor_ambient <a>'" in r.stderr
    r = subprocess.run(base + ["--vcf", "v.vcf", "--donors", "d.vcf", "--estimate_ambient", "maybe"], capture_output=True, text=True)
    assert r.returncode != 0 and "expected true, apply or false" in r.stderr
    assert not os.path.exists(tmp_path / "o")
    r = subprocess.run([host_bin, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--estimate_ambient <true|apply>" in r.stdout
    for word in ("cellector_ambient.tsv", "cellector_ambient_cells.tsv", "--donor_ambient"):
        assert word in r.stdout, word
