"""CPU: the donor pair fraction calls are declared behind the ambient block, exported and bound with the header's argument names; the
header states the model; the struct layouts and the defaults; a null ctx is refused; the binding's argument checks; the twin's
functions; the host binary's usage errors and help text for --doublet_fraction."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from cellector_amd import ffi, pair_fraction
from test_host_cli import host_bin  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "cellector_ffi.h")).read()

ARGS = {
    "cellector_pair_fraction_default_params": ["out"],
    "cellector_pair_fraction_tables": ["ctx", "donor_params", "frac", "n_grid", "mask", "tab"],
    "cellector_donor_pair_fractions": ["ctx", "gt", "n_donors", "donor_params", "params", "pair_a", "pair_b", "frac", "n_grid", "mask", "ll",
                                       "n_entries", "cell_frac", "cell_se", "j_star", "kind", "summary", "tab"],
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
    for m in ("pair_fraction_default_params", "pair_fraction_tables", "donor_pair_fractions"):
        assert callable(getattr(ffi.Cellector, m))
    # behind the ambient block, in front of what followed it
    at = [HEADER.index(s) for s in ("cellector_status cellector_estimate_ambient(", "cellector_status cellector_pair_fraction_default_params(",
                                    "cellector_status cellector_pair_fraction_tables(", "cellector_status cellector_donor_pair_fractions(",
                                    "cellector_status cellector_final_allele_tallies(")]
    assert at == sorted(at)
    for f in ("tables", "cell_sums", "fractions", "kinds"):
        assert callable(getattr(pair_fraction, f)), f


def test_struct_layouts_and_defaults(hip_lib_path):
    lib = ffi.load_library(hip_lib_path)
    assert ctypes.sizeof(ffi.PairFractionParams) == 16 and ffi.PairFractionParams.min_loci.offset == 8
    assert ctypes.sizeof(ffi.PairFractionSummary) == 5 * 8 + 64 * 8 and ffi.PairFractionSummary.donor_cells.offset == 40
    assert ffi.PairFractionSummary.n_none.offset == 32
    p = ffi.PairFractionParams()
    assert lib.cellector_pair_fraction_default_params(ctypes.byref(p)) == 0
    assert {k: getattr(p, k) for k, _ in ffi.PairFractionParams._fields_} == pair_fraction.DEFAULTS == dict(min_fraction=0.1, min_loci=1)
    assert lib.cellector_pair_fraction_default_params(None) == 1
    assert pair_fraction.DEFAULT_GRID.tolist() == [j / 16.0 for j in range(17)]
    assert pair_fraction.KIND_NAMES == {0: "balanced", 1: "toward_a", 2: "toward_b", 3: "flat", 255: "NA"}


def test_null_ctx_is_refused(hip_lib_path):
    lib = ffi.load_library(hip_lib_path)
    assert lib.cellector_pair_fraction_tables(None, None, None, 17, None, None) == 1
    assert lib.cellector_donor_pair_fractions(None, None, 3, None, None, None, None, None, 17, *([None] * 9)) == 1


def test_header_states_the_model():
    beg = HEADER.index("donor pair fractions")
    block = HEADER[beg:HEADER.index("cellector_status cellector_pair_fraction_default_params(")]
    for word in ("pair_a == 255", "strictly ascending", "j / 16.0", "4 g_a + g_b", "256 G", "16 G bytes", "tab2[l][4 g_a + g_b]", "tab1[l][g_a]",
                 "tab1[l][g_b]", "pair_ll[c][b]", "anchor[c] = a", "row order", "unresolved", "j_star", "min_fraction", "min_loci", "no zoom",
                 "toward a", "toward b", "balanced", "flat", "CELLECTOR_EINVAL", "CELLECTOR_ENOMEM", "8 G + 24", "first\n * offending cell",
                 "[0, 0.5]", "EM state is never touched", "cellector_cell_log_likelihoods invalidates"):
        assert word in block, word


class _Dims:
    total_cells, total_loci, loci_used, cell_begin, cell_end = 5, 7, 6, 0, 5


def test_binding_argument_checks():
    """the checks the binding makes before the library is called, on an object that holds no ctx"""
    g = object.__new__(ffi.Cellector)
    g.dims = lambda: _Dims
    g.donor_default_params = lambda: ffi.DonorParams()
    g.pair_fraction_default_params = lambda: ffi.PairFractionParams()
    gt, a, b = np.zeros((3, 7), np.uint8), np.zeros(5, np.uint8), np.ones(5, np.uint8)
    with pytest.raises(ValueError, match=r"gt: shape \(D, 7\)"):
        g.donor_pair_fractions(np.zeros((3, 6), np.uint8), a, b)
    with pytest.raises(ValueError, match="pair_a: 5 values"):
        g.donor_pair_fractions(gt, a[:4], b)
    with pytest.raises(ValueError, match="pair_b: 5 values"):
        g.donor_pair_fractions(gt, a, np.ones((5, 1), np.uint8))
    with pytest.raises(ValueError, match="frac: one dimension"):
        g.donor_pair_fractions(gt, a, b, frac=np.zeros((2, 4)))
    with pytest.raises(ValueError, match="frac: one dimension"):
        g.pair_fraction_tables(frac=np.zeros((2, 4)))
    with pytest.raises(ValueError, match="mask: 6 entries"):
        g.donor_pair_fractions(gt, a, b, mask=np.ones(7, np.uint8))
    with pytest.raises(TypeError, match="unknown parameter 'min_frac'"):
        g.donor_pair_fractions(gt, a, b, params=dict(min_frac=0.2))
    with pytest.raises(TypeError, match="unknown parameter 'rate'"):
        g.donor_pair_fractions(gt, a, b, donor_params=dict(rate=0.2))
    with pytest.raises(TypeError, match="unknown parameter"):
        pair_fraction.pair_fractions(None, None, a, b, params=dict(min_frac=0.2))


def test_doublet_fraction_usage_errors_and_help(host_bin, tmp_path):
    base = [host_bin, "-a", "a.mtx", "-r", "r.mtx", "--barcodes", "b.tsv", "--output_directory", str(tmp_path / "o")]
    r = subprocess.run(base + ["--vcf", "v.vcf", "--doublet_fraction", "true"], capture_output=True, text=True)
    assert r.returncode == 1 and "'--doublet_fraction true' requires '--donors <vcf>'" in r.stderr
    r = subprocess.run(base + ["--vcf", "v.vcf", "--doublet_min_fraction", "0.2"], capture_output=True, text=True)
    assert r.returncode == 1 and "'--doublet_min_fraction <m>' requires '--doublet_fraction true'" in r.stderr
    r = subprocess.run(base + ["--vcf", "v.vcf", "--donors", "d.vcf", "--doublet_fraction", "maybe"], capture_output=True, text=True)
    assert r.returncode != 0 and "expected true or false" in r.stderr
    for v in ("0.6", "-0.1", "nan"):
        r = subprocess.run(base + ["--vcf", "v.vcf", "--donors", "d.vcf", "--doublet_fraction", "true", "--doublet_min_fraction", v],
                           capture_output=True, text=True)
        assert r.returncode == 1 and f"Invalid value '{v}' for '--doublet_min_fraction <m>': expected a number in [0, 0.5]" in r.stderr, v
    assert not os.path.exists(tmp_path / "o")
    r = subprocess.run([host_bin, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--doublet_fraction <true>" in r.stdout
    for word in ("cellector_doublet_fractions.tsv", "--doublet_min_fraction"):
        assert word in r.stdout, word
