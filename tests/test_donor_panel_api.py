"""CPU: the donor panel's C ABI as the binding sees it (exports, signatures, the summary's size), the Python signatures and the twin's
argument errors."""
import ctypes
import inspect

import numpy as np
import pytest

import donor_reference as dr
from cellector_amd import cluster, donors, ffi
from test_donors_api import _prototype
from test_host_cli import host_bin  # noqa: F401


@pytest.mark.parametrize("name, n_args", [("cellector_donor_panel", 27), ("cellector_match_donors_panel", 11)])
def test_signatures_follow_the_header(hip_lib_path, name, n_args):
    args = _prototype(name)
    res, argtypes = ffi.SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == len(argtypes) == n_args
    for a, t in zip(args, argtypes):
        want = ctypes.c_void_p if "*" in a else ctypes.c_uint32 if a.startswith("uint32_t") else None
        assert t is want, (name, a, t)
    assert hasattr(ffi.load_library(hip_lib_path), name)


def test_struct_layout_and_null_arguments(hip_lib_path):
    assert ctypes.sizeof(ffi.DonorPanelSummary) == 40 and ffi.DonorPanelSummary.n_present.offset == 32
    assert [f for f, _ in ffi.DonorPanelSummary._fields_] == ["n_singlet", "n_doublet", "n_ambiguous", "n_unassigned", "n_present"]
    lib = ffi.load_library(hip_lib_path)
    assert lib.cellector_donor_panel(None, None, 1, 8, *([None] * 23)) == 1  # (a null ctx)
    assert lib.cellector_match_donors_panel(None, None, 1, None, 1, *([None] * 6)) == 1


def test_python_signatures():
    sig = inspect.signature(ffi.Cellector.donor_panel)
    assert list(sig.parameters)[:8] == ["self", "gt", "shortlist", "log_prior", "anchor", "mask", "ll", "tables"]
    assert sig.parameters["shortlist"].default == 8 and sig.parameters["ll"].default is False and sig.parameters["tables"].default is False
    assert list(inspect.signature(ffi.Cellector.match_donors_panel).parameters)[:5] == ["self", "labels", "n_classes", "gt", "mask"]
    sig = inspect.signature(donors.panel_posteriors)
    assert list(sig.parameters)[:5] == ["mat", "gt_used", "alt_total", "ref_total", "shortlist"] and sig.parameters["shortlist"].default == 8
    assert inspect.signature(donors.panel_present).parameters["min_cells"].default == 1
    assert donors.PANEL_NONE == 65535 and donors.PANEL_MAX_DONORS == 4096


def test_the_twins_argument_errors():
    L, N, coo = dr.case_matrix()
    A, R = dr.totals(L, coo)
    mat = cluster.Matrix(L, N, coo)
    for m in (0, 65):
        with pytest.raises(ValueError, match="shortlist"):
            donors.panel_posteriors(mat, dr.case_gt(5), A, R, m)
    with pytest.raises(ValueError, match="1..4096"):
        donors.panel_posteriors(mat, np.zeros((4097, L), np.uint8), A, R)
    with pytest.raises(ValueError, match="1..4096"):
        donors.panel_posteriors(mat, np.zeros((0, L), np.uint8), A, R)
    with pytest.raises(TypeError, match="unknown parameter"):
        donors.panel_posteriors(mat, dr.case_gt(5), A, R, nonsense=1)
    res = dict(donor_cells=np.array([0, 3, 1, 0, 7], np.uint64))
    assert donors.panel_present(res).tolist() == [1, 2, 4] and donors.panel_present(res, 2).tolist() == [1, 4]
    assert donors.panel_present(res, 0).tolist() == [1, 2, 4] and donors.panel_present(res, 8).tolist() == []


def test_cli_usage_errors(host_bin, tmp_path):
    import os
    import subprocess
    base = [host_bin, "-a", "a.mtx", "-r", "r.mtx", "--barcodes", "b.tsv", "--output_directory", str(tmp_path / "o")]
    with_donors = base + ["--vcf", "v.vcf", "--donors", "d.vcf"]
    for cmd, message in ((base + ["--donor_panel", "8"], "'--donor_panel <M>' requires '--donors <vcf>'"),
                         (with_donors + ["--donor_panel", "8", "--donor_field", "GP"], "'--donor_panel <M>' cannot be used with '--donor_field GP'"),
                         (with_donors + ["--donor_panel", "0"], "Invalid value '0' for '--donor_panel <M>'"),
                         (with_donors + ["--donor_panel", "65"], "Invalid value '65' for '--donor_panel <M>'"),
                         (with_donors + ["--donor_panel_min_cells", "3"], "'--donor_panel_min_cells <n>' requires '--donor_panel <M>'"),
                         (with_donors + ["--donor_panel", "8", "--donor_panel_min_cells", "0"], "Invalid value '0' for '--donor_panel_min_cells <n>'"),
                         (with_donors + ["--donor_panel", "8", "--devices", "0,0"], "works on one GPU")):
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 1 and message in r.stderr, (cmd, r.stderr)
        assert not os.path.exists(tmp_path / "o")
    r = subprocess.run([host_bin, "--help"], capture_output=True, text=True)
    for flag in ("--donor_panel <M>", "--donor_panel_min_cells <n>", "cellector_donor_panel_donors.tsv"):
        assert flag in r.stdout, flag
