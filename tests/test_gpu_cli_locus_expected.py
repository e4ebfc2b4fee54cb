"""GPU: `host/cellector --locus_expected true` — the columns expected_loglike_minority / _majority of every
iteration_N_locus_contribution.tsv hold the library's locus moments (option locus_moments = 1) instead of a copy of the two columns
before them, and four columns follow majority_af: the two variances and the two z-scores; every other byte is the plain run's.
With false every file and stdout are the plain run's."""
import os
import subprocess

import numpy as np
import pytest

from test_host_cli import host_bin, rust_display  # noqa: F401

pytestmark = pytest.mark.gpu

L, N, D = 2000, 1000, 0.10  # matrix B of tests/test_gpu_cell_variance.py
HEAD17 = ["locus_id", "chrom", "pos", "log_likelihood_minority", "log_likelihood_majority", "expected_loglike_minority",
          "expected_loglike_majority", "minority_cellcount", "majority_cellcount", "log_likelihood_minority_per_cell",
          "log_likelihood_majority_per_cell", "minority_alt", "minority_ref", "majority_alt", "majority_ref", "minority_af", "majority_af"]
NEW4 = ["variance_minority", "variance_majority", "zscore_minority", "zscore_majority"]


@pytest.fixture(scope="module")
def runs(host_bin, tmp_path_factory):
    from cellector_amd import synth
    tmp = str(tmp_path_factory.mktemp("locus_expected"))
    coo = synth.generate_coo(L, N, D)
    alt, ref = synth.write_mtx_pair(tmp, L, N, *coo, header_nnz=0)
    bc = os.path.join(tmp, "barcodes.tsv")
    synth.write_barcodes(bc, N)
    out = {}
    for name, extra in (("plain", []), ("false", ["--locus_expected", "false"]), ("true", ["--locus_expected", "true"])):
        d = os.path.join(tmp, name)
        cmd = [host_bin, "-a", alt, "-r", ref, "--output_directory", d, "--min_alt", "4", "--min_ref", "4", "--barcodes", bc] + extra
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        out[name] = dict(dir=d, stdout=r.stdout)
    return dict(alt=alt, ref=ref, **out)


def _table(path):
    rows = [ln.split("\t") for ln in open(path).read().splitlines()]
    return rows[0], rows[1:]


def test_false_is_the_plain_run(runs):
    a, b = runs["plain"], runs["false"]
    assert a["stdout"] == b["stdout"] and a["stdout"].startswith("detected ")
    files = sorted(os.listdir(a["dir"]))
    assert files == sorted(os.listdir(b["dir"])) and "iteration_0_locus_contribution.tsv" in files
    for f in files:
        assert open(os.path.join(a["dir"], f), "rb").read() == open(os.path.join(b["dir"], f), "rb").read(), f
    head, rows = _table(os.path.join(a["dir"], "iteration_0_locus_contribution.tsv"))
    assert head == HEAD17 and all(len(x) == 17 for x in rows)
    assert all(x[5] == x[3] and x[6] == x[4] for x in rows)  # quirk Q6: the copy


def test_true_holds_the_library_vectors(runs):
    from cellector_amd import Cellector
    a, t = runs["plain"], runs["true"]
    assert a["stdout"] == t["stdout"]
    files = sorted(os.listdir(a["dir"]))
    assert files == sorted(os.listdir(t["dir"]))
    locus_files = [f for f in files if f.endswith("_locus_contribution.tsv")]
    assert len(locus_files) >= 2
    for f in files:
        if f not in locus_files:
            assert open(os.path.join(a["dir"], f), "rb").read() == open(os.path.join(t["dir"], f), "rb").read(), f
    g = Cellector(0)
    g.set_option("locus_moments", 1)
    g.load_mtx(runs["alt"], runs["ref"], 4, 4)
    ids = g.locus_ids()
    index = {str(int(v)): i for i, v in enumerate(ids)}
    differs = 0
    for it in range(len(locus_files)):
        s = g.em_iteration(5.0)
        mo, lo = g.iter_locus_moments(), g.locus_outputs()
        z_min = Cellector.locus_zscore(lo["contrib_min"], mo["exp_min"], mo["var_min"], lo["cells_min"])
        z_maj = Cellector.locus_zscore(lo["contrib_maj"], mo["exp_maj"], mo["var_maj"], lo["cells_maj"])
        head_a, rows_a = _table(os.path.join(a["dir"], f"iteration_{it}_locus_contribution.tsv"))
        head_t, rows_t = _table(os.path.join(t["dir"], f"iteration_{it}_locus_contribution.tsv"))
        assert head_a == HEAD17 and head_t == HEAD17 + NEW4
        assert len(rows_t) == len(rows_a) == len(ids) and all(len(x) == 21 for x in rows_t)
        for ra, rt in zip(rows_a, rows_t):  # the row order and every other column of the first 17 are the plain run's
            assert ra[:5] == rt[:5] and ra[7:] == rt[7:17], (it, ra[0])
            l = index[rt[0]]
            want = [mo["exp_min"][l], mo["exp_maj"][l]]
            assert rt[5:7] == [rust_display(v) for v in want], (it, l)
            assert rt[17:] == [rust_display(v) for v in (mo["var_min"][l], mo["var_maj"][l], z_min[l], z_maj[l])], (it, l)
            differs += rt[5:7] != rt[3:5]
        assert (it == len(locus_files) - 1) == (not s.any_change)
        assert (mo["var_maj"] > 0).any() and np.isfinite(z_maj).all() and np.isfinite(z_min).all()
        if lo["cells_min"].any():
            assert z_min.any(), it
    assert differs > len(ids)  # no longer the copy
    g.close()
