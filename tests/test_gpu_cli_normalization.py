"""GPU: `host/cellector --normalization zscore` — the loop scores by the z-score of main.rs:317-318 (option normalization = 1),
iteration_N.tsv gets a seventh column expected_log_variance, the normalised column of cellector_assignments.tsv holds the z-score;
without the flag, or with per_locus, every file and stdout are what they were."""
import os
import subprocess

import numpy as np
import pytest

from test_host_cli import host_bin, rust_display  # noqa: F401

pytestmark = pytest.mark.gpu

L, N, D, SEED = 1500, 800, 0.1, 11


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    from cellector_amd import synth
    tmp = str(tmp_path_factory.mktemp("normalization"))
    coo = synth.generate_coo(L, N, D, seed=SEED, minority_fraction=0.08)
    alt, ref = synth.write_mtx_pair(tmp, L, N, *coo, header_nnz=0)
    bc = os.path.join(tmp, "barcodes.tsv")
    synth.write_barcodes(bc, N)
    return dict(coo=coo, alt=alt, ref=ref, bc=bc, names=open(bc).read().split())


def _run(host_bin, inp, out, *extra):
    cmd = [host_bin, "-a", inp["alt"], "-r", inp["ref"], "--output_directory", out, "--min_alt", "4", "--min_ref", "4",
           "--barcodes", inp["bc"]] + list(extra)
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600)


def _table(path):
    rows = [ln.split("\t") for ln in open(path).read().splitlines()]
    return rows[0], rows[1:]


def test_zscore_files_are_the_python_loop(host_bin, inputs, tmp_path):
    from cellector_amd import Cellector
    out = str(tmp_path / "z")
    r = _run(host_bin, inputs, out, "--normalization", "zscore")
    assert r.returncode == 0, r.stderr
    g = Cellector(0)
    g.set_option("normalization", 1)
    g.load_mtx(inputs["alt"], inputs["ref"], 4, 4)
    it = 0
    while True:
        s = g.em_iteration(5.0)
        co, var = g.cell_outputs(), g.cell_variances()
        head, rows = _table(os.path.join(out, f"iteration_{it}.tsv"))
        assert head == ["cell_id", "barcode", "assignment", "log_likelihood", "expected_log_likelihood", "num_loci_used",
                        "expected_log_variance"]
        assert len(rows) == N and all(len(x) == 7 for x in rows)
        assert [x[6] for x in rows] == [rust_display(v) for v in var], it
        assert [x[3] for x in rows] == [rust_display(v) for v in co["ll"]], it
        assert open(os.path.join(out, f"iteration_{it}_threshold.tsv")).read() == rust_display(s.threshold)
        it += 1
        if not s.any_change:
            break
    assert it >= 2 and not os.path.exists(os.path.join(out, f"iteration_{it}.tsv"))
    assert (var > 0).all()
    head, rows = _table(os.path.join(out, "cellector_assignments.tsv"))
    assert head[3] == "log_likelihood_loci_normalized" and len(rows) == N
    assert [x[3] for x in rows] == [rust_display(v) for v in co["normalized"]]  # the last iteration's z-scores
    z = (co["ll"] - co["expected_ll"]) / np.sqrt(var)
    assert np.allclose(co["normalized"], z, rtol=1e-14, atol=0) and not np.allclose(co["normalized"], co["ll"] / co["loci_used"])
    assert [x[2] for x in rows] == ["0" if e else "1" for e in g.excluded()]
    assert [x[0] for x in rows] == inputs["names"][:N]
    g.close()


def test_absent_flag_and_per_locus_write_the_same_files(host_bin, inputs, tmp_path):
    outs, stdouts = [], []
    for name, extra in (("plain", []), ("per_locus", ["--normalization", "per_locus"])):
        out = str(tmp_path / name)
        r = _run(host_bin, inputs, out, *extra)
        assert r.returncode == 0, r.stderr
        outs.append(out)
        stdouts.append(r.stdout)
    assert stdouts[0] == stdouts[1] and stdouts[0].startswith("detected 70 new anomylous cells and rescued 0 cells")
    files = sorted(os.listdir(outs[0]))
    assert files == sorted(os.listdir(outs[1])) and "cellector_assignments.tsv" in files and "iteration_1.tsv" in files
    for f in files:
        assert open(os.path.join(outs[0], f), "rb").read() == open(os.path.join(outs[1], f), "rb").read(), f
    head, rows = _table(os.path.join(outs[0], "iteration_0.tsv"))
    assert len(head) == 6 and all(len(x) == 6 for x in rows)
