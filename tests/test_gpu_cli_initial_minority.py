"""GPU: `host/cellector --initial_minority <file>` — the loop starts from the named cells as the exclusion set
(the reference's main.rs:37 starts from the empty one) and everything else, every output file included, is what it was."""
import os
import subprocess

import numpy as np
import pytest

from test_host_cli import host_bin  # noqa: F401

L, N, D, SEED = 1500, 800, 0.1, 11


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    from cellector_amd import synth
    tmp = str(tmp_path_factory.mktemp("initial_minority"))
    coo = synth.generate_coo(L, N, D, seed=SEED, minority_fraction=0.08)
    alt, ref = synth.write_mtx_pair(tmp, L, N, *coo, header_nnz=0)
    bc = os.path.join(tmp, "barcodes.tsv")
    synth.write_barcodes(bc, N)
    names = open(bc).read().split()
    flags = (np.random.default_rng(1).random(N) < 0.1).astype(np.uint8)
    start = os.path.join(tmp, "start.tsv")
    with open(start, "w") as f:  # the shape of a filtered cellector_assignments.tsv: barcode first, more columns, a blank line
        for i in np.nonzero(flags)[0]:
            f.write(f"{names[i]}\t0\t0\t-1.5\n")
        f.write("\n")
    return dict(tmp=tmp, coo=coo, alt=alt, ref=ref, bc=bc, names=names, flags=flags, start=start)


def _run(host_bin, inp, out, *extra, env=None):
    cmd = [host_bin, "-a", inp["alt"], "-r", inp["ref"], "--output_directory", out, "--min_alt", "4", "--min_ref", "4",
           "--barcodes", inp["bc"]] + list(extra)
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)


def _label_columns(out):
    rows = [ln.split("\t") for ln in open(os.path.join(out, "cellector_assignments.tsv")).read().splitlines()]
    return [(r[0], r[1], r[2], r[4], r[5]) for r in rows[1:]]  # barcode, label, anomaly, loci, qual


@pytest.mark.gpu
def test_warm_start_matches_the_oracle_from_set_excluded(host_bin, oracle_lib, inputs, tmp_path):
    out = str(tmp_path / "warm")
    r = _run(host_bin, inputs, out, "--initial_minority", inputs["start"])
    assert r.returncode == 0, r.stderr
    o = oracle_lib.Oracle.from_mtx(inputs["alt"], inputs["ref"], 4, 4)
    o.set_excluded(inputs["flags"])
    lines = [ln for ln in r.stdout.splitlines() if not ln.startswith("filtering locus")]
    it = 0
    while True:
        s = o.em_iteration(5.0)
        assert lines[2 * it] == (f"detected {s.n_new_excluded} new anomylous cells and rescued {s.n_rescued} cells to the "
                                 f"majority in iteration {it + 1}")
        tok = lines[2 * it + 1].split()
        assert tok[:4] == ["median", "normalized", "log", "likelihood"]
        assert float(tok[4]) == pytest.approx(s.median, abs=1e-9) and float(tok[-1]) == pytest.approx(s.threshold, abs=1e-9)
        assert float(tok[tok.index("range") + 1].rstrip(",")) == pytest.approx(s.iqr, abs=1e-9)
        it += 1
        if not s.any_change:
            break
    assert it == 2 and lines[0].startswith("detected 64 new anomylous cells and rescued 68 cells")  # counted against the start
    assert not os.path.exists(os.path.join(out, f"iteration_{it}.tsv"))
    po = o.posteriors()
    pa, aa, q = o.assignments(po["posterior"], po["doublet_posterior"], 0.999, 30)
    names = {0: "0", 1: "1", 2: "doublet", 3: "unassigned"}
    co = o.cell_outputs()
    cols = _label_columns(out)
    assert len(cols) == N
    for c, (bc, label, anomaly, loci, qual) in enumerate(cols):
        assert bc == inputs["names"][c] and label == names[pa[c]] and anomaly == str(aa[c]) and int(loci) == int(co["loci_used"][c])
        assert int(qual) == int(q[c]), (bc, qual, int(q[c]))
    # the same run sharded over two logical shards of the GPU
    out2 = str(tmp_path / "warm2")
    r2 = _run(host_bin, inputs, out2, "--initial_minority", inputs["start"], "--devices", "0,0")
    assert r2.returncode == 0, r2.stderr
    assert _label_columns(out2) == cols
    assert [ln for ln in r2.stdout.splitlines() if ln.startswith("detected")] == [ln for ln in lines if ln.startswith("detected")]
    # ... and with the near ties resolved on one GPU
    out3 = str(tmp_path / "warm3")
    r3 = _run(host_bin, inputs, out3, "--initial_minority", inputs["start"], "--resolve_near_ties", "true")
    assert r3.returncode == 0, r3.stderr
    assert [c[:3] for c in _label_columns(out3)] == [c[:3] for c in cols]


@pytest.mark.gpu
def test_absent_flag_and_empty_file_write_the_same_files(host_bin, inputs, tmp_path):
    empty = tmp_path / "empty.tsv"
    empty.write_text("\n\n")
    outs, stdouts = [], []
    for name, extra in (("plain", []), ("empty", ["--initial_minority", str(empty)])):
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


@pytest.mark.gpu
def test_unknown_barcode_and_unreadable_file(host_bin, inputs, tmp_path):
    bad = tmp_path / "bad.tsv"
    bad.write_text(inputs["names"][3] + "\n\nNOT_A_BARCODE-1\tx\n")
    r = _run(host_bin, inputs, str(tmp_path / "o"), "--initial_minority", str(bad))
    assert r.returncode == 1 and "NOT_A_BARCODE-1" in r.stderr and "line 3" in r.stderr
    r = _run(host_bin, inputs, str(tmp_path / "o"), "--initial_minority", str(tmp_path / "nope.tsv"))
    assert r.returncode != 0 and "couldn't open file" in r.stderr


def test_help_lists_the_flag(host_bin):
    r = subprocess.run([host_bin, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--initial_minority <file>" in r.stdout
    assert "--devices <a,b,...>" in r.stdout and "--resolve_assignments" in r.stdout
    r = subprocess.run([host_bin, "-a", "a", "-r", "r", "-b", "b", "--output_directory", "o", "--initial_minority"],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "requires a value" in r.stderr
