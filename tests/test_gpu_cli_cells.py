"""GPU: `host/cellector --cells <file>`, `--downsample_rate <r>` and `--seed <n>` — the run on a cell subset / on thinned reads,
cut on the device after the load (cellector_restage), is byte for byte the run of the binary WITHOUT the flags on files filtered
beforehand: a barcodes.tsv with only the listed lines and both matrices with only those columns, renumbered; or matrices written
from the numpy twin's thinned arrays."""
import os
import subprocess

import numpy as np
import pytest

from test_host_cli import _write_inputs, host_bin  # noqa: F401

L, N = 1500, 800


def _run(host_bin, inp, out, *extra, alt=None, ref=None, bc=None):
    cmd = [host_bin, "-a", alt or inp["alt"], "-r", ref or inp["ref"], "--output_directory", out, "--min_alt", "4", "--min_ref", "4",
           "--barcodes", bc or inp["bc"], "--vcf", inp["vcf"], "-g", inp["gt"]] + list(extra)
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600)


def _same_runs(r0, out0, r1, out1):
    assert r0.returncode == 0, r0.stderr
    assert r1.returncode == 0, r1.stderr
    assert r0.stdout == r1.stdout
    files = sorted(os.listdir(out0))
    assert files == sorted(os.listdir(out1)) and "cellector_assignments.tsv" in files and "cellector.vcf" in files
    for f in files:
        assert open(os.path.join(out0, f), "rb").read() == open(os.path.join(out1, f), "rb").read(), f
    return files


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    from cellector_amd import restage, synth
    tmp = str(tmp_path_factory.mktemp("cli_cells"))
    coo, alt, ref, bc, gt, vcf = _write_inputs(tmp, L, N, 0.1, seed=11, minority=0.08)
    names = open(bc).read().split()
    keep = np.random.default_rng(3).random(N) < 0.7
    keep[0], keep[N - 1] = False, True
    kept = np.nonzero(keep)[0]
    assert len(kept) == 569
    lst = os.path.join(tmp, "cells.tsv")
    with open(lst, "w") as f:  # any order, more columns, a blank line, a barcode twice: the SET counts
        for j, i in enumerate(np.random.default_rng(8).permutation(kept)):
            f.write(names[i] + ("\tx\ty\n" if j % 5 == 0 else "\n"))
            if j == 7:
                f.write("\n" + names[i] + "\n")
    every = os.path.join(tmp, "every.tsv")
    open(every, "w").write("\n".join(names) + "\n")
    start = os.path.join(tmp, "start.tsv")
    open(start, "w").write("".join(names[i] + "\n" for i in kept[np.random.default_rng(1).random(len(kept)) < 0.1]))
    detail = os.path.join(tmp, "detail.tsv")
    open(detail, "w").write("".join(names[i] + "\n" for i in kept[[0, 5, 300, 568]]))
    # the files a user would have filtered by hand
    sub = os.path.join(tmp, "subset")
    t = restage.restage_coo(*coo, N, keep)
    sub_alt, sub_ref = synth.write_mtx_pair(sub, L, t[4], *t[:4], header_nnz=0)
    sub_bc = os.path.join(sub, "barcodes.tsv")
    open(sub_bc, "w").write("".join(names[i] + "\n" for i in kept))
    thin = os.path.join(tmp, "thinned")
    t = restage.restage_coo(*coo, N, None, 0.6, 4)
    assert int(((t[2] == 0) & (t[3] == 0)).sum()) == 61634
    thin_alt, thin_ref = synth.write_mtx_pair(thin, L, N, *t[:4], header_nnz=0)
    return dict(tmp=tmp, alt=alt, ref=ref, bc=bc, gt=gt, vcf=vcf, names=names, keep=keep, lst=lst, every=every, start=start,
                detail=detail, sub=(sub_alt, sub_ref, sub_bc), thin=(thin_alt, thin_ref))


@pytest.mark.gpu
def test_cells_equals_a_run_on_filtered_files(host_bin, inputs, tmp_path):
    more = ["--initial_minority", inputs["start"], "--cell_detail", inputs["detail"]]
    o0, o1 = str(tmp_path / "filtered"), str(tmp_path / "flag")
    r0 = _run(host_bin, inputs, o0, *more, alt=inputs["sub"][0], ref=inputs["sub"][1], bc=inputs["sub"][2])
    r1 = _run(host_bin, inputs, o1, "--cells", inputs["lst"], *more)
    files = _same_runs(r0, o0, r1, o1)
    assert "cell_detail.tsv" in files
    rows = open(os.path.join(o1, "cellector_assignments.tsv")).read().splitlines()
    assert len(rows) == 1 + 569 and [r.split("\t")[0] for r in rows[1:]] == [n for n, k in zip(inputs["names"], inputs["keep"]) if k]
    assert any(r.split("\t")[-1] != "na" for r in rows[1:])  # the -g labels followed the cells


@pytest.mark.gpu
def test_downsample_equals_a_run_on_thinned_files(host_bin, inputs, tmp_path):
    o0, o1 = str(tmp_path / "files"), str(tmp_path / "flag")
    r0 = _run(host_bin, inputs, o0, alt=inputs["thin"][0], ref=inputs["thin"][1])
    r1 = _run(host_bin, inputs, o1, "--downsample_rate", "0.6", "--seed", "4")
    _same_runs(r0, o0, r1, o1)
    o2 = str(tmp_path / "default_seed")  # --seed defaults to 4
    _same_runs(r0, o0, _run(host_bin, inputs, o2, "--downsample_rate=0.6"), o2)
    o3 = str(tmp_path / "other_seed")
    r3 = _run(host_bin, inputs, o3, "--downsample_rate", "0.6", "--seed", "5")
    assert r3.returncode == 0 and open(os.path.join(o3, "iteration_0.tsv")).read() != open(os.path.join(o0, "iteration_0.tsv")).read()


@pytest.mark.gpu
def test_rate_zero_and_every_barcode_change_nothing(host_bin, inputs, tmp_path):
    o0, o1 = str(tmp_path / "plain"), str(tmp_path / "noop")
    r0 = _run(host_bin, inputs, o0)
    r1 = _run(host_bin, inputs, o1, "--downsample_rate", "0", "--cells", inputs["every"])
    _same_runs(r0, o0, r1, o1)
    assert r0.stdout.startswith("detected ")


@pytest.mark.gpu
def test_errors(host_bin, inputs, tmp_path):
    bad = tmp_path / "bad.tsv"
    bad.write_text(inputs["names"][3] + "\n\nNOT_A_BARCODE-1\tx\n")
    r = _run(host_bin, inputs, str(tmp_path / "o"), "--cells", str(bad))
    assert r.returncode == 1 and "NOT_A_BARCODE-1" in r.stderr and "line 3" in r.stderr and "--cells" in r.stderr
    r = _run(host_bin, inputs, str(tmp_path / "o"), "--cells", inputs["lst"], "--devices", "0,0")
    assert r.returncode == 1 and "--cells" in r.stderr and "--devices" in r.stderr
    r = _run(host_bin, inputs, str(tmp_path / "o"), "--downsample_rate", "0.5", "--devices", "0,0")
    assert r.returncode == 1 and "--downsample_rate" in r.stderr
    dropped = inputs["names"][0]  # cell 0 is not in the list
    det = tmp_path / "det.tsv"
    det.write_text(inputs["names"][799] + "\n" + dropped + "\n")
    for flag in ("--cell_detail", "--initial_minority"):
        r = _run(host_bin, inputs, str(tmp_path / "o"), "--cells", inputs["lst"], flag, str(det))
        assert r.returncode == 1 and dropped in r.stderr and "line 2" in r.stderr and "--cells" in r.stderr, r.stderr
    r = _run(host_bin, inputs, str(tmp_path / "o"), "--downsample_rate", "1.5")
    assert r.returncode == 1 and "[0, 1]" in r.stderr
    empty = tmp_path / "empty.tsv"
    empty.write_text("\n")
    r = _run(host_bin, inputs, str(tmp_path / "o"), "--cells", str(empty))
    assert r.returncode == 1 and "lists no barcode" in r.stderr


def test_help_lists_the_flags(host_bin):
    r = subprocess.run([host_bin, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--cells <file>", "--downsample_rate <r>", "--seed <n>"):
        assert flag in r.stdout, flag
