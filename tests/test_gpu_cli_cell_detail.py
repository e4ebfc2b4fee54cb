"""GPU: `host/cellector --cell_detail <file>` writes cell_detail.tsv — per listed barcode, one row per entry of its matrix row with
the PMFData values (cellector_cell_pmfs) under the alpha / beta the loop ended with and the entry's log-pmf under the minority,
majority and doublet distributions of the posterior phase — and changes nothing else: every other file and stdout are the bytes of
a run without the flag."""
import os
import subprocess

import numpy as np
import pytest

from test_host_cli import _write_inputs, host_bin, rust_display  # noqa: F401

pytestmark = pytest.mark.gpu

L, N = 1500, 700
HEADER = ["cell_id", "barcode", "locus_id", "chrom", "pos", "alt", "ref", "used", "alpha", "beta", "log_pmf", "expected_log_pmf",
          "expected_log_variance", "minority_log_pmf", "majority_log_pmf", "doublet_log_pmf"]


def _run(host_bin, inp, out, *extra):
    cmd = [host_bin, "-a", inp["alt"], "-r", inp["ref"], "--output_directory", out, "--min_alt", "4", "--min_ref", "4",
           "--barcodes", inp["bc"], "--vcf", inp["vcf"], "-g", inp["gt"]] + list(extra)
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def runs(host_bin, hip_lib_path, tmp_path_factory):
    """the inputs, the library's own run of them, a run without the flag and one with it"""
    from cellector_amd import Cellector
    tmp = str(tmp_path_factory.mktemp("cell_detail"))
    coo, alt, ref, bc, gt, vcf = _write_inputs(tmp, L, N, 0.12, seed=4, minority=0.08)
    inp = dict(tmp=tmp, alt=alt, ref=ref, bc=bc, gt=gt, vcf=vcf, names=open(bc).read().split())
    g = Cellector(0)
    g.load_mtx(alt, ref, 4, 4)
    g.run()
    exc = np.nonzero(g.excluded())[0]
    inc = np.nonzero(g.excluded() == 0)[0]
    assert len(exc) >= 4 and len(inc) >= 6
    cells = [int(exc[0]), int(inc[0]), int(exc[1]), int(inc[-1]), int(inc[1]), int(exc[-1]), int(inc[2]), int(exc[2]), int(inc[3]),
             int(exc[0])]  # ten barcodes, finally excluded and not, one given twice
    lst = os.path.join(tmp, "detail.tsv")
    with open(lst, "w") as f:
        for i, c in enumerate(cells):
            f.write(inp["names"][c] + ("\tsome\tmore\n" if i % 3 == 0 else "\n"))
            if i == 4:
                f.write("\n")
    plain, detail = os.path.join(tmp, "plain"), os.path.join(tmp, "detail")
    r0 = _run(host_bin, inp, plain)
    r1 = _run(host_bin, inp, detail, "--cell_detail", lst)
    return dict(inp=inp, g=g, cells=cells, lst=lst, plain=plain, detail=detail, r0=r0, r1=r1)


def _rows(out):
    rows = [ln.split("\t") for ln in open(os.path.join(out, "cell_detail.tsv")).read().splitlines()]
    assert rows[0] == HEADER
    return rows[1:]


def _close(a, b):
    return abs(a - b) <= 1e-9 * max(1.0, abs(b))


def test_the_file_is_the_librarys_records(runs):
    r, g, cells, inp = runs["r1"], runs["g"], runs["cells"], runs["inp"]
    assert r.returncode == 0, r.stderr
    rows = _rows(runs["detail"])
    a, b = g.alpha_betas()
    used = g.loci_mask()
    ids = g.locus_ids()
    rec = g.cell_pmfs(cells, a, b, np.ones(len(a), np.uint8))
    post = [g.cell_pmfs(cells, *g.posterior_alpha_betas(w), np.ones(len(a), np.uint8))["log_pmf"] for w in (0, 1, 2)]
    n = int(rec["rec_ptr"][-1])
    assert len(rows) == n > 0
    cell_of = np.repeat(cells, np.diff(rec["rec_ptr"].astype(np.int64)))
    vcf = [ln.split("\t")[:2] for ln in open(inp["vcf"]) if not ln.startswith("#")]
    for i, row in enumerate(rows):
        l = int(rec["locus_index"][i])
        assert row[:8] == [str(cell_of[i]), inp["names"][cell_of[i]], str(ids[l]), vcf[ids[l]][0], vcf[ids[l]][1], str(rec["alt"][i]),
                           str(rec["ref"][i]), str(int(used[l]))], i
        assert float(row[8]) == a[l] and float(row[9]) == b[l]
        if used[l]:
            assert [float(x) for x in row[10:13]] == [rec["log_pmf"][i], rec["expected_log_pmf"][i], rec["expected_log_variance"][i]], i
        else:  # "na" exactly where used == 0
            assert row[10:13] == ["na"] * 3, i
        assert "na" not in row[13:] and [float(x) for x in row[13:]] == [post[w][i] for w in range(3)], i
        for x in row[8:]:
            assert x == "na" or rust_display(float(x)) == x, x
    # per barcode: the posterior phase's sums (cellector_assignments.tsv) and the cell pass' under the final mask
    asg = {t[0]: t for t in (ln.split("\t") for ln in open(os.path.join(runs["detail"], "cellector_assignments.tsv")).read().splitlines()[1:])}
    ll = g.cell_log_likelihoods(a, b, used)[0]
    for j, c in enumerate(cells):
        sel = slice(int(rec["rec_ptr"][j]), int(rec["rec_ptr"][j + 1]))
        rs = rows[sel]
        assert _close(sum(float(x[13]) for x in rs), float(asg[inp["names"][c]][7])), c  # minority_log_likelihood
        assert _close(sum(float(x[14]) for x in rs), float(asg[inp["names"][c]][6])), c  # majority_log_likelihood
        assert _close(sum(float(x[10]) for x in rs if x[7] == "1"), ll[c]), c


def test_nothing_else_changes(runs):
    r0, r1 = runs["r0"], runs["r1"]
    assert r0.returncode == 0 and r1.returncode == 0, (r0.stderr, r1.stderr)
    assert r0.stdout == r1.stdout
    f0, f1 = sorted(os.listdir(runs["plain"])), sorted(os.listdir(runs["detail"]))
    assert f1 == sorted(f0 + ["cell_detail.tsv"]) and "cellector.vcf" in f0
    for f in f0:
        assert open(os.path.join(runs["plain"], f), "rb").read() == open(os.path.join(runs["detail"], f), "rb").read(), f


def test_sharded_run_writes_the_same_bytes(host_bin, runs):
    out = os.path.join(runs["inp"]["tmp"], "sharded")
    r = _run(host_bin, runs["inp"], out, "--cell_detail", runs["lst"], "--devices", "0,0")
    assert r.returncode == 0, r.stderr
    assert open(os.path.join(out, "cell_detail.tsv"), "rb").read() == open(os.path.join(runs["detail"], "cell_detail.tsv"), "rb").read()


def test_unknown_barcode_and_help(host_bin, runs, tmp_path):
    bad = tmp_path / "bad.tsv"
    bad.write_text(runs["inp"]["names"][3] + "\nNOT_A_BARCODE-1\n")
    r = _run(host_bin, runs["inp"], str(tmp_path / "o"), "--cell_detail", str(bad))
    assert r.returncode != 0 and "NOT_A_BARCODE-1" in r.stderr
    r = subprocess.run([host_bin, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--cell_detail <file>" in r.stdout and "(not in the reference)" in r.stdout
