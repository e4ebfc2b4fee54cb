"""GPU: `host/cellector --vcf <vcf> --donors <vcf> --estimate_ambient <true|apply>` on the planted pool of
ambient_reference.planted (rho 0.08).  true: cellector_ambient.tsv and cellector_ambient_cells.tsv hold the Python binding's
estimate_ambient of the donor pass' singlets rendered the same way, one line more on stdout, and every other output file is the
run's without the flag, byte for byte.  apply: the donor files are those of a run with --donor_ambient <the estimate printed>."""
import os
import subprocess

import numpy as np
import pytest

import ambient_reference as ar
from test_host_cli import host_bin, rust_display  # noqa: F401

pytestmark = pytest.mark.gpu

DONORS = ["alice", "bob", "carol"]
CLASSES = ["x", "y"]
GT_TEXT = {0: "0/0", 1: "0|1", 2: "1/1", 3: "./."}
PLANTED = 0.08


def _vcfs(vcf, dvcf, gt):
    L = gt.shape[1]
    with open(vcf, "w") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        for i in range(L):
            f.write(f"chr{1 + i % 3}\t{100 + i}\t.\tA\tG\t.\t.\t.\n")
    with open(dvcf, "w") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(DONORS) + "\n")
        for i in range(L):
            f.write(f"chr{1 + i % 3}\t{100 + i}\t.\tA\tG\t.\t.\t.\tGT\t" + "\t".join(GT_TEXT[int(g)] for g in gt[:, i]) + "\n")


@pytest.fixture(scope="module")
def runs(host_bin, tmp_path_factory):
    from cellector_amd import synth
    tmp = str(tmp_path_factory.mktemp("ambient"))
    L, N, coo, gt, truth = ar.planted(PLANTED, 0)
    alt, ref = synth.write_mtx_pair(tmp, L, N, *[np.asarray(x, np.uint32) for x in coo], header_nnz=0)
    bc = os.path.join(tmp, "barcodes.tsv")
    synth.write_barcodes(bc, N)
    barcodes = open(bc).read().splitlines()
    gt = gt.copy()
    gt[:, ::11] = 3  # (some loci without a call)
    vcf, dvcf = os.path.join(tmp, "variants.vcf"), os.path.join(tmp, "donors.vcf")
    _vcfs(vcf, dvcf, gt)
    cf = os.path.join(tmp, "classes.tsv")
    with open(cf, "w") as f:
        for i in range(N):
            f.write(f"{barcodes[i]}\t{CLASSES[i % 2]}\n")
    out = {}

    def run(name, extra):
        d = os.path.join(tmp, name)
        cmd = [host_bin, "-a", alt, "-r", ref, "--output_directory", d, "--min_alt", "4", "--min_ref", "4", "--barcodes", bc, "--vcf", vcf,
               "--donors", dvcf, "--donor_error", "0.02", "--classes", cf] + extra
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        out[name] = dict(dir=d, stdout=r.stdout, stderr=r.stderr)

    run("plain", [])
    run("true", ["--estimate_ambient", "true"])
    run("apply", ["--estimate_ambient", "apply"])
    line = [ln for ln in out["apply"]["stdout"].splitlines() if ln.startswith("ambient: rho=")]
    assert len(line) == 1
    printed = line[0].split()[1][len("rho="):]
    run("direct", ["--donor_ambient", printed])
    return dict(alt=alt, ref=ref, bc=bc, barcodes=barcodes, gt=gt, vcf=vcf, dvcf=dvcf, printed=printed, **out)


NEW = ["cellector_ambient.tsv", "cellector_ambient_cells.tsv"]


def test_true_adds_exactly_the_two_files(runs):
    a, b = runs["plain"], runs["true"]
    files = sorted(os.listdir(a["dir"]))
    assert not any("ambient" in f for f in files) and "cellector_donors.tsv" in files and "cellector_cluster_donors.tsv" in files
    assert sorted(os.listdir(b["dir"])) == sorted(files + NEW)
    for f in files:
        assert open(os.path.join(a["dir"], f), "rb").read() == open(os.path.join(b["dir"], f), "rb").read(), f
    extra = [ln for ln in b["stdout"].splitlines() if ln.startswith("ambient: ")]
    assert len(extra) == 1 and [ln for ln in b["stdout"].splitlines() if not ln.startswith("ambient: ")] == a["stdout"].splitlines()
    assert "ambient:" not in a["stdout"]


def _na(v):
    return "NA" if v != v else rust_display(float(v))


def test_the_values_are_the_bindings(runs):
    from cellector_amd import Cellector
    g = Cellector(0)
    g.load_mtx(runs["alt"], runs["ref"], 4, 4)
    r = g.donor_posteriors(runs["gt"], min_loci=30, posterior_threshold=0.999, err=0.02)
    assign = np.where(r["status"] == 0, r["best"], 255).astype(np.uint8)
    assert (assign != 255).sum() > 200  # (the pool is planted: most cells are singlets of their donor)
    e = g.estimate_ambient(runs["gt"], assign, err=0.02)
    g.close()
    # (no recovery claim here: this run scores at --donor_error 0.02 and on the loci --min_alt 4 --min_ref 4 leave, not under the
    # model the pool was planted with; test_gpu_ambient.py holds the estimate to the planted value)
    assert e["curvature"] < 0 and not e["at_boundary"] and np.isfinite(e["se"])
    for name in ("true", "apply"):
        d = runs[name]["dir"]
        assert f"ambient: rho={rust_display(e['rho'])} se={rust_display(e['se'])} cells={e['n_cells_used']} at_boundary={e['at_boundary']}" \
            in runs[name]["stdout"].splitlines()
        rows = [ln.split("\t") for ln in open(os.path.join(d, "cellector_ambient.tsv")).read().splitlines()]
        assert rows[0] == ["source", "cells", "rho", "se"] and len(rows) == 5
        assert rows[1] == ["pool", str(e["n_cells_used"]), rust_display(e["rho"]), rust_display(e["se"])]
        for k in range(3):
            assert rows[2 + k] == [DONORS[k], str(int(e["source_cells"][k])), _na(e["source_rho"][k]), _na(e["source_se"][k])]
        rows = [ln.split("\t") for ln in open(os.path.join(d, "cellector_ambient_cells.tsv")).read().splitlines()]
        assert rows[0] == ["barcode", "donor", "n_loci", "rho", "se"] and len(rows) == len(assign) + 1
        for c in range(len(assign)):
            if assign[c] == 255:
                want = [runs["barcodes"][c], "NA", "NA", "NA", "NA"]
            else:
                want = [runs["barcodes"][c], DONORS[assign[c]], str(int(e["n_entries"][c])), _na(e["cell_rho"][c]), _na(e["cell_se"][c])]
            assert rows[1 + c] == want, c
    assert runs["printed"] == rust_display(e["rho"])


def test_apply_writes_the_donor_files_of_the_estimate(runs):
    a, b, plain = runs["apply"], runs["direct"], runs["plain"]
    assert sorted(os.listdir(a["dir"])) == sorted(os.listdir(b["dir"]) + NEW)
    for f in sorted(os.listdir(b["dir"])):
        assert open(os.path.join(a["dir"], f), "rb").read() == open(os.path.join(b["dir"], f), "rb").read(), f
    for f in ("cellector_donors.tsv", "cellector_cluster_donors.tsv"):  # (and they are not the files of the default 0.03)
        assert open(os.path.join(a["dir"], f), "rb").read() != open(os.path.join(plain["dir"], f), "rb").read(), f
    # the ambient files of apply are those of true: they come from the first donor pass
    for f in NEW:
        assert open(os.path.join(a["dir"], f), "rb").read() == open(os.path.join(runs["true"]["dir"], f), "rb").read(), f


def test_usage_errors(host_bin, runs, tmp_path):
    base = [host_bin, "-a", runs["alt"], "-r", runs["ref"], "--output_directory", str(tmp_path / "o"), "--barcodes", runs["bc"]]
    r = subprocess.run(base + ["--vcf", runs["vcf"], "--estimate_ambient", "true"], capture_output=True, text=True)
    assert r.returncode == 1 and "'--estimate_ambient <true|apply>' requires '--donors <vcf>'" in r.stderr
    r = subprocess.run(base + ["--vcf", runs["vcf"], "--donors", runs["dvcf"], "--estimate_ambient", "apply", "--donor_ambient", "0.05"],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "cannot be used with '--donor_ambient <a>'" in r.stderr
    r = subprocess.run(base + ["--vcf", runs["vcf"], "--donors", runs["dvcf"], "--estimate_ambient", "maybe"], capture_output=True, text=True)
    assert r.returncode != 0 and "expected true, apply or false" in r.stderr
    assert not os.path.exists(tmp_path / "o")
