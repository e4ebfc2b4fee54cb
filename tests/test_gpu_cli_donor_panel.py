"""GPU: `host/cellector --vcf <vcf> --donors <panel vcf> --donor_panel <M>` on the planted pool written as files: the three planted
donors in shuffled columns of a 100-sample VCF among 97 decoys.  cellector_donor_panel.tsv and cellector_donor_panel_donors.tsv are
the Python binding's donor_panel of the same genotypes rendered the same way (the binding is held to the twin and the reference in
test_gpu_donor_panel.py); the donors present are read from the binding, never from the planted truth; every file from the donor pass on
is the run with --donors on a VCF that holds only those columns, byte for byte; every other output is the run's without the flags."""
import os
import subprocess

import numpy as np
import pytest

import donor_panel_reference as pn
from test_host_cli import host_bin, rust_display  # noqa: F401

pytestmark = pytest.mark.gpu

SEED, D, M = 5, 100, 8
GT_TEXT = {0: "0/0", 1: "0|1", 2: "1/1", 3: "./."}
STATUS = {0: "singlet", 1: "doublet", 2: "ambiguous", 255: "unassigned"}
PANEL_FILES = ["cellector_donor_panel.tsv", "cellector_donor_panel_donors.tsv"]


def _variant_vcf(path, L):
    with open(path, "w") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        for i in range(L):
            f.write(f"chr{1 + i % 3}\t{100 + i}\t.\tA\tG\t.\t.\t.\n")


def _donor_vcf(path, gt, names):
    """every fifth record is left out, every seventh has ref and alt swapped (its calls written mirrored), one extra record"""
    with open(path, "w") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names) + "\n")
        f.write("chr9\t1\t.\tA\tG\t.\t.\t.\tGT" + "\t1/1" * len(names) + "\n")
        for i in range(gt.shape[1]):
            if i % 5 == 4:
                continue
            swap = i % 7 == 3
            calls = [GT_TEXT[int(g) if g == 3 or not swap else 2 - int(g)] for g in gt[:, i]]
            f.write(f"chr{1 + i % 3}\t{100 + i}\t.\t{'G' if swap else 'A'}\t{'A' if swap else 'G'}\t.\t.\t.\tGT:DP\t" +
                    "\t".join(c + ":7" for c in calls) + "\n")


@pytest.fixture(scope="module")
def runs(host_bin, hip_lib_path, tmp_path_factory):
    from cellector_amd import Cellector, donors, synth
    tmp = str(tmp_path_factory.mktemp("donor_panel"))
    L, N, coo, gt, rows, truth, par = pn.planted_panel(SEED, D)
    gt = gt.copy()
    gt[:, 4::5] = 3  # (the records the donor VCF leaves out)
    names = [f"donor{k:03d}" for k in range(D)]
    alt, ref = synth.write_mtx_pair(tmp, L, N, *(np.asarray(x, np.uint32) for x in coo), header_nnz=0)
    bc = os.path.join(tmp, "barcodes.tsv")
    synth.write_barcodes(bc, N)
    barcodes = open(bc).read().splitlines()
    vcf, pvcf, svcf = (os.path.join(tmp, n) for n in ("variants.vcf", "panel.vcf", "subset.vcf"))
    _variant_vcf(vcf, L)
    _donor_vcf(pvcf, gt, names)
    # the binding's call under the CLI's parameters, and the donors it finds present
    g = Cellector(0)
    g.load_mtx(alt, ref, 4, 4)
    res = g.donor_panel(gt, M, min_loci=30, posterior_threshold=0.999)
    g.close()
    present = donors.panel_present(res)
    assert 1 <= len(present) <= 64, len(present)
    _donor_vcf(svcf, gt[present], [names[k] for k in present])
    labels = (np.arange(N) % 2).astype(np.uint8)
    cf = os.path.join(tmp, "classes.tsv")
    with open(cf, "w") as f:
        for i in range(N):
            f.write(f"{barcodes[i]}\t{'xy'[labels[i]]}\n")
    base = [host_bin, "-a", alt, "-r", ref, "--min_alt", "4", "--min_ref", "4", "--barcodes", bc, "--vcf", vcf]
    more = ["--donor_fit", "true", "--doublet_fraction", "true"]
    huge = ["--donors", pvcf, "--donor_panel", str(M), "--donor_panel_min_cells", "1000000"]
    out = {}
    for name, extra, rc in (("plain", [], 0), ("panel", ["--donors", pvcf, "--donor_panel", str(M)], 0), ("subset", ["--donors", svcf], 0),
                            ("panel_more", ["--donors", pvcf, "--donor_panel", str(M), "--classes", cf] + more, 0),
                            ("subset_more", ["--donors", svcf, "--classes", cf] + more, 0),
                            ("nobody", huge, 0), ("nobody_fit", huge + ["--donor_fit", "true"], 1)):
        d = os.path.join(tmp, name)
        r = subprocess.run(base + ["--output_directory", d] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == rc, (name, r.stderr)
        out[name] = dict(dir=d, stdout=r.stdout, stderr=r.stderr)
    return dict(alt=alt, ref=ref, barcodes=barcodes, gt=gt, names=names, res=res, present=present, labels=labels, N=N, **out)


def _read(run, name):
    return open(os.path.join(run["dir"], name), "rb").read()


def test_the_panel_files_are_the_binding(runs):
    r, names, N = runs["res"], runs["names"], runs["N"]
    rows = [ln.split("\t") for ln in _read(runs["panel"], PANEL_FILES[0]).decode().splitlines()]
    head = ["barcode", "status", "donor", "second_donor", "best_pair", "posterior", "pair_posterior", "doublet_posterior", "n_loci"]
    for j in range(M):
        head += [f"candidate_{j}", f"log_likelihood_{j}", f"posterior_{j}"]
    assert rows[0] == head and len(rows) == N + 1
    for c in range(N):
        b, a, p = int(r["best"][c]), int(r["anchor"][c]), int(r["best_pair"][c])
        slot = np.flatnonzero(r["cand"][c] == p)
        want = [runs["barcodes"][c], STATUS[int(r["status"][c])], names[b], names[int(r["second"][c])],
                "NA" if p == 65535 else f"{names[a]}+{names[p]}", rust_display(float(r["best_posterior"][c])),
                rust_display(float(r["cand_pair_posterior"][c, slot[0]]) if len(slot) else 0.0),
                rust_display(float(r["doublet_posterior"][c])), str(int(r["n_entries"][c]))]
        for j in range(M):
            want += [names[int(r["cand"][c, j])], rust_display(float(r["cand_ll"][c, j])), rust_display(float(r["cand_posterior"][c, j]))]
        assert rows[1 + c] == want, c
    dbl = np.zeros(D, np.int64)
    for c in np.flatnonzero((r["status"] == 1) & (r["best_pair"] != 65535)):
        dbl[r["anchor"][c]] += 1
        dbl[r["best_pair"][c]] += 1
    rows = [ln.split("\t") for ln in _read(runs["panel"], PANEL_FILES[1]).decode().splitlines()]
    assert rows[0] == ["donor", "singlet_cells", "doublet_cells", "present"] and len(rows) == D + 1
    for k in range(D):
        assert rows[1 + k] == [names[k], str(int(r["donor_cells"][k])), str(int(dbl[k])), "1" if k in runs["present"] else "0"], k
    s = r["summary"]
    line = (f"donor_panel: {D} donors, shortlist {M}, singlet={s.n_singlet} doublet={s.n_doublet} ambiguous={s.n_ambiguous} "
            f"unassigned={s.n_unassigned} present={len(runs['present'])}")
    assert line in runs["panel"]["stderr"] and s.n_present == len(runs["present"])


def test_the_donor_pass_is_the_run_on_the_present_donors_alone(runs):
    for panel, subset, new in (("panel", "subset", PANEL_FILES), ("panel_more", "subset_more", PANEL_FILES + ["cellector_cluster_panel_donors.tsv"])):
        a, b = runs[subset], runs[panel]
        files = sorted(os.listdir(a["dir"]))
        assert "cellector_donors.tsv" in files and sorted(os.listdir(b["dir"])) == sorted(files + new)
        for f in files:
            assert _read(a, f) == _read(b, f), (panel, f)
        assert a["stdout"] == b["stdout"]
        assert f"donors: {len(runs['present'])} donors" in b["stderr"]
    for f in ("cellector_donor_fit.tsv", "cellector_doublet_fractions.tsv", "cellector_cluster_donors.tsv"):
        assert f in os.listdir(runs["panel_more"]["dir"]), f


def test_the_class_match_is_the_binding(runs):
    from cellector_amd import Cellector
    g = Cellector(0)
    g.load_mtx(runs["alt"], runs["ref"], 4, 4)
    m = g.match_donors_panel(runs["labels"], 2, runs["gt"], min_loci=30, posterior_threshold=0.999)
    g.close()
    rows = [ln.split("\t") for ln in _read(runs["panel_more"], "cellector_cluster_panel_donors.tsv").decode().splitlines()]
    assert rows[0] == ["class", "cells", "donor", "margin"] and len(rows) == 3
    for k in range(2):
        assert rows[1 + k] == ["xy"[k], str(int(m["cells"][k])), runs["names"][int(m["best"][k])], rust_display(float(m["margin"][k]))]


def test_every_other_output_is_the_run_without_the_flags(runs):
    a, b = runs["plain"], runs["panel"]
    files = sorted(os.listdir(a["dir"]))
    assert not any("donor" in f for f in files) and a["stdout"] == b["stdout"]
    assert sorted(os.listdir(b["dir"])) == sorted(files + PANEL_FILES + ["cellector_donors.tsv"])
    for f in files:
        assert _read(a, f) == _read(b, f), f


def test_nobody_present_skips_the_donor_pass(runs):
    for name in ("nobody", "nobody_fit"):
        r = runs[name]
        assert "donor_panel: 0 donors are present, the donor pass takes 1..64: skipped" in r["stderr"] and "present=0" in r["stderr"]
        assert sorted(os.listdir(r["dir"])) == sorted(os.listdir(runs["plain"]["dir"]) + PANEL_FILES)
        assert _read(r, PANEL_FILES[0]) == _read(runs["panel"], PANEL_FILES[0])
        assert all(ln.endswith("\t0") for ln in _read(r, PANEL_FILES[1]).decode().splitlines()[1:])
    assert "--donor_fit" in runs["nobody_fit"]["stderr"] and "found 0 donors present" in runs["nobody_fit"]["stderr"]
