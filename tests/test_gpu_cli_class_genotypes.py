"""GPU: `host/cellector --classes <file> --class_doublets true --refine_classes 3 --vcf <vcf> --class_genotypes true` on a small
mixture of three genotypes.  cellector_classes.vcf is rebuilt here byte for byte from the class_assignment column of the run's own
cellector_classes.tsv, the twin's tallies of the input matrices and the oracle's genotype call rendered like Rust's `{}`;
cellector_class_concordance.tsv is the rendering of genotypes.concordance; without the flag neither file exists and every other
output is the same."""
import os
import subprocess

import numpy as np
import pytest

import class_reference as cr
from test_host_cli import host_bin, rust_display  # noqa: F401

pytestmark = pytest.mark.gpu

NAMES = ["donorB", "donorA", "third"]  # numbered by first appearance in the file
NEW = ["cellector_class_concordance.tsv", "cellector_classes.vcf"]


@pytest.fixture(scope="module")
def runs(host_bin, tmp_path_factory):
    from cellector_amd import synth
    tmp = str(tmp_path_factory.mktemp("class_genotypes"))
    L, N, coo, truth = cr.mixture()
    alt, ref = synth.write_mtx_pair(tmp, L, N, *coo, header_nnz=0)
    bc = os.path.join(tmp, "barcodes.tsv")
    synth.write_barcodes(bc, N)
    barcodes = open(bc).read().splitlines()
    rng = np.random.default_rng(31)
    lab = truth.astype(np.uint8).copy()
    r = rng.random(N)
    lab[r < 0.1] = rng.integers(0, 3, int((r < 0.1).sum()))
    lab[r > 0.95] = 255
    lab[:3] = [0, 1, 2]
    cf = os.path.join(tmp, "classes.tsv")
    with open(cf, "w") as f:
        f.writelines(f"{barcodes[i]}\t{NAMES[lab[i]]}\n" for i in range(N) if lab[i] != 255)
    vcf = os.path.join(tmp, "variants.vcf")
    with open(vcf, "w") as f:
        f.write("##fileformat=VCFv4.2\n##source=synthetic\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        f.writelines(f"chr{1 + l % 22}\t{1000 + 37 * l}\t.\tA\tG\t50\tPASS\t.\n" for l in range(L))
    out = {}
    for name, extra in (("without", []), ("with", ["--class_genotypes", "true"])):
        d = os.path.join(tmp, name)
        cmd = [host_bin, "-a", alt, "-r", ref, "--output_directory", d, "--min_alt", "4", "--min_ref", "4", "--barcodes", bc, "--classes", cf,
               "--class_doublets", "true", "--refine_classes", "3", "--vcf", vcf] + extra
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr
        out[name] = dict(dir=d, stdout=res.stdout, stderr=res.stderr)
    return dict(L=L, N=N, coo=coo, vcf=vcf, **out)


def test_without_the_flag_nothing_changes(runs):
    a, b = runs["without"], runs["with"]
    files = sorted(os.listdir(a["dir"]))
    assert "cellector.vcf" in files and "cellector_classes.tsv" in files and not set(NEW) & set(files)
    assert sorted(os.listdir(b["dir"])) == sorted(files + NEW)
    assert a["stdout"] == b["stdout"] and a["stderr"] == b["stderr"]
    for f in files:
        assert open(os.path.join(a["dir"], f), "rb").read() == open(os.path.join(b["dir"], f), "rb").read(), f


def test_the_vcf_and_the_concordance(runs, oracle_lib):
    from cellector_amd import genotypes as gn
    L, N, d = runs["L"], runs["N"], runs["with"]["dir"]
    rows = [ln.split("\t") for ln in open(os.path.join(d, "cellector_classes.tsv")).read().splitlines()][1:]
    assert len(rows) == N
    called = [x[2] for x in rows]
    assert set(called) <= set(NAMES) | {"doublet", "unassigned"} and "unassigned" in called and set(NAMES) <= set(called)
    lab = np.array([NAMES.index(x) if x in NAMES else 255 for x in called], np.uint8)
    cells, alt, ref = gn.class_genotype_tallies(L, runs["coo"], lab, 3)
    tot_a, tot_r = alt.sum(axis=0), ref.sum(axis=0)
    gt = np.zeros((3, L), np.uint8)
    want = []
    rec = 0
    for ln in open(runs["vcf"]).read().splitlines():
        if ln.startswith("##"):
            want.append(ln)
        elif ln.startswith("#CHROM"):
            want.append(ln + "".join("\t" + n for n in NAMES))
        else:
            cols = []
            for k in range(3):
                a, r = int(alt[k, rec]), int(ref[k, rec])
                _, _, g, p = oracle_lib.vcf_genotype(a, r, int(tot_a[rec]) - a, int(tot_r[rec]) - r)
                gt[k, rec] = g
                cols.append(f"{gn.GT_STRINGS[g]}:{rust_display(p)}:{a}:{r}")
            want.append(ln + "\tGT:GP:AO:RO\t" + "\t".join(cols))
            rec += 1
    assert rec == L
    got = open(os.path.join(d, "cellector_classes.vcf"), "rb").read()
    assert got == ("\n".join(want) + "\n").encode()
    assert {1, 2, 3} <= set(np.unique(gt).tolist())  # all three genotypes occur
    both, disc = gn.concordance(gt)
    text = "class_a\tclass_b\tboth_called\tdiscordant\n"
    for a in range(3):
        for b in range(a + 1, 3):
            text += f"{NAMES[a]}\t{NAMES[b]}\t{both[a, b]}\t{disc[a, b]}\n"
    assert open(os.path.join(d, "cellector_class_concordance.tsv")).read() == text
    assert disc[0, 1] > 0 and both[0, 1] > disc[0, 1]
