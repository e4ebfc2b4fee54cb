"""GPU: `host/cellector --cluster 3` on a small mixture of three genotypes: cellector_clusters.tsv holds the planted partition, one
row per barcode in barcode order, and no other output changes; with --refine_classes and --class_genotypes the clusters become the
classes (cellector_classes.tsv, cellector_classes.vcf: from no labels to a per-cluster VCF); --cluster with --classes is a usage
error; --help names the flags."""
import os
import subprocess

import numpy as np
import pytest

import class_reference as cr
from test_host_cli import host_bin  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def runs(host_bin, tmp_path_factory):
    from cellector_amd import synth
    tmp = str(tmp_path_factory.mktemp("cluster"))
    L, N, coo, truth = cr.mixture()
    alt, ref = synth.write_mtx_pair(tmp, L, N, *coo, header_nnz=0)
    bc = os.path.join(tmp, "barcodes.tsv")
    synth.write_barcodes(bc, N)
    vcf = os.path.join(tmp, "variants.vcf")
    with open(vcf, "w") as f:
        f.write("##fileformat=VCFv4.2\n##source=synthetic\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        f.writelines(f"chr{1 + l % 22}\t{1000 + 37 * l}\t.\tA\tG\t50\tPASS\t.\n" for l in range(L))
    base = [host_bin, "-a", alt, "-r", ref, "--min_alt", "4", "--min_ref", "4", "--barcodes", bc, "--vcf", vcf]
    out = dict(base=base, tmp=tmp, barcodes=open(bc).read().splitlines(), truth=truth, L=L, N=N)
    for name, extra in (("without", []), ("with", ["--cluster", "3", "--seed", "2"]), ("loop", ["--cluster", "3", "--cluster_mask", "loop", "--cluster_restarts", "8"]),
                        ("classes", ["--cluster", "3", "--refine_classes", "10", "--class_genotypes", "true"])):
        d = os.path.join(tmp, name)
        res = subprocess.run(base + ["--output_directory", d] + extra, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr
        out[name] = dict(dir=d, stdout=res.stdout, stderr=res.stderr)
    return out


def _clusters(runs, name):
    from cellector_amd import cluster as cl
    lines = open(os.path.join(runs[name]["dir"], "cellector_clusters.tsv")).read().splitlines()
    assert lines[0].split("\t") == ["barcode", "cluster"] + [f"posterior_{k}" for k in range(3)] + [f"log_likelihood_{k}" for k in range(3)]
    rows = [ln.split("\t") for ln in lines[1:]]
    assert [r[0] for r in rows] == runs["barcodes"] and all(len(r) == 8 for r in rows)
    lab = np.array([255 if r[1] == "unassigned" else int(r[1]) for r in rows], np.uint8)
    post, ll = np.array([[float(x) for x in r[2:5]] for r in rows]), np.array([[float(x) for x in r[5:8]] for r in rows])
    on = lab != 255
    assert np.array_equal(lab[on], np.argmax(ll[on], axis=1)) and np.allclose(post.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    assert (lab[:cr.MIX_N] != 255).all()
    return lab, cl.best_permutation(lab[:cr.MIX_N], runs["truth"][:cr.MIX_N], 3)


def test_the_partition_is_the_truths(runs):
    for name in ("with", "loop", "classes"):
        lab, (perm, agree) = _clusters(runs, name)
        assert agree == cr.MIX_N, (name, agree)
    assert "cluster: restart" in runs["with"]["stderr"] and " of 16," in runs["with"]["stderr"] and " of 8," in runs["loop"]["stderr"]


def test_no_other_output_changes(runs):
    a, b = runs["without"], runs["with"]
    files = sorted(os.listdir(a["dir"]))
    assert "cellector_clusters.tsv" not in files and "cellector_classes.tsv" not in files
    assert sorted(os.listdir(b["dir"])) == sorted(files + ["cellector_clusters.tsv"])
    assert a["stdout"] == b["stdout"]
    for f in files:
        assert open(os.path.join(a["dir"], f), "rb").read() == open(os.path.join(b["dir"], f), "rb").read(), f


def test_clusters_become_the_classes(runs):
    d = runs["classes"]["dir"]
    files = os.listdir(d)
    assert {"cellector_clusters.tsv", "cellector_classes.tsv", "cellector_classes.vcf", "cellector_class_concordance.tsv"} <= set(files)
    lab, _ = _clusters(runs, "classes")
    rows = [ln.split("\t") for ln in open(os.path.join(d, "cellector_classes.tsv")).read().splitlines()]
    assert rows[0][:4] == ["barcode", "input_label", "class_assignment", "qual"] and rows[0][4] == "log_likelihood_0"
    assert [r[1] for r in rows[1:]] == ["na" if x == 255 else str(x) for x in lab]
    assert "refine_classes step 1" in runs["classes"]["stderr"]
    head = [ln for ln in open(os.path.join(d, "cellector_classes.vcf")).read().splitlines() if ln.startswith("#CHROM")]
    assert head and head[0].split("\t")[-3:] == ["0", "1", "2"]


def test_usage(runs, host_bin):
    cf = os.path.join(runs["tmp"], "classes.tsv")
    with open(cf, "w") as f:
        f.write(f"{runs['barcodes'][0]}\tx\n")
    d = os.path.join(runs["tmp"], "refused")
    res = subprocess.run(runs["base"] + ["--output_directory", d, "--cluster", "3", "--classes", cf], capture_output=True, text=True, timeout=60)
    assert res.returncode == 1 and "'--cluster <K>' cannot be used with '--classes <file>'" in res.stderr and not os.path.exists(d)
    for extra, msg in ((["--cluster", "1"], "expected 2..16"), (["--cluster_restarts", "4"], "requires '--cluster <K>'"),
                       (["--cluster", "3", "--cluster_restarts", "22"], "expected 1..64 / K"), (["--cluster_mask", "loop"], "requires '--cluster <K>'")):
        res = subprocess.run(runs["base"] + ["--output_directory", d] + extra, capture_output=True, text=True, timeout=60)
        assert res.returncode == 1 and msg in res.stderr, (extra, res.stderr)
    res = subprocess.run([host_bin, "--help"], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0
    for flag in ("--cluster <K>", "--cluster_restarts <R>", "--cluster_mask <all|loop>"):
        assert flag in res.stdout, flag
