"""GPU: `host/cellector --donors <vcf> --donor_field <GT|GP|GL|PL>` — with GP cellector_donors.tsv holds the Python binding's
donor_posteriors_gp of the same weights rendered the same way, and with --classes cellector_cluster_donors.tsv its match_donors_gp;
with GT every file and stdout are the run's without the flag, byte for byte."""
import os
import subprocess

import numpy as np
import pytest

from test_host_cli import host_bin, rust_display  # noqa: F401

pytestmark = pytest.mark.gpu

L, N, D = 1500, 700, 0.10
DONORS = ["alice", "bob", "carol"]
CLASSES = ["x", "y"]
GT_TEXT = {0: "0/0", 1: "0|1", 2: "1/1", 3: "./."}


def _variant_vcf(path):
    with open(path, "w") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        for i in range(L):
            f.write(f"chr{1 + i % 3}\t{100 + i}\t.\tA\tG\t.\t.\t.\n")


def _donor_vcf(path, gt, gp):
    """every fifth record is left out, every seventh has ref and alt swapped (its calls mirrored, its weights reversed); a sample
    whose weights are NaN has '.' for its GP and falls back to its GT"""
    with open(path, "w") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(DONORS) + "\n")
        for i in range(L):
            if i % 5 == 4:
                continue
            swap = i % 7 == 3
            cols = []
            for d in range(3):
                g = int(gt[d, i])
                call = GT_TEXT[g if g == 3 or not swap else 2 - g]
                row = gp[d, i][::-1] if swap else gp[d, i]
                cols.append(call + ":" + ("." if np.isnan(row).any() else ",".join(repr(float(x)) for x in row)))
            f.write(f"chr{1 + i % 3}\t{100 + i}\t.\t{'G' if swap else 'A'}\t{'A' if swap else 'G'}\t.\t.\t.\tGT:GP\t" + "\t".join(cols) + "\n")


@pytest.fixture(scope="module")
def runs(host_bin, tmp_path_factory):
    from cellector_amd import donors, synth
    tmp = str(tmp_path_factory.mktemp("donor_field"))
    coo = synth.generate_coo(L, N, D)
    alt, ref = synth.write_mtx_pair(tmp, L, N, *coo, header_nnz=0)
    bc = os.path.join(tmp, "barcodes.tsv")
    synth.write_barcodes(bc, N)
    barcodes = open(bc).read().splitlines()
    rng = np.random.default_rng(23)
    gt = rng.choice(4, (3, L), p=[0.4, 0.3, 0.2, 0.1]).astype(np.uint8)
    gt[:, 4::5] = 3  # (the records the donor VCF leaves out)
    # the weights written: a third of the rows soft (float32 values, so that their shortest decimal form reads back exactly), a third
    # without a GP (the reader falls back to GT: one-hot, or no call), the others one-hot
    written = np.full((3, L, 3), np.nan, np.float32)
    kind = rng.integers(0, 3, (3, L))
    soft = rng.dirichlet(np.ones(3), (3, L)).astype(np.float32)
    written[kind == 0] = soft[kind == 0]
    one = donors.one_hot(gt)
    written[(kind == 1) & (gt < 3)] = one[(kind == 1) & (gt < 3)]
    written[:, 4::5] = np.nan
    want = np.where(np.isnan(written), one, written)  # what the reader must return: the fallback where no GP was written
    want[:, 4::5] = np.nan
    vcf, dvcf = os.path.join(tmp, "variants.vcf"), os.path.join(tmp, "donors.vcf")
    _variant_vcf(vcf)
    _donor_vcf(dvcf, gt, written)
    lab = (np.arange(N) % 2).astype(np.uint8)
    lab[4::9] = 255
    cf = os.path.join(tmp, "classes.tsv")
    with open(cf, "w") as f:
        for i in range(N):
            if lab[i] != 255:
                f.write(f"{barcodes[i]}\t{CLASSES[lab[i]]}\n")
    out = {}
    for name, extra in (("run_plain", []), ("run_gt", ["--donor_field", "GT"]), ("run_gp", ["--donor_field", "GP"])):
        d = os.path.join(tmp, name)
        cmd = [host_bin, "-a", alt, "-r", ref, "--output_directory", d, "--min_alt", "4", "--min_ref", "4", "--barcodes", bc, "--vcf", vcf,
               "--classes", cf, "--donors", dvcf] + extra
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        out[name] = dict(dir=d, stdout=r.stdout, stderr=r.stderr)
    return dict(alt=alt, ref=ref, barcodes=barcodes, gt=gt, gp=want, vcf=vcf, dvcf=dvcf, labels=lab, **out)


def test_the_donor_vcf_reads_back(runs):
    from cellector_amd import donors
    names, gp = donors.read_donor_vcf_gp(runs["dvcf"], runs["vcf"], "GP")
    assert names == DONORS and gp.tobytes() == runs["gp"].tobytes()
    assert (np.isnan(gp).all(axis=2) | ~np.isnan(gp).any(axis=2)).all() and np.isnan(gp).any() and (donors.soft_weights(gp, np.arange(L))[1] == 4).any()


def test_gt_is_the_run_without_the_flag(runs):
    a, b = runs["run_plain"], runs["run_gt"]
    files = sorted(os.listdir(a["dir"]))
    assert "cellector_donors.tsv" in files and "cellector_cluster_donors.tsv" in files and sorted(os.listdir(b["dir"])) == files
    assert a["stdout"] == b["stdout"]
    for f in files:
        assert open(os.path.join(a["dir"], f), "rb").read() == open(os.path.join(b["dir"], f), "rb").read(), f
    # ... and with GP only the two donor files differ
    c = runs["run_gp"]
    assert sorted(os.listdir(c["dir"])) == files and a["stdout"] == c["stdout"]
    for f in files:
        same = open(os.path.join(a["dir"], f), "rb").read() == open(os.path.join(c["dir"], f), "rb").read()
        assert same == (f not in ("cellector_donors.tsv", "cellector_cluster_donors.tsv")), f


def test_the_gp_tables_are_the_binding(runs):
    from cellector_amd import Cellector
    g = Cellector(0)
    g.load_mtx(runs["alt"], runs["ref"], 4, 4)
    status = {0: "singlet", 1: "doublet", 2: "ambiguous", 255: "unassigned"}
    head = ["barcode", "status", "donor", "second_donor", "best_pair", "posterior", "pair_posterior", "doublet_posterior", "n_loci"] + \
           [f"log_likelihood_{n}" for n in DONORS]
    r = g.donor_posteriors_gp(runs["gp"], min_loci=30, posterior_threshold=0.999)
    rows = [ln.split("\t") for ln in open(os.path.join(runs["run_gp"]["dir"], "cellector_donors.tsv")).read().splitlines()]
    assert rows[0] == head and len(rows) == N + 1
    for c in range(N):
        b, p = int(r["best"][c]), int(r["best_pair"][c])
        want = [runs["barcodes"][c], status[int(r["status"][c])], DONORS[b], DONORS[int(r["second"][c])], f"{DONORS[b]}+{DONORS[p]}",
                rust_display(float(r["posterior"][c, b])), rust_display(float(r["pair_posterior"][c, p])),
                rust_display(float(r["doublet_posterior"][c])), str(int(r["n_entries"][c]))] + \
               [rust_display(float(r["ll"][c, d])) for d in range(3)]
        assert rows[1 + c] == want, c
    s = r["summary"]
    assert f"singlet={s.n_singlet} doublet={s.n_doublet} ambiguous={s.n_ambiguous} unassigned={s.n_unassigned}" in runs["run_gp"]["stderr"]
    m = g.match_donors_gp(runs["labels"], 2, runs["gp"], min_loci=30, posterior_threshold=0.999)
    rows = [ln.split("\t") for ln in open(os.path.join(runs["run_gp"]["dir"], "cellector_cluster_donors.tsv")).read().splitlines()]
    assert rows[0] == ["class", "cells", "donor", "margin"] + [f"log_likelihood_{n}" for n in DONORS] and len(rows) == 3
    for k in range(2):
        assert rows[1 + k] == [CLASSES[k], str(int(m["cells"][k])), DONORS[int(m["best"][k])], rust_display(float(m["margin"][k]))] + \
            [rust_display(float(m["ll"][k, d])) for d in range(3)]
    g.close()
