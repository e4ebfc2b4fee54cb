"""GPU: `host/cellector --donors <vcf> --donor_genotypes <true|apply>` — with true every other file and the rest of stdout are the
run's without the flag, byte for byte, and cellector_donor_genotypes.vcf / .tsv hold the Python binding's donor_genotypes rendered the
same way (the twin's rendering); with apply cellector_donors.tsv, cellector_cluster_donors.tsv, cellector_donor_fit.tsv and
cellector_doublet_fractions.tsv are those of a run given the refined genotypes beforehand as a --donor_field GP VCF; with --estimate_ambient apply the genotypes are formed under the estimated ambient share."""
import os
import subprocess

import numpy as np
import pytest

import donor_genotypes_reference as gr
from test_host_cli import host_bin, rust_display  # noqa: F401

pytestmark = pytest.mark.gpu

# planted pool 6 (600 loci x 966 cells: three donors, a decoy without cells, 60 doublets) under its damaged genotypes: a tenth of the
# calls blanked, a twentieth of the rest flipped.  Random genotypes would call no singlet, and the genotypes would have no reads.
L = 600
DONORS = ["alice", "bob", "carol", "decoy"]
GT_TEXT = {0: "0/0", 1: "0/1", 2: "1/1", 3: "./."}


def _variant_vcf(path):
    with open(path, "w") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        for i in range(L):
            f.write(f"chr{1 + i % 3}\t{100 + i}\t.\tA\tG\t.\t.\t.\n")


def _donor_vcf(path, cols, fmt):
    with open(path, "w") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(DONORS) + "\n")
        for i in range(L):
            f.write(f"chr{1 + i % 3}\t{100 + i}\t.\tA\tG\t.\t.\t.\t{fmt}\t" + "\t".join(cols(i, d) for d in range(len(DONORS))) + "\n")


def _run(host_bin, r, name, extra, dvcf=None):
    d = os.path.join(r["tmp"], name)
    cmd = [host_bin, "-a", r["alt"], "-r", r["ref"], "--output_directory", d, "--min_alt", "4", "--min_ref", "4", "--barcodes", r["bc"], "--vcf",
           r["vcf"], "--donors", dvcf or r["dvcf"]] + extra
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    return dict(dir=d, stdout=p.stdout, stderr=p.stderr)


@pytest.fixture(scope="module")
def runs(host_bin, tmp_path_factory):
    from cellector_amd import synth
    tmp = str(tmp_path_factory.mktemp("donor_genotypes"))
    P = gr.planted(6)
    assert P["L"] == L
    N, gt = P["N"], P["damaged"]
    alt, ref = synth.write_mtx_pair(tmp, L, N, *[np.asarray(x, np.uint32) for x in P["coo"]], header_nnz=0)
    bc = os.path.join(tmp, "barcodes.tsv")
    synth.write_barcodes(bc, N)
    vcf, dvcf = os.path.join(tmp, "variants.vcf"), os.path.join(tmp, "donors.vcf")
    _variant_vcf(vcf)
    _donor_vcf(dvcf, lambda i, d: GT_TEXT[int(gt[d, i])], "GT")
    r = dict(tmp=tmp, alt=alt, ref=ref, bc=bc, vcf=vcf, dvcf=dvcf, gt=gt, barcodes=open(bc).read().splitlines())
    r["plain"] = _run(host_bin, r, "plain", [])
    r["true"] = _run(host_bin, r, "true", ["--donor_genotypes", "true"])
    r["apply"] = _run(host_bin, r, "apply", ["--donor_genotypes", "apply"])
    cf = os.path.join(tmp, "classes.tsv")
    with open(cf, "w") as f:
        for c, k in enumerate(P["truth_cell"]):
            if k != 255:
                f.write(f"{r['barcodes'][c]}\tclass{k}\n")
    r["second_pass"] = ["--classes", cf, "--donor_fit", "true", "--doublet_fraction", "true"]
    r["apply_all"] = _run(host_bin, r, "apply_all", ["--donor_genotypes", "apply"] + r["second_pass"])
    r["amb"] = _run(host_bin, r, "amb", ["--estimate_ambient", "apply"])
    r["amb_true"] = _run(host_bin, r, "amb_true", ["--estimate_ambient", "apply", "--donor_genotypes", "true"])
    return r


NEW = ["cellector_donor_genotypes.tsv", "cellector_donor_genotypes.vcf"]


def _same_but_new(a, b):
    files = sorted(os.listdir(a["dir"]))
    assert sorted(os.listdir(b["dir"])) == sorted(files + NEW)
    for f in files:
        assert open(os.path.join(a["dir"], f), "rb").read() == open(os.path.join(b["dir"], f), "rb").read(), f
    lines = b["stdout"].splitlines(keepends=True)
    new = [ln for ln in lines if ln.startswith("donor_genotypes: ")]
    assert len(new) == 1 and "".join(ln for ln in lines if ln is not new[0]) == a["stdout"]
    return new[0]


def _binding(runs, ambient):
    from cellector_amd import Cellector, donor_genotypes as dg
    g = Cellector(0)
    g.load_mtx(runs["alt"], runs["ref"], 4, 4)
    prior = dg.prior_from_gt(runs["gt"])
    don = g.donor_posteriors_gp(prior, min_loci=30, posterior_threshold=0.999, ambient=ambient)
    assign = np.where(don["status"] == 0, don["best"], 255).astype(np.uint8)
    gen = g.donor_genotypes(assign, prior, ambient=ambient)
    again = g.donor_posteriors_gp(dg.to_gp(gen["q"]), min_loci=30, posterior_threshold=0.999, ambient=ambient)
    g.close()
    return don, gen, again


def _check_files(runs, run, gen, line):
    from cellector_amd import donor_genotypes as dg
    s = gen["summary"]
    assert open(os.path.join(run["dir"], NEW[0])).read() == dg.render_tsv(DONORS, s)
    tot = {k: int(s[k].sum()) for k in s}
    assert line == (f"donor_genotypes: donors=4 cells={tot['cells']} confirmed={tot['confirmed']} filled={tot['filled']} "
                    f"changed={tot['changed']} withdrawn={tot['withdrawn']}\n")
    assert tot["cells"] > 800 and tot["filled"] > 100 and tot["confirmed"] > 1000 and tot["changed"] > 50
    cols = dg.render_vcf_columns(gen["gt_out"], gen["q"], gen["alt"], gen["ref"], fmt=rust_display)
    rows = open(os.path.join(run["dir"], NEW[1])).read().splitlines()
    assert rows[0] == "##fileformat=VCFv4.2" and rows[1].split("\t")[-4:] == DONORS and len(rows) == L + 2
    src = open(runs["vcf"]).read().splitlines()
    for t in range(L):
        assert rows[2 + t] == src[2 + t] + "\tGT:GP:AO:RO\t" + "\t".join(cols[t]), t


def test_true_changes_no_other_output_and_matches_the_binding(runs):
    line = _same_but_new(runs["plain"], runs["true"])
    don, gen, _ = _binding(runs, 0.03)
    _check_files(runs, runs["true"], gen, line)


def test_apply_is_a_run_given_the_refined_genotypes_beforehand(host_bin, runs):
    don, gen, again = _binding(runs, 0.03)
    gp = np.asarray(gen["q"], np.float32)
    refined = os.path.join(runs["tmp"], "refined.vcf")
    # float32 values in their shortest decimal form read back exactly
    _donor_vcf(refined, lambda i, d: GT_TEXT[int(np.argmax(gp[d, i]))] + ":" + ",".join(repr(float(x)) for x in gp[d, i]), "GT:GP")
    given = _run(host_bin, runs, "given", ["--donor_field", "GP"], dvcf=refined)
    a, b = runs["apply"], given
    assert open(os.path.join(a["dir"], "cellector_donors.tsv"), "rb").read() == open(os.path.join(b["dir"], "cellector_donors.tsv"), "rb").read()
    assert open(os.path.join(a["dir"], "cellector_donors.tsv"), "rb").read() != open(os.path.join(runs["plain"]["dir"], "cellector_donors.tsv"), "rb").read()
    # the genotype files of apply are those of true: the refinement itself ran on the first pass
    for f in NEW:
        assert open(os.path.join(a["dir"], f), "rb").read() == open(os.path.join(runs["true"]["dir"], f), "rb").read(), f
    # ... and everything written behind the second pass: the class match, the fit and the doublet fractions
    given_all = _run(host_bin, runs, "given_all", ["--donor_field", "GP"] + runs["second_pass"], dvcf=refined)
    for f in ("cellector_donors.tsv", "cellector_cluster_donors.tsv", "cellector_donor_fit.tsv", "cellector_doublet_fractions.tsv"):
        x = open(os.path.join(runs["apply_all"]["dir"], f), "rb").read()
        assert len(x) > 100 and x == open(os.path.join(given_all["dir"], f), "rb").read(), f
    s = again["summary"]
    want = f"singlet={s.n_singlet} doublet={s.n_doublet} ambiguous={s.n_ambiguous} unassigned={s.n_unassigned}"
    passes = [ln for ln in a["stderr"].splitlines() if ln.startswith("donors: ")]
    assert len(passes) == 2 and want in passes[1]


def test_with_estimate_ambient_apply(runs):
    line = _same_but_new(runs["amb"], runs["amb_true"])
    rho = None
    for ln in open(os.path.join(runs["amb"]["dir"], "cellector_ambient.tsv")).read().splitlines():
        if ln.startswith("pool\t"):
            rho = float(ln.split("\t")[2])
    assert rho is not None and rho != 0.03
    don, gen, _ = _binding(runs, rho)
    _check_files(runs, runs["amb_true"], gen, line)
