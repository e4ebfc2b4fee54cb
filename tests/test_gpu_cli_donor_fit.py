"""GPU: `host/cellector --vcf <vcf> --donors <vcf> --donor_fit true` — cellector_donor_fit.tsv holds the Python binding's donor fit of
the same genotypes rendered the same way (the binding is held to the twin and the reference in test_gpu_donor_fit.py); with one donor's
column taken out of the VCF the planted cells of that donor carry unmatched 1; every other output file is the run's without the flag,
byte for byte, and stdout gains one line; --donor_fit without --donors is a usage error.

The fixture is built the way tests/test_gpu_cli_donors.py builds its own (text matrices, barcodes, a variant VCF and a donor VCF with
records left out and swapped), around donor_reference.planted_pool so that there are planted cells to withhold.
"""
import os
import subprocess

import numpy as np
import pytest

import class_reference as cr
import donor_reference as dr
from test_gpu_cli_donors import GT_TEXT
from test_host_cli import host_bin, rust_display  # noqa: F401

pytestmark = pytest.mark.gpu

NAMES = ["alice", "bob", "carol", "decoy"]
STATUS = {0: "singlet", 1: "doublet", 2: "ambiguous", 255: "unassigned"}
HEAD = ["barcode", "status", "donor", "second_donor", "n_loci", "ll", "expected", "variance", "z", "unmatched"]


def _variant_vcf(path, L):
    with open(path, "w") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        for i in range(L):
            f.write(f"chr{1 + i % 3}\t{100 + i}\t.\tA\tG\t.\t.\t.\n")


def _donor_vcf(path, gt, names):
    """every record whose calls are all blank is left out, every seventh has ref and alt swapped (its calls written mirrored)"""
    with open(path, "w") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names) + "\n")
        for i in range(gt.shape[1]):
            if (gt[:, i] == 3).all():
                continue
            swap = i % 7 == 3
            calls = [GT_TEXT[int(g) if g == 3 or not swap else 2 - int(g)] for g in gt[:, i]]
            f.write(f"chr{1 + i % 3}\t{100 + i}\t.\t{'G' if swap else 'A'}\t{'A' if swap else 'G'}\t.\t.\t.\tGT\t" + "\t".join(calls) + "\n")


@pytest.fixture(scope="module")
def runs(host_bin, tmp_path_factory):
    from cellector_amd import synth
    tmp = str(tmp_path_factory.mktemp("donor_fit"))
    L, N, coo, gt, truth, par = dr.planted_pool(5)
    alt, ref = synth.write_mtx_pair(tmp, L, N, *[np.asarray(x, np.uint32) for x in coo], header_nnz=0)
    bc = os.path.join(tmp, "barcodes.tsv")
    synth.write_barcodes(bc, N)
    vcf, dvcf, less = (os.path.join(tmp, n) for n in ("variants.vcf", "donors.vcf", "donors_without_bob.vcf"))
    _variant_vcf(vcf, L)
    _donor_vcf(dvcf, gt, NAMES)
    _donor_vcf(less, gt[[0, 2, 3]], [NAMES[d] for d in (0, 2, 3)])
    out = {}
    for name, extra in (("donors", ["--donors", dvcf]), ("fit", ["--donors", dvcf, "--donor_fit", "true"]),
                        ("fit_less", ["--donors", less, "--donor_fit", "true", "--donor_fit_iqr", "3.5"])):
        d = os.path.join(tmp, name)
        cmd = [host_bin, "-a", alt, "-r", ref, "--output_directory", d, "--min_alt", "4", "--min_ref", "4", "--barcodes", bc, "--vcf", vcf] + extra
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        out[name] = dict(dir=d, stdout=r.stdout, stderr=r.stderr)
    return dict(alt=alt, ref=ref, bc=bc, barcodes=open(bc).read().splitlines(), gt=gt, truth=truth, N=N, vcf=vcf, dvcf=dvcf, **out)


def test_every_other_output_is_the_run_without_the_flag(runs):
    a, b = runs["donors"], runs["fit"]
    files = sorted(os.listdir(a["dir"]))
    assert "cellector_donors.tsv" in files and not any("donor_fit" in f for f in files)
    assert sorted(os.listdir(b["dir"])) == sorted(files + ["cellector_donor_fit.tsv"])
    for f in files:
        assert open(os.path.join(a["dir"], f), "rb").read() == open(os.path.join(b["dir"], f), "rb").read(), f
    extra = [ln for ln in b["stdout"].splitlines() if ln.startswith("donor_fit: ")]
    assert len(extra) == 1 and "donor_fit" not in a["stdout"]
    assert [ln for ln in b["stdout"].splitlines() if not ln.startswith("donor_fit: ")] == a["stdout"].splitlines()


def test_the_table_is_the_binding(runs):
    from cellector_amd import Cellector
    g = Cellector(0)
    g.load_mtx(runs["alt"], runs["ref"], 4, 4)
    N = runs["N"]
    for name, rows_of, names, fit in (("fit", [0, 1, 2, 3], NAMES, {}), ("fit_less", [0, 2, 3], [NAMES[d] for d in (0, 2, 3)], dict(iqr_multiple=3.5))):
        gt = runs["gt"][rows_of]
        r = g.donor_fit(gt, min_loci=30, posterior_threshold=0.999, **fit)
        call = g.donor_posteriors(gt, min_loci=30, posterior_threshold=0.999)
        rows = [ln.split("\t") for ln in open(os.path.join(runs[name]["dir"], "cellector_donor_fit.tsv")).read().splitlines()]
        assert rows[0] == HEAD and len(rows) == N + 1
        for c in range(N):
            st, a, b = int(r["status"][c]), int(r["hyp_a"][c]), int(r["hyp_b"][c])
            if st == 255:
                want = [runs["barcodes"][c], "unassigned", "NA", "NA", str(int(call["n_entries"][c]))] + ["NA"] * 5
            else:
                ll, e, v = (call["pair_ll"], r["pair_e"], r["pair_v"]) if b != 255 else (call["ll"], r["fit_e"], r["fit_v"])
                d = b if b != 255 else a
                want = [runs["barcodes"][c], STATUS[st], names[a], names[b] if b != 255 else "NA", str(int(call["n_entries"][c])),
                        rust_display(float(ll[c, d])), rust_display(float(e[c, d])), rust_display(float(v[c, d])),
                        rust_display(float(r["call_z"][c])), str(int(r["unmatched"][c]))]
            assert rows[1 + c] == want, (name, c)
        s = r["summary"]
        line = (f"donor_fit: keys={s.n_keys} median={rust_display(s.median)} iqr={rust_display(s.iqr)} "
                f"threshold={rust_display(s.threshold)} unmatched={s.n_unmatched}")
        assert line in runs[name]["stdout"].splitlines(), (line, runs[name]["stdout"])
    g.close()


def test_the_cells_of_a_donor_the_vcf_does_not_hold_are_unmatched(runs):
    truth = runs["truth"]
    single = np.arange(cr.MIX_N)
    flags = {}
    for name in ("fit", "fit_less"):
        rows = [ln.split("\t") for ln in open(os.path.join(runs[name]["dir"], "cellector_donor_fit.tsv")).read().splitlines()[1:]]
        flags[name] = np.array([r[9] == "1" for r in rows])
        assert all(r[9] in ("0", "1", "NA") for r in rows)
    bob = single[truth[single] == 1]
    assert flags["fit_less"][bob].all()
    assert not flags["fit_less"][np.setdiff1d(single, bob)].any() and not flags["fit"][single].any()


def test_usage_errors_and_help(host_bin, runs, tmp_path):
    base = [host_bin, "-a", runs["alt"], "-r", runs["ref"], "--output_directory", str(tmp_path / "o"), "--barcodes", runs["bc"], "--vcf", runs["vcf"]]
    r = subprocess.run(base + ["--donor_fit", "true"], capture_output=True, text=True)
    assert r.returncode == 1 and "'--donor_fit true' requires '--donors <vcf>'" in r.stderr and not os.path.exists(tmp_path / "o")
    r = subprocess.run(base + ["--donors", runs["dvcf"], "--donor_fit_iqr", "2"], capture_output=True, text=True)
    assert r.returncode == 1 and "requires '--donor_fit true'" in r.stderr
    r = subprocess.run(base + ["--donors", runs["dvcf"], "--donor_fit", "true", "--donor_fit_iqr", "-1"], capture_output=True, text=True)
    assert r.returncode == 1 and "Invalid value" in r.stderr
    r = subprocess.run([host_bin, "--help"], capture_output=True, text=True)
    for flag in ("--donor_fit <true>", "--donor_fit_iqr <k>"):
        assert flag in r.stdout, flag
