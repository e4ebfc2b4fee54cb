"""GPU: `host/cellector --vcf <vcf> --donors <vcf> --doublet_fraction true` on a small planted pool written to files, with and without
`--estimate_ambient apply`: cellector_doublet_fractions.tsv is the twin's rendering (pair_fraction.render of the twin fed the device's
tables, and of the binding's own outputs) byte for byte; every other output file is the run's without the flag, byte for byte, and
stdout gains one line; --doublet_fraction without --donors is a usage error.

The pool is pair_fraction_reference.planted(0): 300 singlets of three donors and 300 cells at each planted share 1, 0.5, 0.3, 0.15; the
donor pass calls most of the cells planted below 1 doublets, and only those take part.
"""
import os
import subprocess

import numpy as np
import pytest

import pair_fraction_reference as pf
from test_gpu_cli_donor_fit import _donor_vcf, _variant_vcf
from test_host_cli import host_bin, rust_display  # noqa: F401

pytestmark = pytest.mark.gpu

NAMES = ["alice", "bob", "carol"]
RUNS = (("donors", []), ("frac", ["--doublet_fraction", "true"]), ("apply", ["--estimate_ambient", "apply"]),
        ("apply_frac", ["--estimate_ambient", "apply", "--doublet_fraction", "true", "--doublet_min_fraction", "0.25"]))


@pytest.fixture(scope="module")
def runs(host_bin, tmp_path_factory):
    from cellector_amd import synth
    tmp = str(tmp_path_factory.mktemp("doublet_fraction"))
    L, N, coo, gt, a, b, f = pf.planted(0)
    alt, ref = synth.write_mtx_pair(tmp, L, N, *[np.asarray(x, np.uint32) for x in coo], header_nnz=0)
    bc = os.path.join(tmp, "barcodes.tsv")
    synth.write_barcodes(bc, N)
    vcf, dvcf = os.path.join(tmp, "variants.vcf"), os.path.join(tmp, "donors.vcf")
    _variant_vcf(vcf, L)
    _donor_vcf(dvcf, gt, NAMES)
    out = {}
    for name, extra in RUNS:
        d = os.path.join(tmp, name)
        cmd = [host_bin, "-a", alt, "-r", ref, "--output_directory", d, "--min_alt", "4", "--min_ref", "4", "--barcodes", bc, "--vcf", vcf,
               "--donors", dvcf] + extra
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        out[name] = dict(dir=d, stdout=r.stdout, stderr=r.stderr)
    return dict(alt=alt, ref=ref, bc=bc, barcodes=open(bc).read().splitlines(), coo=coo, gt=gt, f=f, L=L, N=N, vcf=vcf, dvcf=dvcf, **out)


@pytest.mark.parametrize("without, with_", [("donors", "frac"), ("apply", "apply_frac")])
def test_every_other_output_is_the_run_without_the_flag(runs, without, with_):
    a, b = runs[without], runs[with_]
    files = sorted(os.listdir(a["dir"]))
    assert "cellector_donors.tsv" in files and not any("doublet_fraction" in f for f in files)
    assert sorted(os.listdir(b["dir"])) == sorted(files + ["cellector_doublet_fractions.tsv"])
    for f in files:
        assert open(os.path.join(a["dir"], f), "rb").read() == open(os.path.join(b["dir"], f), "rb").read(), f
    extra = [ln for ln in b["stdout"].splitlines() if ln.startswith("doublet_fraction: ")]
    assert len(extra) == 1 and "doublet_fraction" not in a["stdout"]
    assert [ln for ln in b["stdout"].splitlines() if not ln.startswith("doublet_fraction: ")] == a["stdout"].splitlines()


def test_the_table_is_the_twins_rendering(runs):
    from cellector_amd import Cellector, cluster, pair_fraction
    g = Cellector(0)
    g.load_mtx(runs["alt"], runs["ref"], 4, 4)
    N, gt = runs["N"], runs["gt"]
    ids = g.locus_ids().astype(np.int64)
    at = np.full(runs["L"], -1, np.int64)
    at[ids] = np.arange(len(ids))
    lo, ce, al, re = (np.asarray(x, np.int64) for x in runs["coo"])
    keep = at[lo] >= 0
    mat = cluster.Matrix(len(ids), N, [at[lo[keep]], ce[keep], al[keep], re[keep]])
    dprm = dict(min_loci=30, posterior_threshold=0.999)
    for name, min_fraction in (("frac", 0.1), ("apply_frac", 0.25)):
        if name == "apply_frac":
            first = g.donor_posteriors(gt, **dprm)
            rho = g.estimate_ambient(gt, np.where(first["status"] == 0, first["best"], 255).astype(np.uint8))["rho"]
            dprm = dict(dprm, ambient=rho)
        call = g.donor_posteriors(gt, **dprm)
        dbl = call["status"] == 1
        pa, pb = np.where(dbl, call["best"], 255).astype(np.uint8), np.where(dbl, call["best_pair"], 255).astype(np.uint8)
        assert np.array_equal(call["anchor"], call["best"]) and dbl.sum() > 300
        prm = dict(min_fraction=min_fraction, min_loci=30)
        got = g.donor_pair_fractions(gt, pa, pb, None, prm, dprm, tables=True)
        tw = pair_fraction.pair_fractions(mat, gt[:, ids].T, pa, pb, None, tab=got["tab"], params=prm)
        text = open(os.path.join(runs[name]["dir"], "cellector_doublet_fractions.tsv")).read()
        assert text == pair_fraction.render(runs["barcodes"], NAMES, tw, pa, pb), name
        assert text == pair_fraction.render(runs["barcodes"], NAMES, got, pa, pb), name
        rows = [ln.split("\t") for ln in text.splitlines()]
        assert rows[0] == ["barcode", "donor_a", "donor_b", "n_loci", "fraction", "se", "ll_half", "ll_max", "kind"] and len(rows) == N + 1
        assert all(r[1:] == ["NA"] * 8 for r, d in zip(rows[1:], dbl) if not d)
        c = int(np.flatnonzero(dbl)[0])
        assert rows[1 + c][4] == rust_display(float(got["cell_frac"][c])) and rows[1 + c][6] == rust_display(float(got["ll"][c, 8]))
        assert {r[8] for r in rows[1:]} <= {"balanced", "toward_a", "toward_b", "flat", "NA"}
        s = got["summary"]
        line = f"doublet_fraction: balanced={s.n_balanced} toward_a={s.n_toward_a} toward_b={s.n_toward_b} flat={s.n_flat} none={s.n_none}"
        assert line in runs[name]["stdout"].splitlines(), (line, runs[name]["stdout"])
        # the planted shares come back: the called doublets planted at 0.5 are balanced, whichever of the two the pass anchored
        f = runs["f"]
        half = dbl & (f == 0.5)
        assert half.sum() > 250 and (got["kind"][half] == 0).all()
        print(name, "doublets", int(dbl.sum()), "of them planted at 0.5:", int(half.sum()), line)
    g.close()


def test_usage_errors(host_bin, runs, tmp_path):
    base = [host_bin, "-a", runs["alt"], "-r", runs["ref"], "--output_directory", str(tmp_path / "o"), "--barcodes", runs["bc"], "--vcf", runs["vcf"]]
    r = subprocess.run(base + ["--doublet_fraction", "true"], capture_output=True, text=True)
    assert r.returncode == 1 and "'--doublet_fraction true' requires '--donors <vcf>'" in r.stderr and not os.path.exists(tmp_path / "o")
    r = subprocess.run(base + ["--donors", runs["dvcf"], "--doublet_min_fraction", "0.2"], capture_output=True, text=True)
    assert r.returncode == 1 and "requires '--doublet_fraction true'" in r.stderr
    r = subprocess.run(base + ["--donors", runs["dvcf"], "--doublet_fraction", "true", "--doublet_min_fraction", "0.6"], capture_output=True, text=True)
    assert r.returncode == 1 and "Invalid value" in r.stderr and not os.path.exists(tmp_path / "o")
