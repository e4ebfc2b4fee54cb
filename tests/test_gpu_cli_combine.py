"""GPU: `host/cellector --mix_alt <alt2> --mix_ref <ref2> --mix_barcodes <barcodes2> [--mix_cells <file>]` — the second dataset is
merged in on the device after the load (cellector_combine, identity locus map).  The run is byte for byte the run of the binary
WITHOUT the flags on files written beforehand from the numpy twin's arrays, with the mixture's barcodes.tsv and, as -g, its gt.tsv;
and the barcodes.tsv / gt.tsv the flagged run writes into its output directory are those files.

The case is tests/test_gpu_combine.py's with src regenerated on ctx's 1500 loci: 800 + 300 cells, or 800 + the 66 of
default_rng(3).random(300) < 0.25 at rate 0.2."""
import os
import subprocess

import numpy as np
import pytest

from test_host_cli import host_bin  # noqa: F401

L, N1, N2 = 1500, 800, 300


def _run(host_bin, alt, ref, bc, vcf, out, *extra):
    cmd = [host_bin, "-a", alt, "-r", ref, "--output_directory", out, "--min_alt", "4", "--min_ref", "4", "--barcodes", bc, "--vcf", vcf]
    return subprocess.run(cmd + list(extra), capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    from cellector_amd import combine, restage, synth
    tmp = str(tmp_path_factory.mktemp("cli_combine"))
    dst = synth.generate_coo(L, N1, 0.1, seed=11, minority_fraction=0)
    src = synth.generate_coo(L, N2, 0.1, seed=12, minority_fraction=0)
    d1, d2 = os.path.join(tmp, "first"), os.path.join(tmp, "second")
    alt1, ref1 = synth.write_mtx_pair(d1, L, N1, *dst, header_nnz=0)
    alt2, ref2 = synth.write_mtx_pair(d2, L, N2, *src, header_nnz=0)
    bc1, bc2 = os.path.join(d1, "barcodes.tsv"), os.path.join(d2, "barcodes.tsv")
    synth.write_barcodes(bc1, N1)
    synth.write_barcodes(bc2, N2)
    names1, names2 = open(bc1).read().split(), open(bc2).read().split()
    vcf = os.path.join(tmp, "variants.vcf")
    with open(vcf, "w") as f:
        f.write("##fileformat=VCFv4.2\n##source=synthetic\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        for l in range(L):
            f.write(f"chr{1 + l % 22}\t{1000 + 37 * l}\t.\tA\tG\t50\tPASS\t.\n")
    keep = np.random.default_rng(3).random(N2) < 0.25
    lst = os.path.join(tmp, "mix_cells.tsv")
    with open(lst, "w") as f:  # any order, more columns, a blank line: the SET counts
        for j, i in enumerate(np.random.default_rng(8).permutation(np.flatnonzero(keep))):
            f.write(names2[i] + ("\tx\n\n" if j % 5 == 0 else "\n"))
    # a third dataset on other loci
    d3 = os.path.join(tmp, "third")
    alt3, ref3 = synth.write_mtx_pair(d3, L - 100, N2, *synth.generate_coo(L - 100, N2, 0.1, seed=12, minority_fraction=0), header_nnz=0)

    def mixture(name, kp, rate):
        """the files a user would have made with the combiner: the twin's arrays, its barcodes.tsv and gt.tsv"""
        own = restage.restage_coo(*dst, N1, None, rate, 4)  # --downsample_rate thins the first dataset as a restage does
        t = combine.combine_coo(own[:4], N1, src, N2, kp, None, L, rate, 4)
        d = os.path.join(tmp, name)
        alt, ref = synth.write_mtx_pair(d, L, t[4], *t[:4], header_nnz=0)
        taken = names2 if kp is None else [n for n, k in zip(names2, kp) if k]
        mixed = names1 + [n[:-1] + "2" for n in taken]
        assert len(mixed) == t[4]
        bc, gt = os.path.join(d, "barcodes.tsv"), os.path.join(d, "gt.tsv")
        open(bc, "w").write("".join(n + "\n" for n in mixed))
        open(gt, "w").write("".join(n + ("\tmajority\n" if i < N1 else "\tminority\n") for i, n in enumerate(mixed)))
        return dict(alt=alt, ref=ref, bc=bc, gt=gt, n=t[4])

    return dict(first=(alt1, ref1, bc1), second=(alt2, ref2, bc2), third=(alt3, ref3), vcf=vcf, lst=lst,
                all=mixture("mix_all", None, 0.0), some=mixture("mix_some", keep, 0.2))


def _check(host_bin, inputs, tmp_path, which, *extra):
    m = inputs[which]
    alt1, ref1, bc1 = inputs["first"]
    alt2, ref2, bc2 = inputs["second"]
    o0, o1 = str(tmp_path / "files"), str(tmp_path / "flags")
    r0 = _run(host_bin, m["alt"], m["ref"], m["bc"], inputs["vcf"], o0, "-g", m["gt"])
    r1 = _run(host_bin, alt1, ref1, bc1, inputs["vcf"], o1, "--mix_alt", alt2, "--mix_ref", ref2, "--mix_barcodes", bc2, *extra)
    assert r0.returncode == 0, r0.stderr
    assert r1.returncode == 0, r1.stderr
    assert r0.stdout == r1.stdout
    files = sorted(os.listdir(o0))
    assert sorted(os.listdir(o1)) == sorted(files + ["barcodes.tsv", "gt.tsv"]) and "cellector_assignments.tsv" in files and "cellector.vcf" in files
    for f in files:
        assert open(os.path.join(o0, f), "rb").read() == open(os.path.join(o1, f), "rb").read(), f
    for f in ("bc", "gt"):
        assert open(m[f], "rb").read() == open(os.path.join(o1, os.path.basename(m[f])), "rb").read(), f
    rows = open(os.path.join(o1, "cellector_assignments.tsv")).read().splitlines()
    assert len(rows) == 1 + m["n"]
    assert [r.split("\t")[-1] for r in rows[1:]] == ["majority"] * N1 + ["minority"] * (m["n"] - N1)  # the run's ground truth
    return rows


@pytest.mark.gpu
def test_mix_equals_a_run_on_combined_files(host_bin, inputs, tmp_path):
    assert inputs["all"]["n"] == N1 + N2
    _check(host_bin, inputs, tmp_path, "all")


@pytest.mark.gpu
def test_mix_cells_and_downsample_equal_a_run_on_combined_files(host_bin, inputs, tmp_path):
    assert inputs["some"]["n"] == N1 + 66
    rows = _check(host_bin, inputs, tmp_path, "some", "--mix_cells", inputs["lst"], "--downsample_rate", "0.2")
    # the titration's answer: exactly the cells mixed in are excluded and labelled 0, the others 1
    assert [r.split("\t")[1:3] for r in rows[1:]] == [["1", "1"]] * N1 + [["0", "0"]] * 66


@pytest.mark.gpu
def test_errors(host_bin, inputs, tmp_path):
    alt1, ref1, bc1 = inputs["first"]
    alt2, ref2, bc2 = inputs["second"]
    triple = {"--mix_alt": alt2, "--mix_ref": ref2, "--mix_barcodes": bc2}
    out = str(tmp_path / "o")
    for missing in triple:
        args = [x for k, v in triple.items() if k != missing for x in (k, v)]
        r = _run(host_bin, alt1, ref1, bc1, inputs["vcf"], out, *args)
        assert r.returncode == 1 and missing in r.stderr, r.stderr
    r = _run(host_bin, alt1, ref1, bc1, inputs["vcf"], out, "--mix_cells", inputs["lst"])
    assert r.returncode == 1 and "--mix_alt" in r.stderr
    all3 = [x for kv in triple.items() for x in kv]
    r = _run(host_bin, alt1, ref1, bc1, inputs["vcf"], out, *all3, "--devices", "0,0")
    assert r.returncode == 1 and "--mix_alt" in r.stderr and "--devices" in r.stderr
    other = dict(triple, **{"--mix_alt": inputs["third"][0], "--mix_ref": inputs["third"][1]})
    r = _run(host_bin, alt1, ref1, bc1, inputs["vcf"], out, *[x for kv in other.items() for x in kv])
    assert r.returncode == 1 and "1400 loci" in r.stderr and "1500 loci" in r.stderr, r.stderr
    # an input of the run that lies in the output directory as barcodes.tsv / gt.tsv would be overwritten: refused, file intact
    mine = tmp_path / "mine"
    mine.mkdir()
    for name in ("barcodes.tsv", "gt.tsv"):
        text = open(bc1).read() if name == "barcodes.tsv" else "".join(n + "\tsinglet\n" for n in open(bc1).read().split())
        (mine / name).write_text(text)
        args = [host_bin, "-a", alt1, "-r", ref1, "--output_directory", str(mine), "--vcf", inputs["vcf"], *all3]
        args += ["--barcodes", str(mine / name) if name == "barcodes.tsv" else bc1] + ([] if name == "barcodes.tsv" else ["-g", str(mine / name)])
        r = subprocess.run(args, capture_output=True, text=True, timeout=600)
        assert r.returncode == 1 and "overwrite" in r.stderr and name in r.stderr, r.stderr
        assert open(mine / name).read() == text
        os.remove(mine / name)
    bad = tmp_path / "bad.tsv"
    bad.write_text(open(bc2).read().split()[3] + "\nNOT_A_BARCODE-1\n")
    r = _run(host_bin, alt1, ref1, bc1, inputs["vcf"], out, *all3, "--mix_cells", str(bad))
    assert r.returncode == 1 and "NOT_A_BARCODE-1" in r.stderr and "line 2" in r.stderr and "--mix_cells" in r.stderr


def test_help_lists_the_flags(host_bin):
    r = subprocess.run([host_bin, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--mix_alt <alt2>", "--mix_ref <ref2>", "--mix_barcodes <barcodes2>", "--mix_cells <file>"):
        assert flag in r.stdout, flag
