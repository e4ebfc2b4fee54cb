"""GPU: `host/cellector --doublets <file> [--doublet_downsample_rate <r>]` — synthetic doublets of the run's own cells, added on the
device after --cells, --downsample_rate and --mix_* (cellector_add_doublets).  The run is byte for byte the run of the binary
WITHOUT the flags on files written beforehand from the numpy twins' arrays, with the expected barcodes.tsv and, as -g, the expected
gt.tsv; and the barcodes.tsv / gt.tsv the flagged run writes into its output directory are those files."""
import os
import subprocess

import numpy as np
import pytest

from test_host_cli import host_bin  # noqa: F401

L, N1, N2, NP = 400, 300, 120, 30


def _run(host_bin, alt, ref, bc, vcf, out, *extra):
    cmd = [host_bin, "-a", alt, "-r", ref, "--output_directory", out, "--min_alt", "4", "--min_ref", "4", "--barcodes", bc, "--vcf", vcf]
    return subprocess.run(cmd + list(extra), capture_output=True, text=True, timeout=600)


def _write(path, text):
    with open(path, "w") as f:
        f.write(text)
    return path


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    from cellector_amd import combine, doublets, restage, synth
    tmp = str(tmp_path_factory.mktemp("cli_doublets"))
    dst = synth.generate_coo(L, N1, 0.1, seed=11, minority_fraction=0.1)
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
    rng = np.random.default_rng(5)

    def expected(name, coo, n, names, labels, a, b, rate):
        """the files a user would have made by hand: the twin's arrays, the barcodes with <A>+<B> behind them, the labels"""
        assert len({(int(x), int(y)) for x, y in zip(a, b)}) == len(a)  # (the command line takes a pair once)
        t = doublets.add_doublets_coo(coo, n, a, b, rate, 4)
        d = os.path.join(tmp, name)
        alt, ref = synth.write_mtx_pair(d, L, t[4], *t[:4], header_nnz=0)
        every = names + [names[x] + "+" + names[y] for x, y in zip(a, b)]
        gt = labels + ["doublet"] * len(a)
        pairs = "".join(names[x] + "\t" + names[y] + ("\n\n" if j % 7 == 0 else "\n") for j, (x, y) in enumerate(zip(a, b)))
        return dict(alt=alt, ref=ref, n=t[4], labels=gt, bc=_write(os.path.join(d, "barcodes.tsv"), "".join(x + "\n" for x in every)),
                    gt=_write(os.path.join(d, "gt.tsv"), "".join(x + "\t" + y + "\n" for x, y in zip(every, gt))),
                    pairs=_write(os.path.join(d, "pairs.tsv"), pairs))

    # 1. --doublets alone, at rate 0.5: majority x minority parents of the first dataset
    cls = synth.cell_classes(N1, seed=11, minority_fraction=0.1)
    a, b = rng.choice(np.flatnonzero(cls == 0), NP), rng.choice(np.flatnonzero(cls == 1), NP)
    alone = expected("alone", dst, N1, names1, ["singlet"] * N1, a, b, 0.5)
    # ... the same with -g: the labels of the cells it names, na for the others, doublet for the new cells
    named = ["hashtag%d" % (i % 3) if i % 4 else "na" for i in range(N1)]
    with_g = expected("with_g", dst, N1, names1, named, a, b, 0.5)
    with_g["g"] = _write(os.path.join(tmp, "hash.tsv"), "".join(n + "\t" + x + "\n" for n, x in zip(names1, named) if x != "na"))
    # 2. with --cells, --downsample_rate, --mix_* and --mix_cells: the doublets come last and pair first x second cells
    keep1 = rng.random(N1) < 0.8
    keep2 = rng.random(N2) < 0.5
    cells = _write(os.path.join(tmp, "cells.tsv"), "".join(names1[i] + "\n" for i in rng.permutation(np.flatnonzero(keep1))))
    mix_cells = _write(os.path.join(tmp, "mix_cells.tsv"), "".join(names2[i] + "\n" for i in rng.permutation(np.flatnonzero(keep2))))
    own = restage.restage_coo(*dst, N1, keep1, 0.2, 4)
    mixed = combine.combine_coo(own[:4], own[4], src, N2, keep2, None, L, 0.2, 4)
    n1, n2 = int(keep1.sum()), int(keep2.sum())
    names = [n for n, k in zip(names1, keep1) if k] + [n[:-1] + "2" for n, k in zip(names2, keep2) if k]
    assert mixed[4] == n1 + n2 == len(names)
    a, b = rng.integers(0, n1, NP), n1 + rng.integers(0, n2, NP)
    a[1], b[1] = b[1], a[1]  # (either order)
    assert len({(x, y) for x, y in zip(a, b)}) == NP
    both = expected("mixed", mixed[:4], mixed[4], names, ["majority"] * n1 + ["minority"] * n2, a, b, 0.25)
    # a dataset whose doublet would hold more than 65535 reads of one allele at one locus
    big = [x.copy() for x in dst]
    big[2][0] = big[2][1] = 40000
    d4 = os.path.join(tmp, "big")
    alt4, ref4 = synth.write_mtx_pair(d4, L, N1, *big, header_nnz=0)
    return dict(first=(alt1, ref1, bc1), second=(alt2, ref2, bc2), big=(alt4, ref4, names1[int(dst[1][0])], names1[int(dst[1][1])], int(dst[0][0])),
                vcf=vcf, names1=names1, alone=alone, with_g=with_g, both=both, cells=cells, mix_cells=mix_cells)


def _check(host_bin, inputs, tmp_path, which, *extra):
    m = inputs[which]
    alt1, ref1, bc1 = inputs["first"]
    o0, o1 = str(tmp_path / "files"), str(tmp_path / "flags")
    r0 = _run(host_bin, m["alt"], m["ref"], m["bc"], inputs["vcf"], o0, "-g", m["gt"])
    r1 = _run(host_bin, alt1, ref1, bc1, inputs["vcf"], o1, "--doublets", m["pairs"], *extra)
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
    assert [r.split("\t")[-1] for r in rows[1:]] == m["labels"]  # the run's ground truth
    assert rows[-1].split("\t")[0].count("+") == 1


@pytest.mark.gpu
def test_doublets_equal_a_run_on_files_with_the_doublets_in_them(host_bin, inputs, tmp_path):
    assert inputs["alone"]["n"] == N1 + NP
    _check(host_bin, inputs, tmp_path, "alone", "--doublet_downsample_rate", "0.5")


@pytest.mark.gpu
def test_doublets_keep_the_labels_of_a_ground_truth(host_bin, inputs, tmp_path):
    _check(host_bin, inputs, tmp_path, "with_g", "--doublet_downsample_rate", "0.5", "-g", inputs["with_g"]["g"])


@pytest.mark.gpu
def test_doublets_after_cells_downsampling_and_a_mixture(host_bin, inputs, tmp_path):
    alt2, ref2, bc2 = inputs["second"]
    _check(host_bin, inputs, tmp_path, "both", "--doublet_downsample_rate", "0.25", "--cells", inputs["cells"], "--downsample_rate", "0.2",
           "--mix_alt", alt2, "--mix_ref", ref2, "--mix_barcodes", bc2, "--mix_cells", inputs["mix_cells"])


@pytest.mark.gpu
def test_errors(host_bin, inputs, tmp_path):
    alt1, ref1, bc1 = inputs["first"]
    names = inputs["names1"]
    out = str(tmp_path / "o")

    def refused(text, *extra, inp=(alt1, ref1, bc1)):
        r = _run(host_bin, *inp, inputs["vcf"], out, "--doublets", _write(str(tmp_path / "pairs.tsv"), text), *extra)
        assert r.returncode == 1 and "--doublets" in r.stderr, (r.returncode, r.stderr)
        return r.stderr

    ok = names[3] + "\t" + names[9] + "\n"
    err = refused(ok + "\n" + names[4] + "\tNOT_A_BARCODE-1\n")
    assert "NOT_A_BARCODE-1" in err and "line 3" in err
    assert "line 2" in refused(ok + names[4] + "\n")  # one column
    assert "line 2" in refused(ok + names[4] + "\t" + names[5] + "\t" + names[6] + "\n")  # three
    err = refused(ok + names[7] + "\t" + names[7] + "\n")
    assert "line 2" in err and names[7] in err
    err = refused(ok + names[5] + "\t" + names[6] + "\n" + ok)
    assert "line 3" in err and "twice" in err
    assert "no pair" in refused("\n\n")
    # a barcode that --cells dropped is not one of the run's cells
    only = _write(str(tmp_path / "cells.tsv"), "".join(n + "\n" for n in names[:8]))
    assert names[9] in refused(ok, "--cells", only)
    # one GPU
    err = refused(ok, "--devices", "0,0")
    assert "--devices" in err
    r = _run(host_bin, alt1, ref1, bc1, inputs["vcf"], out, "--doublet_downsample_rate", "0.5")
    assert r.returncode == 1 and "--doublets" in r.stderr
    r = _run(host_bin, alt1, ref1, bc1, inputs["vcf"], out, "--doublets", _write(str(tmp_path / "pairs.tsv"), ok), "--doublet_downsample_rate", "1.5")
    assert r.returncode == 1 and "--doublet_downsample_rate" in r.stderr and "[0, 1]" in r.stderr
    # a summed count above 65535: pair, locus and allele
    alt4, ref4, na, nb, locus = inputs["big"]
    err = refused(ok + nb + "\t" + na + "\n", inp=(alt4, ref4, bc1))
    assert "pair 1 " in err and f"locus {locus}" in err and " alt " in err and "65535" in err
    # an input of the run that lies in the output directory as barcodes.tsv would be overwritten: refused, file intact
    mine = tmp_path / "mine"
    mine.mkdir()
    text = open(bc1).read()
    (mine / "barcodes.tsv").write_text(text)
    r = _run(host_bin, alt1, ref1, str(mine / "barcodes.tsv"), inputs["vcf"], str(mine), "--doublets", _write(str(tmp_path / "p.tsv"), ok))
    assert r.returncode == 1 and "overwrite" in r.stderr and "barcodes.tsv" in r.stderr, r.stderr
    assert open(mine / "barcodes.tsv").read() == text


def test_help_lists_the_flags(host_bin):
    r = subprocess.run([host_bin, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--doublets <file>", "--doublet_downsample_rate <r>"):
        assert flag in r.stdout, flag
