"""GPU: `host/cellector --write_matrices <aligned|sparse|depth>` writes the matrix the run works on — after --mix_*, --mix_cells and
--downsample_rate here — into the output directory as text formatted on the device.  The files are the numpy twin's rendering
(cellector_amd/mtx_write.py) of combine.combine_coo's arrays; a run of the binary WITHOUT flags on the written files is the same run
byte for byte, the sparse and depth pairs through --matrix_pair join / depth; without the flag nothing new appears.

The sparse and depth pairs lack the entries with alt = ref = 0, and such an entry is a locus of its cell to the loop's normalisation
(the reference divides by the entries of the cell, main.rs:316): a pair without them is another matrix.  So the byte-for-byte feed-back
of those two words is held on the mixture WITHOUT --downsample_rate, which has no such entry, and on the thinned mixture against a run
on the aligned files of the matrix without them.

The case is tests/test_gpu_cli_combine.py's: 800 + the 66 listed cells of 300 at rate 0.2 on 1500 loci."""
import os
import subprocess

import numpy as np
import pytest

from cellector_amd import combine, mtx_write, restage, synth
from test_gpu_cli_combine import L, N1, N2, _run, inputs  # noqa: F401
from test_host_cli import host_bin  # noqa: F401

NAMES = {"aligned": ("alt.mtx", "ref.mtx"), "sparse": ("alt.mtx", "ref.mtx"), "depth": ("ad.mtx", "dp.mtx")}
PAIR = {"aligned": [], "sparse": ["--matrix_pair", "join"], "depth": ["--matrix_pair", "depth"]}


def _mix_args(inputs, thinned=True):  # noqa: F811
    alt2, ref2, bc2 = inputs["second"]
    return ["--mix_alt", alt2, "--mix_ref", ref2, "--mix_barcodes", bc2, "--mix_cells", inputs["lst"]] + (["--downsample_rate", "0.2"] if thinned else [])


@pytest.fixture(scope="module")
def mixture():
    """the twin's arrays of the mixture the flags make (the `some` case of test_gpu_cli_combine.py)"""
    dst = synth.generate_coo(L, N1, 0.1, seed=11, minority_fraction=0)
    src = synth.generate_coo(L, N2, 0.1, seed=12, minority_fraction=0)
    keep = np.random.default_rng(3).random(N2) < 0.25
    own = restage.restage_coo(*dst, N1, None, 0.2, 4)
    t = combine.combine_coo(own[:4], N1, src, N2, keep, None, L, 0.2, 4)
    return t[:4], t[4]


@pytest.fixture(scope="module")
def written(host_bin, inputs, tmp_path_factory):  # noqa: F811
    """one flagged run per word, and the run without the flag"""
    alt1, ref1, bc1 = inputs["first"]
    out = {}
    for word in (None, "aligned", "sparse", "depth", "sparse whole", "depth whole"):  # whole: the mixture without --downsample_rate
        o = str(tmp_path_factory.mktemp("write_" + str(word).replace(" ", "_")))
        r = _run(host_bin, alt1, ref1, bc1, inputs["vcf"], o, *_mix_args(inputs, thinned=not str(word).endswith("whole")),
                 *(["--write_matrices", word.split()[0]] if word else []))
        assert r.returncode == 0, r.stderr
        out[word] = (o, r)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("word", ["aligned", "sparse", "depth"])
def test_the_files_are_the_twins_rendering(written, mixture, word):
    coo, n_cells = mixture
    assert n_cells == N1 + 66 and ((coo[2] == 0) & (coo[3] == 0)).any()  # (the thinned mixture has 0 / 0 entries)
    o, r = written[word]
    for k, name in enumerate(NAMES[word]):
        want = mtx_write.file_bytes(L, n_cells, *coo, k, word, "\t", header_zero=True)  # tabs and the combiner's zero count
        assert open(os.path.join(o, name), "rb").read() == want, name
    # without the flag the directory is what it was; with it, the two names more and one stderr line, the same stdout
    o0, r0 = written[None]
    assert sorted(os.listdir(o)) == sorted(os.listdir(o0) + list(NAMES[word]))
    assert not set(os.listdir(o0)) & {"alt.mtx", "ref.mtx", "ad.mtx", "dp.mtx"}
    assert r.stdout == r0.stdout
    extra = [ln for ln in r.stderr.splitlines() if ln not in r0.stderr.splitlines()]
    s = mtx_write.summary(L, n_cells, *coo, word, "\t", True)
    assert len(extra) == 1 and extra[0].startswith("write_matrices %s: %d entries, %d with alt = ref = 0" % (word, s["n_entries"], s["n_dropped_keys"]))
    assert "%d lines, %d bytes in %s" % (s["lines_first"], s["bytes_first"], NAMES[word][0]) in extra[0]
    assert "%d lines, %d bytes in %s" % (s["lines_second"], s["bytes_second"], NAMES[word][1]) in extra[0]
    for f in os.listdir(o0):
        assert open(os.path.join(o0, f), "rb").read() == open(os.path.join(o, f), "rb").read(), f


def _same_run(host_bin, inputs, o, r, first, second, again, names, *extra):  # noqa: F811
    """the run of the binary on (first, second) with the barcodes.tsv and gt.tsv of the directory `names` is the run r that wrote o"""
    r2 = _run(host_bin, first, second, os.path.join(names, "barcodes.tsv"), inputs["vcf"], again, "-g", os.path.join(names, "gt.tsv"), *extra)
    assert r2.returncode == 0, r2.stderr
    assert r2.stdout == r.stdout
    files = sorted(os.listdir(again))
    assert "cellector_assignments.tsv" in files and "cellector.vcf" in files
    assert set(os.listdir(o)) - set(files) <= {"barcodes.tsv", "gt.tsv", "alt.mtx", "ref.mtx", "ad.mtx", "dp.mtx"}
    for f in files:
        assert open(os.path.join(again, f), "rb").read() == open(os.path.join(o, f), "rb").read(), f


@pytest.mark.gpu
@pytest.mark.parametrize("word", ["aligned", "sparse whole", "depth whole"])
def test_a_run_on_the_written_files_is_the_same_run(host_bin, inputs, written, tmp_path, word):  # noqa: F811
    o, r = written[word]
    w = word.split()[0]
    if w != "aligned":  # no entry with alt = ref = 0: the pair holds every key
        assert " 0 with alt = ref = 0" in r.stderr
    first, second = (os.path.join(o, n) for n in NAMES[w])
    _same_run(host_bin, inputs, o, r, first, second, str(tmp_path / "again"), o, *PAIR[w])


@pytest.mark.gpu
@pytest.mark.parametrize("word", ["sparse", "depth"])
def test_the_thinned_pair_reads_back_without_its_zero_entries(host_bin, inputs, written, mixture, tmp_path, word):  # noqa: F811
    """... and is then, through the join, the run on the aligned files of that smaller matrix"""
    coo, n_cells = mixture
    small = mtx_write.expected_read_back(*coo, word)
    assert len(small[0]) < len(coo[0])
    d = tmp_path / "small"
    d.mkdir()
    mtx_write.write_pair(d / "alt.mtx", d / "ref.mtx", L, n_cells, *small, "aligned", "\t", True)
    o, _ = written[word]
    r_small = _run(host_bin, str(d / "alt.mtx"), str(d / "ref.mtx"), os.path.join(o, "barcodes.tsv"), inputs["vcf"], str(tmp_path / "small_run"),
                   "-g", os.path.join(o, "gt.tsv"))
    assert r_small.returncode == 0, r_small.stderr
    first, second = (os.path.join(o, n) for n in NAMES[word])
    _same_run(host_bin, inputs, str(tmp_path / "small_run"), r_small, first, second, str(tmp_path / "again"), o, *PAIR[word])


@pytest.mark.gpu
def test_barcodes_of_the_cells_in_force(host_bin, inputs, tmp_path):  # noqa: F811
    """without --mix_* / --doublets the run writes no barcodes.tsv of its own: --write_matrices does, after --cells"""
    alt1, ref1, bc1 = inputs["first"]
    names = open(bc1).read().split()
    picked = [names[i] for i in range(0, N1, 2)]
    lst = tmp_path / "cells.tsv"
    lst.write_text("".join(n + "\n" for n in reversed(picked)))
    o = str(tmp_path / "o")
    r = _run(host_bin, alt1, ref1, bc1, inputs["vcf"], o, "--cells", str(lst), "--write_matrices", "aligned")
    assert r.returncode == 0, r.stderr
    assert open(os.path.join(o, "barcodes.tsv")).read().split() == picked  # the barcodes file's order
    dst = synth.generate_coo(L, N1, 0.1, seed=11, minority_fraction=0)
    t = restage.restage_coo(*dst, N1, np.arange(N1) % 2 == 0, 0.0, 4)
    for k, name in enumerate(("alt.mtx", "ref.mtx")):
        assert open(os.path.join(o, name), "rb").read() == mtx_write.file_bytes(L, t[4], *t[:4], k, "aligned", "\t", True), name
    # the flag alone: the input matrix again, under the combiner's header
    o2 = str(tmp_path / "o2")
    r = _run(host_bin, alt1, ref1, bc1, inputs["vcf"], o2, "--write_matrices", "aligned")
    assert r.returncode == 0, r.stderr
    assert open(os.path.join(o2, "barcodes.tsv")).read() == open(bc1).read()
    assert open(os.path.join(o2, "alt.mtx"), "rb").read() == mtx_write.file_bytes(L, N1, *dst, 0, "aligned", "\t", True)


@pytest.mark.gpu
def test_refusals(host_bin, inputs, tmp_path):  # noqa: F811
    alt1, ref1, bc1 = inputs["first"]
    # an input of the run under a name the flag writes, in the output directory, would be lost: refused, file intact
    mine = tmp_path / "mine"
    mine.mkdir()
    for word, name, flag in (("aligned", "alt.mtx", "-a"), ("sparse", "ref.mtx", "-r"), ("depth", "dp.mtx", "-r"), ("depth", "ad.mtx", "--mix_alt"),
                             ("aligned", "barcodes.tsv", "--barcodes")):
        src = {"-a": alt1, "-r": ref1, "--mix_alt": inputs["second"][0], "--barcodes": bc1}[flag]
        text = open(src, "rb").read()
        (mine / name).write_bytes(text)
        paths = {"-a": alt1, "-r": ref1, "--barcodes": bc1}
        extra = []
        if flag == "--mix_alt":
            extra = ["--mix_alt", str(mine / name), "--mix_ref", inputs["second"][1], "--mix_barcodes", inputs["second"][2]]
        else:
            paths[flag] = str(mine / name)
        args = [host_bin, "-a", paths["-a"], "-r", paths["-r"], "--barcodes", paths["--barcodes"], "--output_directory", str(mine), "--vcf", inputs["vcf"],
                "--write_matrices", word] + extra
        r = subprocess.run(args, capture_output=True, text=True, timeout=600)
        assert r.returncode == 1 and "overwrite" in r.stderr and name in r.stderr and "--write_matrices" in r.stderr, r.stderr
        assert (mine / name).read_bytes() == text
        assert sorted(os.listdir(mine)) == [name]  # refused before anything was written
        os.remove(mine / name)
    r = _run(host_bin, alt1, ref1, bc1, inputs["vcf"], str(tmp_path / "o"), "--write_matrices", "aligned", "--devices", "0,0")
    assert r.returncode == 1 and r.stderr.startswith("error: The argument '--write_matrices aligned' works on one GPU"), r.stderr
    r = _run(host_bin, alt1, ref1, bc1, inputs["vcf"], str(tmp_path / "o"), "--write_matrices", "packed")
    assert r.returncode == 1 and "expected aligned, sparse or depth" in r.stderr
