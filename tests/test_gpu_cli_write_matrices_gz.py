"""GPU: `host/cellector --write_matrices <word> --write_matrices_gz true` writes the pair as alt.mtx.gz / ref.mtx.gz (ad.mtx.gz /
dp.mtx.gz): each file is bgzf.compress (cellector_amd/bgzf.py) of the file the run with --write_matrices alone writes; a second run
of the binary on the .gz pair gives every output byte for byte the outputs of the run on the plain pair; without the flag the
output directory is what it was; the flag without --write_matrices is a usage error.

The case is tests/test_gpu_cli_write_matrices.py's: the mixture of tests/test_gpu_cli_combine.py, thinned for the aligned word and
whole for the depth word (a depth pair lacks the entries with alt = ref = 0)."""
import gzip
import os

import pytest

from cellector_amd import bgzf
from test_gpu_cli_combine import L, N1, N2, _run, inputs  # noqa: F401
from test_host_cli import host_bin  # noqa: F401

GZ = ["--write_matrices_gz", "true"]
ALL_NAMES = {"alt.mtx", "ref.mtx", "ad.mtx", "dp.mtx", "alt.mtx.gz", "ref.mtx.gz", "ad.mtx.gz", "dp.mtx.gz"}


def _mix_args(inputs, thinned=True):  # noqa: F811
    alt2, ref2, bc2 = inputs["second"]
    return ["--mix_alt", alt2, "--mix_ref", ref2, "--mix_barcodes", bc2, "--mix_cells", inputs["lst"]] + (["--downsample_rate", "0.2"] if thinned else [])


@pytest.fixture(scope="module")
def written(host_bin, inputs, tmp_path_factory):  # noqa: F811
    alt1, ref1, bc1 = inputs["first"]
    out = {}
    for key, thinned, flags in (("none", True, []), ("aligned", True, ["--write_matrices", "aligned"]),
                                ("aligned gz", True, ["--write_matrices", "aligned"] + GZ),
                                ("depth", False, ["--write_matrices", "depth"]), ("depth gz", False, ["--write_matrices", "depth"] + GZ)):
        o = str(tmp_path_factory.mktemp("gz_" + key.replace(" ", "_")))
        r = _run(host_bin, alt1, ref1, bc1, inputs["vcf"], o, *_mix_args(inputs, thinned), *flags)
        assert r.returncode == 0, r.stderr
        out[key] = (o, r)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("word,names", [("aligned", ("alt.mtx", "ref.mtx")), ("depth", ("ad.mtx", "dp.mtx"))])
def test_the_gz_pair_is_the_compressed_plain_pair(written, word, names):
    (o, r), (og, rg) = written[word], written[word + " gz"]
    for name in names:
        text = open(os.path.join(o, name), "rb").read()
        packed = open(os.path.join(og, name + ".gz"), "rb").read()
        assert packed == bgzf.compress(text), name
        assert gzip.decompress(packed) == text and len(packed) < len(text) / 2
    # the same directory but for the two names; the same stdout; the stderr line gains the compressed sizes
    assert sorted(os.listdir(og)) == sorted((set(os.listdir(o)) - set(names)) | {n + ".gz" for n in names})
    assert rg.stdout == r.stdout
    line = [ln for ln in r.stderr.splitlines() if ln.startswith("write_matrices ")]
    line_gz = [ln for ln in rg.stderr.splitlines() if ln.startswith("write_matrices ")]
    assert len(line) == len(line_gz) == 1
    sizes = tuple(os.path.getsize(os.path.join(og, n + ".gz")) for n in names)
    assert line_gz[0].startswith(line[0].replace(names[0], names[0] + ".gz").replace(names[1], names[1] + ".gz") + "; compressed to %d and %d bytes in " % sizes)
    for f in set(os.listdir(o)) - set(names):
        assert open(os.path.join(o, f), "rb").read() == open(os.path.join(og, f), "rb").read(), f


@pytest.mark.gpu
def test_without_the_flag_nothing_appears_or_changes(written):
    (o0, r0), (o, r) = written["none"], written["aligned"]
    assert not set(os.listdir(o0)) & ALL_NAMES
    assert sorted(os.listdir(o)) == sorted(os.listdir(o0) + ["alt.mtx", "ref.mtx"])  # --write_matrices alone: no .gz
    for f in os.listdir(o0):
        assert open(os.path.join(o0, f), "rb").read() == open(os.path.join(o, f), "rb").read(), f


@pytest.mark.gpu
@pytest.mark.parametrize("word,names,extra", [("aligned", ("alt.mtx", "ref.mtx"), []), ("depth", ("ad.mtx", "dp.mtx"), ["--matrix_pair", "depth"])])
def test_a_run_on_the_gz_pair_is_the_run_on_the_plain_pair(host_bin, inputs, written, tmp_path, word, names, extra):  # noqa: F811
    (o, _), (og, _) = written[word], written[word + " gz"]
    runs = []
    for d, suffix, again in ((o, "", tmp_path / "plain"), (og, ".gz", tmp_path / "gz")):
        r = _run(host_bin, os.path.join(d, names[0] + suffix), os.path.join(d, names[1] + suffix), os.path.join(d, "barcodes.tsv"), inputs["vcf"],
                 str(again), "-g", os.path.join(d, "gt.tsv"), *extra)
        assert r.returncode == 0, r.stderr
        runs.append((str(again), r))
    (a, ra), (b, rb) = runs
    assert ra.stdout == rb.stdout
    files = sorted(os.listdir(a))
    assert files == sorted(os.listdir(b)) and "cellector_assignments.tsv" in files and "cellector.vcf" in files
    for f in files:
        assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), f


@pytest.mark.gpu
def test_usage_errors(host_bin, inputs, tmp_path):  # noqa: F811
    alt1, ref1, bc1 = inputs["first"]
    r = _run(host_bin, alt1, ref1, bc1, inputs["vcf"], str(tmp_path / "o"), *GZ)
    assert r.returncode == 1 and r.stderr.startswith("error: The argument '--write_matrices_gz true' requires '--write_matrices <aligned|sparse|depth>'")
    assert not os.path.exists(tmp_path / "o") or not set(os.listdir(tmp_path / "o")) & ALL_NAMES
    # an input of the run under one of the names the flags write is refused before anything is written
    o = tmp_path / "own"
    o.mkdir()
    mine = o / "alt.mtx.gz"
    mine.write_bytes(bgzf.compress(open(alt1, "rb").read()))
    before = mine.read_bytes()
    r = _run(host_bin, str(mine), ref1, bc1, inputs["vcf"], str(o), "--write_matrices", "aligned", *GZ)
    assert r.returncode == 1 and "overwrite" in r.stderr and "alt.mtx.gz" in r.stderr, r.stderr
    assert mine.read_bytes() == before
