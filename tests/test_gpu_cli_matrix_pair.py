"""GPU: `host/cellector --matrix_pair <aligned|join|depth>` — one planted dataset written three ways gives one run, byte for byte:
the completed aligned pair of the numpy twin's join (read line by line, the default), an alt / ref pair with each file's zero lines
dropped and the ref file's lines shuffled (join), and an alt-depth / total-depth pair (depth).  --mix_alt / --mix_ref are read the
same way."""
import os
import subprocess

import numpy as np
import pytest

from test_host_cli import host_bin  # noqa: F401

L, N, N2 = 1500, 700, 200


def _run(host_bin, alt, ref, bc, vcf, out, *extra):
    cmd = [host_bin, "-a", alt, "-r", ref, "--output_directory", out, "--min_alt", "4", "--min_ref", "4", "--barcodes", bc, "--vcf", vcf]
    return subprocess.run(cmd + list(extra), capture_output=True, text=True, timeout=600)


def three_ways(directory, n_cells, coo, seed):
    """{aligned, join, depth: (first path, second path)} of one matrix"""
    from cellector_amd import join, synth
    l, c, a, r = coo
    rng = np.random.default_rng(seed)

    def write(name, idx, vals):
        path = os.path.join(directory, name)
        body = np.stack([l[idx].astype(np.int64) + 1, c[idx].astype(np.int64) + 1, vals[idx].astype(np.int64)], 1)
        with open(path, "w") as f:
            f.write("%%MatrixMarket matrix coordinate integer general\n%\n" + f"{L} {n_cells} {len(idx)}\n")
            np.savetxt(f, body, fmt="%d")
        return path
    os.makedirs(directory, exist_ok=True)
    nz_a, nz_r, nz_d = np.flatnonzero(a), rng.permutation(np.flatnonzero(r)), np.flatnonzero(a + r)
    pair = join.join_coo((l[nz_a], c[nz_a], a[nz_a]), (l[nz_r], c[nz_r], r[nz_r]), join.MODE_REF, L, n_cells)
    assert len(nz_a) < len(l) and len(nz_r) < len(l) and pair[4]["n_first_only"] > 0 and pair[4]["n_second_only"] > 0
    return dict(aligned=synth.write_mtx_pair(os.path.join(directory, "aligned"), L, n_cells, *pair[:4]),
                join=(write("alt.mtx", nz_a, a), write("ref_shuffled.mtx", nz_r, r)),
                depth=(write("ad.mtx", nz_a, a), write("dp.mtx", nz_d, a + r)))


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    from cellector_amd import synth
    tmp = str(tmp_path_factory.mktemp("cli_matrix_pair"))
    main = three_ways(os.path.join(tmp, "main"), N, synth.generate_coo(L, N, 0.1, seed=4, minority_fraction=0.08), 1)
    mix = three_ways(os.path.join(tmp, "mix"), N2, synth.generate_coo(L, N2, 0.1, seed=12, minority_fraction=0), 2)
    bc, bc2 = os.path.join(tmp, "barcodes.tsv"), os.path.join(tmp, "barcodes2.tsv")
    synth.write_barcodes(bc, N)
    synth.write_barcodes(bc2, N2)
    vcf = os.path.join(tmp, "variants.vcf")
    with open(vcf, "w") as f:
        f.write("##fileformat=VCFv4.2\n##source=synthetic\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        for i in range(L):
            f.write(f"chr{1 + i % 22}\t{1000 + 37 * i}\t.\tA\tG\t50\tPASS\t.\n")
    return dict(main=main, mix=mix, bc=bc, bc2=bc2, vcf=vcf)


def _same_outputs(runs, dirs):
    for r in runs:
        assert r.returncode == 0, r.stderr
    files = sorted(os.listdir(dirs[0]))
    assert "cellector_assignments.tsv" in files and "cellector.vcf" in files
    for r, d in zip(runs[1:], dirs[1:]):
        assert r.stdout == runs[0].stdout
        assert sorted(os.listdir(d)) == files
        for f in files:
            assert open(os.path.join(dirs[0], f), "rb").read() == open(os.path.join(d, f), "rb").read(), (d, f)
    return files


@pytest.mark.gpu
def test_three_ways_to_write_a_matrix_give_one_run(host_bin, inputs, tmp_path):
    dirs = [str(tmp_path / w) for w in ("aligned", "join", "depth")]
    runs = [_run(host_bin, *inputs["main"][w], inputs["bc"], inputs["vcf"], d, "--matrix_pair", w) for w, d in zip(("aligned", "join", "depth"), dirs)]
    _same_outputs(runs, dirs)
    rows = open(os.path.join(dirs[0], "cellector_assignments.tsv")).read().splitlines()
    assert len(rows) == 1 + N and any(r.split("\t")[1] == "0" for r in rows[1:])  # (the planted minority is found)
    # one stderr line counts the keys; the aligned run has none
    for r, w in zip(runs[1:], ("join", "depth")):
        line = [x for x in r.stderr.splitlines() if x.startswith("matrix_pair ")]
        assert len(line) == 1 and line[0].startswith(f"matrix_pair {w}: ") and "keys in both" in line[0] and "staged" in line[0], r.stderr
    assert "matrix_pair" not in runs[0].stderr
    # a depth pair read as alt / ref is no error (the counts are legal), an alt / ref pair read as depth is: its smallest key is named
    r = _run(host_bin, *inputs["main"]["join"], inputs["bc"], inputs["vcf"], str(tmp_path / "wrong"), "--matrix_pair", "depth")
    assert r.returncode != 0 and "depth below alt at (locus " in r.stderr, r.stderr


@pytest.mark.gpu
def test_mix_pair_is_read_the_same_way(host_bin, inputs, tmp_path):
    dirs = [str(tmp_path / w) for w in ("aligned", "depth")]
    runs = [_run(host_bin, *inputs["main"][w], inputs["bc"], inputs["vcf"], d, "--matrix_pair", w, "--mix_alt", inputs["mix"][w][0], "--mix_ref",
                 inputs["mix"][w][1], "--mix_barcodes", inputs["bc2"]) for w, d in zip(("aligned", "depth"), dirs)]
    files = _same_outputs(runs, dirs)
    assert "gt.tsv" in files and "barcodes.tsv" in files
    assert len(open(os.path.join(dirs[1], "cellector_assignments.tsv")).read().splitlines()) == 1 + N + N2
    assert len([x for x in runs[1].stderr.splitlines() if x.startswith("matrix_pair depth: ")]) == 2
