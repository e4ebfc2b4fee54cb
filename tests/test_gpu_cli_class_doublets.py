"""GPU: `host/cellector --doublets <file> --classes <file> --class_doublets true [--refine_classes <max_iter>]` — a small mixture
of three genotypes with synthetic doublets added by --doublets: cellector_classes.tsv holds the Python binding's doublet scoring of
the same labelling rendered the same way, with doublet_posterior and doublet_pair at the end and class_assignment doublet where the
call is 1; every refine step's stderr line ends in held=<n>; without --class_doublets the file is what it was."""
import os
import subprocess

import numpy as np
import pytest

import class_reference as cr
from test_host_cli import host_bin, rust_display  # noqa: F401

pytestmark = pytest.mark.gpu

NAMES = ["donorB", "donorA", "third"]  # numbered by first appearance in the file
NP = 40


@pytest.fixture(scope="module")
def runs(host_bin, tmp_path_factory):
    from cellector_amd import synth
    tmp = str(tmp_path_factory.mktemp("class_doublets"))
    L, N, coo, truth = cr.mixture()
    alt, ref = synth.write_mtx_pair(tmp, L, N, *coo, header_nnz=0)
    bc = os.path.join(tmp, "barcodes.tsv")
    synth.write_barcodes(bc, N)
    barcodes = open(bc).read().splitlines()
    rng = np.random.default_rng(23)
    a, b = [], []
    while len(a) < NP:  # cross-genotype parents, every pair once
        i, j = (int(x) for x in rng.integers(0, cr.MIX_N, 2))
        if truth[i] != truth[j] and (i, j) not in zip(a, b):
            a.append(i); b.append(j)
    pf = os.path.join(tmp, "pairs.tsv")
    with open(pf, "w") as f:
        f.writelines(f"{barcodes[i]}\t{barcodes[j]}\n" for i, j in zip(a, b))
    every = barcodes + [f"{barcodes[i]}+{barcodes[j]}" for i, j in zip(a, b)]
    # the labelling a caller would have: the genotypes with some noise, a doublet under its first parent's, 5 % unlabelled
    lab = np.concatenate([truth, truth[a]]).astype(np.uint8)
    r = rng.random(len(lab))
    lab[r < 0.1] = rng.integers(0, 3, int((r < 0.1).sum()))
    lab[r > 0.95] = 255
    lab[:3] = [0, 1, 2]
    lab[N:N + 3] = truth[a][:3]
    cf = os.path.join(tmp, "classes.tsv")
    with open(cf, "w") as f:
        f.writelines(f"{every[i]}\t{NAMES[lab[i]]}\n" for i in range(len(lab)) if lab[i] != 255)
    out = {}
    for name, extra in (("classes", ["--classes", cf]), ("off", ["--classes", cf, "--class_doublets", "false"]),
                        ("doublets", ["--classes", cf, "--class_doublets", "true"]),
                        ("refine", ["--classes", cf, "--class_doublets", "true", "--refine_classes", "6"])):
        d = os.path.join(tmp, name)
        cmd = [host_bin, "-a", alt, "-r", ref, "--output_directory", d, "--min_alt", "4", "--min_ref", "4", "--barcodes", bc,
               "--doublets", pf] + extra
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr
        out[name] = dict(dir=d, stdout=res.stdout, stderr=res.stderr)
    return dict(alt=alt, ref=ref, barcodes=every, labels=lab, a=np.array(a), b=np.array(b), host_bin=host_bin, tmp=tmp, bc=bc, **out)


def test_without_the_flag_nothing_changes(runs):
    a = runs["classes"]
    files = sorted(os.listdir(a["dir"]))
    assert "cellector_classes.tsv" in files
    for name in ("off", "doublets", "refine"):
        b = runs[name]
        assert a["stdout"] == b["stdout"] and sorted(os.listdir(b["dir"])) == files
        for f in files:
            same = open(os.path.join(a["dir"], f), "rb").read() == open(os.path.join(b["dir"], f), "rb").read()
            assert same == (f != "cellector_classes.tsv" or name == "off"), (name, f)
    assert "held=" not in a["stderr"] and "held=" not in runs["doublets"]["stderr"]
    r = subprocess.run([runs["host_bin"], "-a", runs["alt"], "-r", runs["ref"], "--output_directory", os.path.join(runs["tmp"], "no"),
                        "--barcodes", runs["bc"], "--class_doublets", "true"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "--classes" in r.stderr


def test_the_table_is_the_binding(runs):
    from cellector_amd import Cellector
    g = Cellector(0)
    g.load_mtx(runs["alt"], runs["ref"], 4, 4)
    g.add_doublets(runs["a"], runs["b"])
    g.ingest_finish(4, 4)
    lab, bcs = runs["labels"], runs["barcodes"]
    n = len(lab)
    assert g.dims().total_cells == n
    epc = g.entries_per_cell()
    head = (["barcode", "input_label", "class_assignment", "qual"] + [f"log_likelihood_{x}" for x in NAMES] + [f"posterior_{x}" for x in NAMES]
            + ["doublet_posterior", "doublet_pair"])
    for name, max_iter in (("doublets", 0), ("refine", 6)):
        rows = [ln.split("\t") for ln in open(os.path.join(runs[name]["dir"], "cellector_classes.tsv")).read().splitlines()]
        assert rows[0] == head and len(rows) == n + 1
        r = g.refine_class_doublets(lab, 3, max_iter=max_iter)
        res = g.class_doublets(r["labels"], 3, held=r["held"])
        for c in range(n):
            b = int(res["best"][c])
            ok = res["posterior"][b, c] > 0.999 and epc[c] >= 30
            what = "doublet" if (res["call"][c] and epc[c] >= 30) else NAMES[b] if ok else "unassigned"
            pa, pb = (int(x) for x in res["best_pair"][c])
            want = ([bcs[c], "na" if lab[c] == 255 else NAMES[lab[c]], what, str(int(res["qual"][c]))]
                    + [rust_display(float(res["ll"][k, c])) for k in range(3)] + [rust_display(float(res["posterior"][k, c])) for k in range(3)]
                    + [rust_display(float(res["doublet_posterior"][c])), f"{NAMES[pa]}+{NAMES[pb]}" if pa != 255 else "na"])
            assert rows[1 + c] == want, (name, c)
        lines = [ln for ln in runs[name]["stderr"].splitlines() if ln.startswith("refine_classes step")]
        assert len(lines) == r["summary"].iterations
        if max_iter:
            assert 2 <= len(lines) <= 6 and r["summary"].converged == 1
            sizes = " ".join(f"{x}={r['summary'].class_cells[k]}" for k, x in enumerate(NAMES))
            assert lines[-1].endswith(f"moved {r['summary'].n_moved_last}, class sizes {sizes} held={r['summary'].n_held}")
            assert all(" held=" in ln for ln in lines)
        # the planted doublets that carry a label come out as doublets, and cells are called that way only with the flag
        calls = np.array([x[2] == "doublet" for x in rows[1:]])
        planted = np.arange(n) >= n - NP
        assert calls[planted & (lab != 255)].any() and [x[1] for x in rows[1:]][n - 1] == ("na" if lab[n - 1] == 255 else NAMES[lab[n - 1]])
        assert {x[2] for x in rows[1:]} <= set(NAMES) | {"unassigned", "doublet"}
    assert (lab[n - NP:] != 255).sum() >= NP - 8  # (the doublets' barcodes <A>+<B> were found in the classes file)
    g.close()
