"""GPU: `host/cellector --classes <file> [--refine_classes <max_iter>]` — cellector_classes.tsv holds the Python binding's class
posteriors of the same labelling rendered the same way; every other output file and stdout are the run's without the two flags;
every refine step prints one stderr line."""
import os
import subprocess

import numpy as np
import pytest

from test_host_cli import host_bin, rust_display  # noqa: F401

pytestmark = pytest.mark.gpu

L, N, D = 1500, 700, 0.10
NAMES = ["donorB", "donorA", "third"]  # numbered by first appearance in the file


def _labels():
    rng = np.random.default_rng(11)
    lab = rng.choice(3, N, p=[0.6, 0.3, 0.1]).astype(np.uint8)
    lab[0] = 0  # (the file's first line names class 0 first, the next new label is 1, ...)
    lab[1], lab[2] = 1, 2
    lab[rng.random(N) < 0.05] = 255
    lab[:3] = [0, 1, 2]
    return lab


@pytest.fixture(scope="module")
def runs(host_bin, tmp_path_factory):
    from cellector_amd import synth
    tmp = str(tmp_path_factory.mktemp("classes"))
    coo = synth.generate_coo(L, N, D)
    alt, ref = synth.write_mtx_pair(tmp, L, N, *coo, header_nnz=0)
    bc = os.path.join(tmp, "barcodes.tsv")
    synth.write_barcodes(bc, N)
    barcodes = open(bc).read().splitlines()
    lab = _labels()
    cf = os.path.join(tmp, "classes.tsv")
    with open(cf, "w") as f:
        for i in range(N):
            if lab[i] != 255:
                f.write(f"{barcodes[i]}\t{NAMES[lab[i]]}\n")
        f.write("not-a-barcode-of-this-run\tdonorA\n")  # ignored, like a ground-truth line of an unknown barcode
    out = {}
    for name, extra in (("plain", []), ("classes", ["--classes", cf]), ("refine", ["--classes", cf, "--refine_classes", "5"])):
        d = os.path.join(tmp, name)
        cmd = [host_bin, "-a", alt, "-r", ref, "--output_directory", d, "--min_alt", "4", "--min_ref", "4", "--barcodes", bc] + extra
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        out[name] = dict(dir=d, stdout=r.stdout, stderr=r.stderr)
    return dict(alt=alt, ref=ref, barcodes=barcodes, labels=lab, **out)


def _expected_rows(g, barcodes, in_lab, lab, threshold=0.999, min_loci=30):
    res = g.class_posteriors(lab, 3)
    epc = g.entries_per_cell()
    rows = []
    for c in range(N):
        b = int(res["best"][c])
        ok = res["posterior"][b, c] > threshold and epc[c] >= min_loci
        rows.append([barcodes[c], "na" if in_lab[c] == 255 else NAMES[in_lab[c]], NAMES[b] if ok else "unassigned", str(int(res["qual"][c]))]
                    + [rust_display(float(res["ll"][k, c])) for k in range(3)] + [rust_display(float(res["posterior"][k, c])) for k in range(3)])
    return rows


def test_every_other_output_is_the_plain_run(runs):
    a = runs["plain"]
    files = sorted(os.listdir(a["dir"]))
    assert "cellector_assignments.tsv" in files and "cellector_classes.tsv" not in files
    for name in ("classes", "refine"):
        b = runs[name]
        assert a["stdout"] == b["stdout"]
        assert sorted(os.listdir(b["dir"])) == sorted(files + ["cellector_classes.tsv"])
        for f in files:
            assert open(os.path.join(a["dir"], f), "rb").read() == open(os.path.join(b["dir"], f), "rb").read(), (name, f)
    assert "refine_classes step" not in runs["classes"]["stderr"] and "refine_classes step" not in a["stderr"]


def test_the_table_is_the_binding(runs):
    from cellector_amd import Cellector
    g = Cellector(0)
    g.load_mtx(runs["alt"], runs["ref"], 4, 4)
    g.run(5.0)  # (the class calls do not read the EM state: the table is the same before and after the loop)
    lab = runs["labels"]
    head = ["barcode", "input_label", "class_assignment", "qual"] + [f"log_likelihood_{n}" for n in NAMES] + [f"posterior_{n}" for n in NAMES]
    for name, max_iter in (("classes", 0), ("refine", 5)):
        rows = [ln.split("\t") for ln in open(os.path.join(runs[name]["dir"], "cellector_classes.tsv")).read().splitlines()]
        assert rows[0] == head and len(rows) == N + 1
        r = g.refine_classes(lab, 3, max_iter=max_iter)
        want = _expected_rows(g, runs["barcodes"], lab, r["labels"])
        for got, w in zip(rows[1:], want):
            assert got == w
        lines = [ln for ln in runs[name]["stderr"].splitlines() if ln.startswith("refine_classes step")]
        assert len(lines) == r["summary"].iterations
        if max_iter:
            assert 1 <= len(lines) <= 5 and lines[0].startswith("refine_classes step 1: moved ")
            sizes = " ".join(f"{n}={r['summary'].class_cells[k]}" for k, n in enumerate(NAMES))
            assert lines[-1].endswith(f"moved {r['summary'].n_moved_last}, class sizes {sizes}")
        assert {x[2] for x in rows[1:]} <= set(NAMES) | {"unassigned"}
    g.close()
