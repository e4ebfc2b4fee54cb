"""CPU: `host/cellector` refuses a bad input file before it opens a device, and every option parses by the one table.

The input stage (read_inputs: --cells, --mix_*, --doublets, the barcode lists, --classes, the overwrite guard) makes no
library call: each refusal below is exit 1 with its message and nothing else on stderr.  On a box without a GPU the device
open that follows ends the run with exit 101, so exit 1 there also says that the refusal came first; the matrices are
never parsed (L = 60, N = 40)."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from test_host_cli import _write_inputs, host_bin  # noqa: F401

L, N = 60, 40


@pytest.fixture(scope="module")
def inp(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("cli_inputs"))
    _, alt, ref, bc, gt, vcf = _write_inputs(tmp, L, N, 0.1, 3, 0.1)
    return dict(tmp=tmp, alt=alt, ref=ref, bc=bc, gt=gt, names=open(bc).read().split())


def refusals(inp):
    """(id, extra arguments, message) of every refusal of the input stage"""
    tmp, bc, n = inp["tmp"], inp["bc"], inp["names"]

    def w(name, text):
        path = os.path.join(tmp, name)
        with open(path, "w") as f:
            f.write(text)
        return path

    kept = w("kept.tsv", "".join(f"{b}\n" for b in n[:10]))
    mix = ["--mix_alt", inp["alt"], "--mix_ref", inp["ref"], "--mix_barcodes", bc]
    with_pair_name = w("barcodes_with_pair.tsv", "".join(f"{b}\n" for b in n) + f"{n[0]}+{n[1]}\n")
    cases = []

    def case(cid, args, message):
        cases.append((cid, args, message))

    p = w("cells_unknown.tsv", f"{n[0]}\nNOPE-1\n")
    case("cells_unknown", ["--cells", p], f"error: --cells {p} line 2: barcode 'NOPE-1' is not in the barcodes file {bc}")
    p = w("cells_nothing.tsv", "\n\n")
    case("cells_nothing", ["--cells", p], f"error: --cells {p} lists no barcode")
    p = w("mix_cells_unknown.tsv", "NOPE-1\tx\n")
    case("mix_cells_unknown", mix + ["--mix_cells", p], f"error: --mix_cells {p} line 1: barcode 'NOPE-1' is not in the barcodes file {bc}")
    p = w("mix_cells_nothing.tsv", "\n")
    case("mix_cells_nothing", mix + ["--mix_cells", p], f"error: --mix_cells {p} lists no barcode")

    p = w("dbl_one_column.tsv", f"{n[0]}\n")
    case("doublets_one_column", ["--doublets", p], f"error: --doublets {p} line 1: two tab-separated barcodes expected, got '{n[0]}'")
    p = w("dbl_unknown.tsv", f"\n{n[0]}\tNOPE-1\n")
    case("doublets_unknown", ["--doublets", p],
         f"error: --doublets {p} line 2: barcode 'NOPE-1' is not among the run's cells (the barcodes file {bc})")
    p = w("dbl_dropped.tsv", f"{n[0]}\t{n[20]}\n")
    case("doublets_unknown_after_cells", ["--cells", kept, "--doublets", p],
         f"error: --doublets {p} line 1: barcode '{n[20]}' is not among the run's cells (the barcodes file {bc} after --cells)")
    p = w("dbl_self.tsv", f"{n[3]}\t{n[3]}\n")
    case("doublets_self_pair", ["--doublets", p], f"error: --doublets {p} line 1: barcode '{n[3]}' is paired with itself")
    p = w("dbl_twice.tsv", f"{n[0]}\t{n[1]}\n{n[2]}\t{n[3]}\n{n[0]}\t{n[1]}\n")
    case("doublets_repeated_pair", ["--doublets", p],
         f"error: --doublets {p} line 3: the pair is line 1 already: the cell '{n[0]}+{n[1]}' would exist twice")
    p = w("dbl_present.tsv", f"{n[0]}\t{n[1]}\n")
    case("doublets_name_present", ["--barcodes", with_pair_name, "--doublets", p],
         f"error: --doublets {p} line 1: the run has a cell named '{n[0]}+{n[1]}' already")
    p = w("dbl_empty.tsv", "")
    case("doublets_empty", ["--doublets", p], f"error: --doublets {p} lists no pair")

    for flag in ("initial_minority", "cell_detail"):
        p = w(f"{flag}_dropped.tsv", f"{n[1]}\n{n[20]}\t0\n")
        case(f"{flag}_dropped_by_cells", ["--cells", kept, f"--{flag}", p],
             f"error: --{flag} {p} line 2: barcode '{n[20]}' is not among the cells --cells {kept} keeps")
        p = w(f"{flag}_unknown.tsv", "NOPE-1\n")
        case(f"{flag}_unknown", [f"--{flag}", p], f"error: --{flag} {p} line 1: barcode 'NOPE-1' is not in the barcodes file {bc}")

    p = w("classes_17.tsv", "".join(f"{n[i]}\tL{i}\n" for i in range(17)))
    case("classes_17th_label", ["--classes", p], f"error: --classes {p}: more than 16 distinct labels ('L16' is the 17th)")
    p = w("classes_empty.tsv", "")
    case("classes_no_label", ["--classes", p], f"error: --classes {p}: no label")

    p = w("dbl_ok.tsv", f"{n[0]}\t{n[1]}\n")  # the output directory is the directory of --barcodes (named barcodes.tsv)
    case("overwrite_guard", ["--doublets", p, "--output_directory", tmp],
         f"error: the run's barcodes.tsv would overwrite the --barcodes file {bc}: choose another --output_directory")
    return cases


def test_bad_input_files_are_refused_before_a_device_is_opened(host_bin, inp, tmp_path):
    before = open(inp["bc"]).read(), open(inp["gt"]).read()
    for cid, args, message in refusals(inp):
        cmd = [host_bin, "-a", inp["alt"], "-r", inp["ref"]]
        if "--barcodes" not in args:
            cmd += ["--barcodes", inp["bc"]]
        if "--output_directory" not in args:
            cmd += ["--output_directory", str(tmp_path / cid)]
        r = subprocess.run(cmd + args, capture_output=True, text=True, timeout=60)
        print(cid, r.returncode, repr(r.stderr))
        assert r.returncode == 1, cid
        assert r.stderr == message + "\n", cid
        assert r.stdout == "", cid
    assert (open(inp["bc"]).read(), open(inp["gt"]).read()) == before  # (the overwrite guard wrote neither barcodes.tsv nor gt.tsv)


def test_every_option_of_the_help_takes_one_value(host_bin):
    r = subprocess.run([host_bin, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    names = []
    for line in r.stdout.split("OPTIONS:\n")[1].splitlines():
        if re.match(r"    (-\w, |    )--\w", line):  # the head of an option's paragraph: 4 columns in, before the two-space gap
            names += re.findall(r"--(\w+) <", re.split(r"\s{2,}", line.strip())[0])
    assert len(names) >= 45 and len(set(names)) == len(names)
    assert {"alt", "min_loci_for_assignment", "devices", "mix_ref", "mix_barcodes", "cluster_mask", "donor_fit_iqr"} <= set(names)
    runs = []
    for name in names:
        runs.append(([host_bin, f"--{name}"], f"error: The argument '--{name} <{name}>' requires a value but none was supplied\n"))
        runs.append(([host_bin, f"--{name}", "x", f"--{name}", "x"], f"error: The argument '--{name} <{name}>' was provided more than once\n"))
    with ThreadPoolExecutor(8) as pool:  # (ninety process starts: side by side they take a fraction of a second)
        done = list(pool.map(lambda run: subprocess.run(run[0], capture_output=True, text=True), runs))
    for (cmd, message), r in zip(runs, done):
        assert (r.returncode, r.stderr, r.stdout) == (1, message, ""), cmd
