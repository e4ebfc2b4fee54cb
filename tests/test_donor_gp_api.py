"""CPU: the soft donor calls' C ABI as the binding sees it (declared behind cellector_match_donors and in front of the ambient block,
exported, bound; a null ctx is refused; the header states the model), donors.read_donor_vcf_gp on hand-written VCFs (GP, GL, PL,
swapped alleles, the fallback to GT, malformed fields, gzip), csrc/donor_vcf_host.h compiled as a plain host program against it, and
the host binary's usage errors and help text for --donor_field."""
import ctypes
import gzip
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from cellector_amd import donors, ffi
from test_host_cli import host_bin  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "cellector_ffi.h")).read()

ARGS = {
    "cellector_donor_posteriors_gp": ["ctx", "gp", "n_donors", "p", "log_prior", "anchor", "mask", "ll", "pair_ll", "posterior",
                                      "pair_posterior", "doublet_posterior", "best", "second", "best_pair", "n_entries", "status",
                                      "anchor_out", "out", "tab1", "tab2"],
    "cellector_donor_weights": ["ctx", "gp", "n_donors", "w", "kind"],
    "cellector_match_donors_gp": ["ctx", "labels", "n_classes", "gp", "n_donors", "p", "mask", "ll", "best", "margin", "cells"],
}


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    m = re.search(r"cellector_status\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared"
    return [a.strip() for a in m.group(1).split(",")]


def test_declared_exported_and_bound(hip_lib_path):
    lib = ffi.load_library(hip_lib_path)
    for name, args in ARGS.items():
        decl = _declared(name)
        assert [re.findall(r"[A-Za-z_][A-Za-z_0-9]*", a)[-1] for a in decl] == args, name
        res, argtypes = ffi.SIGNATURES[name]
        assert hasattr(lib, name) and res is ctypes.c_int and len(argtypes) == len(args), name
        for a, t in zip(decl, argtypes):
            assert t is (ctypes.c_void_p if "*" in a else ctypes.c_uint32), (name, a, t)
        assert any(a.startswith("const float *gp") for a in decl), name
    for m in ("donor_posteriors_gp", "donor_weights", "match_donors_gp"):
        assert callable(getattr(ffi.Cellector, m))
    at = [HEADER.index(s) for s in ("cellector_status cellector_match_donors(", "cellector_status cellector_donor_posteriors_gp(",
                                    "cellector_status cellector_donor_weights(", "cellector_status cellector_match_donors_gp(",
                                    "ambient fraction estimation", "cellector_status cellector_ambient_default_params(")]
    assert at == sorted(at)
    for phrase in ("ambient fraction estimation", "genotype clusters without labels", "---- class genotypes"):
        assert HEADER.count(phrase) == 1, phrase
    for f in ("one_hot", "hard_codes", "soft_weights", "soft_singlet_sums", "soft_pair_sums", "soft_match_sums", "posteriors_gp", "match_gp",
              "read_donor_vcf_gp", "parse_weights"):
        assert callable(getattr(donors, f)), f


def test_null_ctx_is_refused(hip_lib_path):
    lib = ffi.load_library(hip_lib_path)
    assert lib.cellector_donor_posteriors_gp(None, None, 3, *([None] * 18)) == 1
    assert lib.cellector_donor_weights(None, None, 3, None, None) == 1
    assert lib.cellector_match_donors_gp(None, None, 2, None, 3, *([None] * 6)) == 1


def test_header_states_the_model():
    beg = HEADER.index("donor calls from genotype probabilities")
    block = HEADER[beg:HEADER.index("cellector_status cellector_donor_posteriors_gp(")]
    for word in ("three NaN", "not all zero", "CELLECTOR_EINVAL", "(((double)gp_0 + (double)gp_1) + (double)gp_2)", "P = { g : w_g > 0 }",
                 "kind [L][D]", "4 = a soft row", "bit for bit", "m = the maximum of t_g over P", "w_g exp(t_g - m)", "term = m + log(z)",
                 "0 exp(+big)", "(a la_3) + (r lb_3)", "log(1.0) = 0.0", "the hard call's bits", "tab2[l][4 g + h]", "(w_g w_h) exp(t_gh - m)",
                 "a copy of ll[c][a_c]", "steps 4 to 8", "cellector_match_donors_gp", "byte for byte", "CELLECTOR_EDEVICE", "CELLECTOR_ENOMEM",
                 "12 D bytes per locus of the matrix", "25 D + 321 B per used locus", "32 D + 17 B per cell", "16 K B", "never touched"):
        assert word in block, word


def test_hard_codes_and_one_hot():
    nan = np.nan
    gp = np.array([[[0.2, 0.5, 0.3], [0.5, 0.5, 0.0], [0.0, 0.4, 0.4], [nan, nan, nan], [0, 0, 7], [1e-30, 0, 0]]], np.float32)
    assert donors.hard_codes(gp).tolist() == [[1, 0, 1, 3, 2, 0]] and donors.hard_codes(gp).dtype == np.uint8
    gt = np.array([[0, 1, 2, 3]], np.uint8)
    oh = donors.one_hot(gt)
    assert oh.dtype == np.float32 and oh.shape == (1, 4, 3) and np.array_equal(donors.hard_codes(oh), gt)
    assert oh[0, :3].tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 1]] and np.isnan(oh[0, 3]).all()
    w, kind = donors.soft_weights(gp, np.arange(6))
    assert kind[:, 0].tolist() == [4, 4, 4, 3, 2, 0] and w[4, 0].tolist() == [0, 0, 1] and w[5, 0].tolist() == [1, 0, 0] and (w[3] == 0).all()
    assert w[1, 0].tolist() == [0.5, 0.5, 0.0]
    for row in ((0.5, nan, 0.5), (0.5, -0.25, 0.75), (0, 0, 0), (np.inf, 0, 0)):
        bad = gp.copy()
        bad[0, 2] = row
        with pytest.raises(ValueError, match="donor 0 at locus 2"):
            donors.soft_weights(bad, np.arange(6))


VARIANTS = """##fileformat=VCFv4.2
#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO
chr1\t100\t.\tA\tG\t.\t.\t.
chr1\t200\t.\tC\tT\t.\t.\t.
chr1\t300\t.\tG\tA\t.\t.\t.
chr2\t100\t.\tT\tC\t.\t.\t.
chr2\t150\t.\tA\tC\t.\t.\t.
chr2\t900\t.\tG\tT\t.\t.\t.
chr3\t5\t.\tC\tG\t.\t.\t.
chr3\t9\t.\tC\tG\t.\t.\t.
"""
DONORS = """##fileformat=VCFv4.2
#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\talice\tbob\tcarol
chr1\t100\t.\tA\tG\t.\tPASS\t.\tGT:GP:GL:PL\t0/0:0.9,0.1,0:-0.1,-1.5,-7:0,14,70\t0|1:0.05,0.6,0.35:-3,-0.2,-0.5:30,0,5\t1|1:0,0,1:-9,-4,0:90,40,0
chr1\t200\t.\tT\tC\t.\tPASS\t.\tGT:GP:GL:PL\t0/0:0.7,0.2,0.1:0,-1,-2:0,10,20\t1|0:1e-3,.5,2.:-2.5,-0.25,-1e1:25,3,100\t1/1:0.25,0.25,0.5:-1,-1,0:10,10,0
chr1\t300\t.\tG\tA\t.\tPASS\t.\tGP:GT:GL:PL\t.:0/1:.:.\t0.3,0.7:1/1:-1,-2:1,2\t0.5,-0.1,0.6:./.:-1,nan,0:3,-4,0
chr2\t100\t.\tT\tC\t.\tPASS\t.\tGT\t0/1\t1/1\t./.
chr2\t777\t.\tA\tC\t.\tPASS\t.\tGT:GP\t1/1:0,0,1\t1/1:0,0,1\t1/1:0,0,1
chr2\t900\t.\tG\tT\t.\tPASS\t.\tGP:GL:PL\t0,0,0\tinf,0,0\t0.2,0.2,0.2,0.4
chr3\t5\t.\tC\tG\t.\tPASS\t.\tGT:GP:GL:PL\t1/1:0.1,0.2,0.7:-5,-1,0:50,10,0\t0/1:0.2,0.7,0.1:-1,0,-3:10,0,30
chr3\t9\t.\tC\tG\t.\tPASS\t.\tGT:GP:GL:PL\t0/0:1e999,0,0:-1e999,0,0:0,1_0,2\t0/1:0x1,0,0:-0x1,0,0:0x0,1,2\t1/1: 1,0,0:+1,-1,0:+0,+10,+20
"""
NAN3 = [np.nan] * 3


def _want(field):
    """[locus][donor] rows, in double: what the rule of read_donor_vcf_gp gives for DONORS"""
    gl = lambda *v: [10.0 ** (x - max(v)) for x in v]
    pl = lambda *v: [10.0 ** (-(x - min(v)) / 10.0) for x in v]
    A, B, C = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
    per = {
        "GP": [[(0.9, 0.1, 0.0), (0.05, 0.6, 0.35), (0.0, 0.0, 1.0)],
               [(0.1, 0.2, 0.7), (2.0, 0.5, 1e-3), (0.5, 0.25, 0.25)],  # ref and alt swapped: reversed
               [B, C, NAN3],                                            # '.', two values, a negative value: GT, GT, no call
               [B, C, NAN3],                                            # no GP in the record: GT
               [NAN3, NAN3, NAN3],                                      # no donor record
               [NAN3, NAN3, NAN3],                                      # three zeros, inf, four values; no GT
               [(0.1, 0.2, 0.7), (0.2, 0.7, 0.1), NAN3],                # a sample column missing
               [A, B, C]],                                              # 1e999, a hex number, a leading blank: GT
        "GL": [[gl(-0.1, -1.5, -7), gl(-3, -0.2, -0.5), gl(-9, -4, 0)],
               [gl(-2, -1, 0), gl(-10, -0.25, -2.5), gl(0, -1, -1)],
               [B, C, NAN3],
               [B, C, NAN3],
               [NAN3, NAN3, NAN3],
               [NAN3, NAN3, NAN3],
               [gl(-5, -1, 0), gl(-1, 0, -3), NAN3],
               [A, B, gl(1, -1, 0)]],
        "PL": [[pl(0, 14, 70), pl(30, 0, 5), pl(90, 40, 0)],
               [pl(20, 10, 0), pl(100, 3, 25), pl(0, 10, 10)],
               [B, C, NAN3],
               [B, C, NAN3],
               [NAN3, NAN3, NAN3],
               [NAN3, NAN3, NAN3],
               [pl(50, 10, 0), pl(10, 0, 30), NAN3],
               [A, B, pl(0, 10, 20)]],
    }
    return np.array(per[field], np.float64).transpose(1, 0, 2)


def _files(tmp_path, gz):
    v, d = tmp_path / "variants.vcf", tmp_path / ("donors.vcf.gz" if gz else "donors.vcf")
    v.write_text(VARIANTS)
    if gz:
        with gzip.open(d, "wt") as f:
            f.write(DONORS)
    else:
        d.write_text(DONORS)
    return str(v), str(d)


@pytest.mark.parametrize("gz", [False, True], ids=["plain", "gzip"])
@pytest.mark.parametrize("field", ["GP", "GL", "PL"])
def test_read_donor_vcf_gp(tmp_path, field, gz):
    v, d = _files(tmp_path, gz)
    names, gp = donors.read_donor_vcf_gp(d, v, field)
    assert names == ["alice", "bob", "carol"] and gp.dtype == np.float32 and gp.shape == (3, 8, 3)
    want = _want(field).astype(np.float32)
    assert gp.tobytes() == want.tobytes(), (gp, want)
    donors.soft_weights(gp, np.arange(8))  # every row is one the library takes
    _, gt = donors.read_donor_vcf(d, v)  # the hard reader is as it was: GT alone
    assert gt[:, 0].tolist() == [0, 1, 2] and gt[:, 2].tolist() == [1, 2, 3] and gt[:, 5].tolist() == [3, 3, 3]
    with pytest.raises(ValueError, match="field"):
        donors.read_donor_vcf_gp(d, v, "GQ")


DRIVER = r"""
#include <cstdio>
#include <fstream>
#include <string>
#include "donor_vcf_host.h"

// argv: variant vcf, donor vcf (plain text), field.  Prints the names, then per donor one line of %a weights and one of hard codes.
int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    DonorGenotypes dg;
    dg.field = argv[3];
    std::string line;
    std::ifstream v(argv[1]), d(argv[2]);
    while (std::getline(v, line)) dg.add_variant_line(line);
    while (std::getline(d, line)) dg.add_donor_line(line);
    for (const std::string &n : dg.names) printf("%s ", n.c_str());
    printf("\n");
    const std::vector<uint8_t> hard = donor_hard_codes(dg.gp);
    for (size_t k = 0; k < dg.names.size(); k++) {
        for (uint64_t t = 0; t < dg.total_loci * 3; t++) printf("%a ", (double)dg.gp[k * dg.total_loci * 3 + t]);
        printf("\n");
        for (uint64_t t = 0; t < dg.total_loci; t++) printf("%d%d", (int)hard[k * dg.total_loci + t], (int)dg.gt[k * dg.total_loci + t]);
        printf("\n");
    }
    return 0;
}
"""


def test_the_cli_header_reads_what_the_python_reader_reads(tmp_path):
    """csrc/donor_vcf_host.h compiled as plain C++ on the host: GP exactly, GL and PL within one float ulp (two pow of two libraries)"""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    if not cxx:
        pytest.fail("no host C++ compiler")
    src, exe = tmp_path / "driver.cpp", tmp_path / "driver"
    src.write_text(DRIVER)
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "cellector_amd", "csrc"), str(src), "-o", str(exe)])
    v, d = _files(tmp_path, False)
    _, gt = donors.read_donor_vcf(d, v)
    for field in ("GP", "GL", "PL"):
        out = subprocess.run([str(exe), v, d, field], capture_output=True, text=True, check=True).stdout.splitlines()
        names, gp = donors.read_donor_vcf_gp(d, v, field)
        assert out[0].split() == names
        got = np.array([[float.fromhex(x) if "nan" not in x else np.nan for x in out[1 + 2 * k].split()] for k in range(3)]).reshape(3, 8, 3)
        got = got.astype(np.float32)
        assert np.array_equal(np.isnan(got), np.isnan(gp))
        if field == "GP":
            assert got.tobytes() == gp.tobytes()
        else:
            ok = ~np.isnan(gp)
            assert (np.abs(got[ok].astype(np.float64) - gp[ok].astype(np.float64)) <= np.spacing(gp[ok]).astype(np.float64)).all()
        hard = donors.hard_codes(got)
        for k in range(3):
            assert out[2 + 2 * k] == "".join(f"{int(h)}{int(g)}" for h, g in zip(hard[k], gt[k]))


def test_donor_field_usage_errors_and_help(host_bin, tmp_path):
    base = [host_bin, "-a", "a.mtx", "-r", "r.mtx", "--barcodes", "b.tsv", "--output_directory", str(tmp_path / "o")]
    r = subprocess.run(base + ["--vcf", "v.vcf", "--donor_field", "GP"], capture_output=True, text=True)
    assert r.returncode == 1 and "'--donor_field <GT|GP|GL|PL>' requires '--donors <vcf>'" in r.stderr
    for bad in ("GQ", "gp", ""):
        r = subprocess.run(base + ["--vcf", "v.vcf", "--donors", "d.vcf", "--donor_field", bad], capture_output=True, text=True)
        assert r.returncode == 1 and "for '--donor_field <GT|GP|GL|PL>': expected GT, GP, GL or PL" in r.stderr, bad
    assert not os.path.exists(tmp_path / "o")
    r = subprocess.run([host_bin, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--donor_field <GT|GP|GL|PL>" in r.stdout
    for word in ("10^(GL - max GL)", "10^(-(PL - min PL) / 10)", "falls back to its", "the soft ambient profile", "With GT no output changes"):
        assert word in r.stdout, word
