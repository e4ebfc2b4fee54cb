"""CPU: the donor calls' C ABI as the binding sees it (signatures, struct sizes, defaults) and donors.read_donor_vcf on hand-written
VCFs: phased calls, swapped alleles, missing calls, a third allele, records the variant VCF does not have."""
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


def _prototype(name):
    text = open(os.path.join(ROOT, "include", "cellector_ffi.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"cellector_status\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name, n_args", [("cellector_donor_default_params", 1), ("cellector_donor_tables", 8),
                                          ("cellector_donor_posteriors", 21), ("cellector_match_donors", 11)])
def test_signatures_follow_the_header(hip_lib_path, name, n_args):
    args = _prototype(name)
    res, argtypes = ffi.SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == len(argtypes) == n_args
    for a, t in zip(args, argtypes):
        want = ctypes.c_void_p if "*" in a else ctypes.c_uint32 if a.startswith("uint32_t") else None
        assert t is want, (name, a, t)
    assert hasattr(ffi.load_library(hip_lib_path), name)


def test_struct_layouts_and_defaults(hip_lib_path):
    assert ctypes.sizeof(ffi.DonorParams) == 40 and ffi.DonorParams.min_loci.offset == 32
    assert ctypes.sizeof(ffi.DonorSummary) == 4 * 8 + 64 * 8 and ffi.DonorSummary.donor_cells.offset == 32
    lib = ffi.load_library(hip_lib_path)
    p = ffi.DonorParams()
    assert lib.cellector_donor_default_params(ctypes.byref(p)) == 0
    assert {k: getattr(p, k) for k, _ in ffi.DonorParams._fields_} == donors.DEFAULTS
    assert lib.cellector_donor_default_params(None) == 1
    assert lib.cellector_donor_tables(None, None, 1, None, None, None, None, None) == 1  # (a null ctx)
    for name in ("donor_posteriors", "donor_tables", "match_donors", "donor_default_params"):
        assert callable(getattr(ffi.Cellector, name))


VARIANTS = """##fileformat=VCFv4.2
#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO
chr1\t100\t.\tA\tG\t.\t.\t.
chr1\t200\t.\tC\tT\t.\t.\t.
chr1\t300\t.\tG\tA\t.\t.\t.
chr2\t100\t.\tT\tC\t.\t.\t.
chr2\t150\t.\tA\tC\t.\t.\t.
chr2\t900\t.\tG\tT\t.\t.\t.
chr3\t5\t.\tC\tG\t.\t.\t.
"""
DONORS = """##fileformat=VCFv4.2
##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">
#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\talice\tbob\tcarol
chr1\t100\t.\tA\tG\t.\tPASS\t.\tGT\t0/0\t0|1\t1|1
chr1\t200\t.\tT\tC\t.\tPASS\t.\tGT:DP\t0/0:9\t1|0:3\t1/1:2
chr1\t300\t.\tG\tA\t.\tPASS\t.\tDP:GT\t4:./.\t7:.\t1:0/.
chr2\t100\t.\tT\tC,G\t.\tPASS\t.\tGT\t0/1\t1/2\t0/0
chr2\t100\t.\tT\tC\t.\tPASS\t.\tGT\t1/0\t0/2\t0/0/1
chr2\t777\t.\tA\tC\t.\tPASS\t.\tGT\t1/1\t1/1\t1/1
chr2\t900\t.\tG\tT\t.\tPASS\t.\tDP\t3\t4\t5
chr3\t5\t.\tC\tG\t.\tPASS\t.\tGT\t1/1\t0/1
"""


@pytest.mark.parametrize("gz", [False, True], ids=["plain", "gzip"])
def test_read_donor_vcf(tmp_path, gz):
    v, d = tmp_path / "variants.vcf", tmp_path / ("donors.vcf.gz" if gz else "donors.vcf")
    v.write_text(VARIANTS)
    if gz:
        with gzip.open(d, "wt") as f:
            f.write(DONORS)
    else:
        d.write_text(DONORS)
    names, gt = donors.read_donor_vcf(str(d), str(v))
    assert names == ["alice", "bob", "carol"]
    assert gt.dtype == np.uint8 and gt.shape == (3, 7)
    want = np.array([
        [0, 1, 2],  # chr1:100 as it is, phased or not
        [2, 1, 0],  # chr1:200 with ref and alt swapped: the calls mirrored
        [3, 3, 3],  # chr1:300 ./., ., a half call
        [1, 3, 3],  # chr2:100 the biallelic record counts (the multi-allelic one matches no variant); 0/2 and a triploid call: none
        [3, 3, 3],  # chr2:150 no donor record (chr2:777 is not a variant)
        [3, 3, 3],  # chr2:900 a record without GT
        [2, 1, 3],  # chr3:5   a sample column short
    ], np.uint8).T
    assert np.array_equal(gt, want), gt.T


DRIVER = r"""
#include <cstdio>
#include <fstream>
#include <string>
#include "donor_vcf_host.h"

// argv: variant vcf, donor vcf (plain text).  Prints the names, then one line of calls per donor.
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    DonorGenotypes dg;
    std::string line;
    std::ifstream v(argv[1]), d(argv[2]);
    while (std::getline(v, line)) dg.add_variant_line(line);
    while (std::getline(d, line)) dg.add_donor_line(line);
    for (const std::string &n : dg.names) printf("%s ", n.c_str());
    printf("\n");
    for (size_t k = 0; k < dg.names.size(); k++) {
        for (uint64_t t = 0; t < dg.total_loci; t++) printf("%d", (int)dg.gt[k * dg.total_loci + t]);
        printf("\n");
    }
    return 0;
}
"""


def test_the_cli_header_reads_what_the_python_reader_reads(tmp_path):
    """csrc/donor_vcf_host.h, the CLI's reader, compiled as plain C++ on the host"""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    if not cxx:
        pytest.fail("no host C++ compiler")
    src, exe = tmp_path / "driver.cpp", tmp_path / "driver"
    src.write_text(DRIVER)
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "cellector_amd", "csrc"), str(src), "-o", str(exe)])
    v, d = tmp_path / "variants.vcf", tmp_path / "donors.vcf"
    v.write_text(VARIANTS)
    d.write_text(DONORS)
    out = subprocess.run([str(exe), str(v), str(d)], capture_output=True, text=True, check=True).stdout.splitlines()
    names, gt = donors.read_donor_vcf(str(d), str(v))
    assert out[0].split() == names
    assert out[1:] == ["".join(str(int(x)) for x in row) for row in gt]


def test_donors_without_vcf_is_a_usage_error(host_bin, tmp_path):
    BIN = host_bin
    r = subprocess.run([BIN, "-a", "a.mtx", "-r", "r.mtx", "--barcodes", "b.tsv", "--output_directory", str(tmp_path / "o"), "--donors", "d.vcf"],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "'--donors <vcf>' requires '--vcf <vcf>'" in r.stderr
    assert not os.path.exists(tmp_path / "o")
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True)
    for flag in ("--donors <vcf>", "--donor_error", "--donor_ambient", "--donor_doublet_rate"):
        assert flag in r.stdout, flag


def test_parse_gt():
    for field, want in (("0/0", 0), ("0|1", 1), ("1/0", 1), ("1|1", 2), ("./.", 3), (".", 3), ("0/2", 3), ("1", 3), ("0/1/1", 3), ("", 3)):
        assert donors.parse_gt(field) == want, field
    assert donors.parse_gt("7:1/1", 1) == 2 and donors.parse_gt("7:1/1", 2) == 3 and donors.parse_gt("1/1", -1) == 3
