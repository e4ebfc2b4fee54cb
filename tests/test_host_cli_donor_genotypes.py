"""CPU: the host binary's usage errors and help text for --donor_genotypes (no GPU is opened: the refusals come first)."""
import os
import subprocess

from test_host_cli import host_bin  # noqa: F401


def test_donor_genotypes_usage_errors_and_help(host_bin, tmp_path):
    base = [host_bin, "-a", "a.mtx", "-r", "r.mtx", "--barcodes", "b.tsv", "--output_directory", str(tmp_path / "o")]
    for word in ("true", "apply"):
        r = subprocess.run(base + ["--vcf", "v.vcf", "--donor_genotypes", word], capture_output=True, text=True)
        assert r.returncode == 1 and "'--donor_genotypes <true|apply>' requires '--donors <vcf>'" in r.stderr, word
    for word in ("maybe", "TRUE", "1"):
        r = subprocess.run(base + ["--vcf", "v.vcf", "--donors", "d.vcf", "--donor_genotypes", word], capture_output=True, text=True)
        assert r.returncode != 0 and "expected true, apply or false" in r.stderr and f"'{word}'" in r.stderr, word
    assert not os.path.exists(tmp_path / "o")
    r = subprocess.run([host_bin, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--donor_genotypes <true|apply>" in r.stdout
    for word in ("cellector_donor_genotypes.vcf", "cellector_donor_genotypes.tsv", "GT:GP:AO:RO", "loci_with_reads", "confirmed, filled, changed, withdrawn",
                 "--estimate_ambient apply", "floored at 0.01", "true: no other output changes", "apply: the"):
        assert word in r.stdout, word
