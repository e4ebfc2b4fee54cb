"""`host/cellector --class_genotypes <true|false>`: argument handling (exits before any GPU call)."""
import subprocess

from test_host_cli import host_bin  # noqa: F401

BASE = ["-a", "a", "-r", "r", "-b", "b", "--output_directory", "o"]


def test_bad_value_is_refused_like_class_doublets(host_bin):
    r = subprocess.run([host_bin] + BASE + ["--classes", "c", "--vcf", "v", "--class_genotypes", "bogus"], capture_output=True, text=True)
    d = subprocess.run([host_bin] + BASE + ["--classes", "c", "--class_doublets", "bogus"], capture_output=True, text=True)
    assert r.returncode == d.returncode == 101
    assert r.stderr == d.stderr.replace("--class_doublets", "--class_genotypes")


def test_the_flag_requires_classes_and_vcf(host_bin):
    r = subprocess.run([host_bin] + BASE + ["--vcf", "v", "--class_genotypes", "true"], capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.strip() == "error: The argument '--class_genotypes true' requires '--classes <file>'"
    r = subprocess.run([host_bin] + BASE + ["--classes", "c", "--class_genotypes", "true"], capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.strip() == "error: The argument '--class_genotypes true' requires '--vcf <vcf>'"
    # false asks for neither: the run gets as far as opening its input files
    r = subprocess.run([host_bin] + BASE + ["--class_genotypes", "false"], capture_output=True, text=True)
    assert "--class_genotypes" not in r.stderr


def test_true_refuses_devices(host_bin):
    for devices in ("0,1", "auto"):
        r = subprocess.run([host_bin] + BASE + ["--classes", "c", "--vcf", "v", "--class_genotypes", "true", "--devices", devices],
                           capture_output=True, text=True)
        assert r.returncode == 1 and r.stderr.startswith("error:"), r.stderr
        assert "--class_genotypes true" in r.stderr and "--devices" in r.stderr and "one GPU" in r.stderr, r.stderr


def test_help_lists_the_flag(host_bin):
    r = subprocess.run([host_bin, "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and "--class_genotypes <true|false>" in r.stdout
    assert "cellector_classes.vcf" in r.stdout and "cellector_class_concordance.tsv" in r.stdout
