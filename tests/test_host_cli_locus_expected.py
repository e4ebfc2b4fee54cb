"""`host/cellector --locus_expected <true|false>`: argument handling (exits before any GPU call)."""
import subprocess

from test_host_cli import host_bin  # noqa: F401

BASE = ["-a", "a", "-r", "r", "-b", "b", "--output_directory", "o"]


def test_bad_value_names_the_flag_and_the_legal_values(host_bin):
    r = subprocess.run([host_bin] + BASE + ["--locus_expected", "bogus"], capture_output=True, text=True)
    assert r.returncode == 101  # the way --normalization dies for a bad value
    assert "--locus_expected" in r.stderr and "bogus" in r.stderr and "true" in r.stderr and "false" in r.stderr


def test_true_refuses_devices(host_bin):
    for devices in ("0,1", "auto", "0,0"):
        for args in (["--locus_expected", "true", "--devices", devices], ["--devices=" + devices, "--locus_expected=true"]):
            r = subprocess.run([host_bin] + BASE + args, capture_output=True, text=True)
            assert r.returncode == 1 and r.stderr.startswith("error:"), (args, r.stderr)
            assert "--locus_expected true" in r.stderr and "--devices" in r.stderr and "one GPU" in r.stderr, (args, r.stderr)
    # false goes with them, and true with one device: the run gets as far as opening its input files
    for args in (["--locus_expected", "false", "--devices", "0,1"], ["--locus_expected", "true", "--device", "0"]):
        r = subprocess.run([host_bin] + BASE + args, capture_output=True, text=True)
        assert "--locus_expected" not in r.stderr, (args, r.stderr)


def test_help_lists_the_flag(host_bin):
    r = subprocess.run([host_bin, "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and "--locus_expected <true|false>" in r.stdout
    for col in ("variance_minority", "zscore_majority"):
        assert col in r.stdout
    r = subprocess.run([host_bin] + BASE + ["--locus_expected"], capture_output=True, text=True)
    assert r.returncode != 0 and "requires a value" in r.stderr
