"""`host/cellector --normalization <per_locus|zscore>`: argument handling (exits before any GPU call)."""
import subprocess

from test_host_cli import host_bin  # noqa: F401

BASE = ["-a", "a", "-r", "r", "-b", "b", "--output_directory", "o"]


def test_bad_value_names_the_flag_and_the_legal_values(host_bin):
    r = subprocess.run([host_bin] + BASE + ["--normalization", "bogus"], capture_output=True, text=True)
    assert r.returncode == 101  # the way --resolve_near_ties dies for a bad value
    assert "--normalization" in r.stderr and "bogus" in r.stderr and "per_locus" in r.stderr and "zscore" in r.stderr


def test_zscore_refuses_the_resolve_flags(host_bin):
    for extra, named in ((["--resolve_near_ties", "true"], "--resolve_near_ties true"),
                         (["--resolve_assignments", "true"], "--resolve_assignments true"),
                         (["--resolve_assignments", "all"], "--resolve_assignments all")):
        for args in (["--normalization", "zscore"] + extra, extra + ["--normalization=zscore"]):
            r = subprocess.run([host_bin] + BASE + args, capture_output=True, text=True)
            assert r.returncode == 1 and r.stderr.startswith("error:"), (args, r.stderr)
            assert "--normalization zscore" in r.stderr and named in r.stderr, (args, r.stderr)
    # per_locus goes with them: the run gets as far as opening its input files
    r = subprocess.run([host_bin] + BASE + ["--normalization", "per_locus", "--resolve_near_ties", "false"], capture_output=True, text=True)
    assert "--normalization" not in r.stderr


def test_help_lists_the_flag(host_bin):
    r = subprocess.run([host_bin, "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and "--normalization <per_locus|zscore>" in r.stdout
    r = subprocess.run([host_bin] + BASE + ["--normalization"], capture_output=True, text=True)
    assert r.returncode != 0 and "requires a value" in r.stderr
