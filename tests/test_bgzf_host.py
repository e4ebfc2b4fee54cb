"""CPU: the C side of the BGZF writer's format (csrc/bgzf_format.h) against the numpy twin.  tests/bgzf_host_main.cpp is a stand-alone
program around bgzf_encode_block_host; it is built here with the address and undefined-behaviour sanitizers and run as a program over
every input of tests/bgzf_cases.py: its stream must be the twin's bytes, its block counts the twin's, its preset the twin's, and the
sanitizers must stay silent (a report makes the program exit non-zero)."""
import os
import shutil
import subprocess

import pytest

import bgzf_cases
from cellector_amd import bgzf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(bgzf_cases.cases())


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path_factory.mktemp("bgzf_host") / "bgzf_host_main"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           os.path.join(ROOT, "tests", "bgzf_host_main.cpp"), "-o", str(exe)])
    return str(exe)


def _run(program, *args):
    r = subprocess.run([program, *args], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    return r.stdout


def test_preset_arrays_are_the_twins(program):
    lines = dict(l.split(" ", 1) for l in _run(program, "preset").splitlines())
    p = bgzf.preset()
    assert [int(x) for x in lines["litlen"].split()] == p["litlen"]
    assert [int(x) for x in lines["dist"].split()] == p["dist"]
    assert int(lines["header_bits"]) == p["header_bits"] and bytes.fromhex(lines["header"]) == p["header"]


@pytest.mark.parametrize("name", NAMES)
def test_host_stream_is_the_twins(program, tmp_path, name):
    src, dst = tmp_path / "in", tmp_path / "out"
    src.write_bytes(bgzf_cases.cases()[name])
    out = _run(program, "compress", str(src), str(dst))
    stream, stats = bgzf_cases.expected(name)
    assert dst.read_bytes() == stream
    assert out.split() == ["blocks", str(stats["blocks"]), "stored_blocks", str(stats["stored_blocks"])]
