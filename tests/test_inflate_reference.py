"""CPU: the shared DEFLATE decoder (csrc/inflate_format.h) against zlib.  tests/inflate_host_main.cpp is a stand-alone program around
inflate_member_host; it is built here with the address and undefined-behaviour sanitizers and run as a program over the streams of
tests/inflate_cases.py.  The rule for every stream: the program refuses it exactly when inflate_cases.reference does (zlib raises or
leaves input unused, or the length or the CRC-32 is not the trailer's); when it accepts, the bytes are the reference's; the
sanitizers stay silent (a report makes the program exit non-zero and write to stderr).

Mutations the reference itself refuses, of 200 per member (the test asks for 150): text_level6 200, fixed 200, stored 200, rle 200,
full_flush 200."""
import os
import shutil
import subprocess

import pytest

import inflate_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path_factory.mktemp("inflate_host") / "inflate_host_main"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           os.path.join(ROOT, "tests", "inflate_host_main.cpp"), "-o", str(exe)])
    return str(exe)


def _check(program, tmp_path, names):
    """runs the program over the cases; returns how many the reference refuses"""
    src, dst = tmp_path / "in", tmp_path / "out"
    src.write_bytes(ic.records(names))
    r = subprocess.run([program, str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(names)
    got, at, refused = dst.read_bytes(), 0, 0
    for name, line in zip(names, lines):
        status, produced = (int(x) for x in line.split())
        body, isize, crc = ic.all_cases()[name]
        want = ic.reference(body, isize, crc)
        assert (status != 0) == (want is None), (name, status, produced)
        assert produced <= isize, name
        if want is None:
            refused += 1
            continue
        assert got[at:at + isize] == want, name
        at += isize
    assert at == len(got)
    return refused


def test_cases_are_what_they_claim():
    for name, (body, isize, crc, accepted) in ic.hand_cases().items():
        assert (ic.reference(body, isize, crc) is not None) == accepted, name
    for name, m in list(ic.zlib_cases().items()) + list(ic.library_cases().items()):
        assert ic.reference(*m) is not None, name
    z = ic.zlib_cases()
    assert len(z["random_two_stored"][0]) == ic.TEXT + 10 and len(z["empty"][0]) == 2 and len(z["one_byte"][0]) == 3
    assert z["stored"][0][:1] == b"\x01" and z["fixed"][0][0] & 7 == 3   # final stored; final fixed


def test_streams_made_with_zlib(program, tmp_path):
    assert _check(program, tmp_path, sorted(ic.zlib_cases())) == 0


def test_the_librarys_own_streams(program, tmp_path):
    assert _check(program, tmp_path, sorted(ic.library_cases())) == 0


def test_hand_made_streams(program, tmp_path):
    h = ic.hand_cases()
    assert _check(program, tmp_path, sorted(h)) == sum(1 for v in h.values() if not v[3])


@pytest.mark.parametrize("name", ic.MUTATED)
def test_mutations(program, tmp_path, name):
    names = sorted(k for k in ic.mutation_cases() if k.rsplit("_", 1)[0] == "mut_" + name)
    assert len(names) == 200
    refused = _check(program, tmp_path, names)
    print(name, "refused by the reference:", refused)
    assert refused >= 150
