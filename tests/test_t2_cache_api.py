"""Options t2_cache and t2_fill: in the option table of cellector_set_option with their ranges, defaults of -1, documented in the
header with their neighbours (no GPU needed: a ctx cannot be made without a device, so the table is read from the source and a
null ctx is tried against the built library)."""
import os
import re

from cellector_amd import ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cellector_amd", "csrc")


def _read(*parts):
    return open(os.path.join(*parts)).read()


def _branch(key):
    """the branch of cellector_set_option's table that takes `key`"""
    table = _read(CSRC, "api_options.cpp")
    m = re.search(r'else if \(!strcmp\(key, "' + key + r'"\)\) \{(.*?)\n    \}', table, flags=re.S)
    assert m, f'option "{key}" is not in the table'
    return m.group(1)


def test_accepted_and_refused_like_its_neighbours():
    for key in ("t2_cache", "t2_fill"):
        body = _branch(key)
        # -1, 0 and 1 pass; everything else is an argument error with the reason, like t2 and ovf_deep beside it
        assert "v < -1 || v > 1" in body and "CELLECTOR_EINVAL" in body and f"{key} must be -1" in body
        assert f"c->{key} = (int)v;" in body
    assert "v < -1 || v > 1" in _branch("t2")  # the neighbour it is modelled on


def test_the_default_is_minus_one():
    ctx = _read(CSRC, "ctx.h")
    for key in ("t2_cache", "t2_fill"):
        m = re.search(r"int " + key + r" = (-?\d+);\s*// option \"" + key + '"', ctx)
        assert m and int(m.group(1)) == -1, key


def test_documented_with_the_other_options():
    options = _read(ROOT, "include", "cellector_ffi.h").split("cellector_status cellector_set_option", 1)[0]
    assert '"t2_helper"' in options
    tail = options.split('"t2_helper"', 1)[1]
    for word in ('"t2_cache"', '"t2_fill"', "-1 = automatic", "same bits either way"):
        assert word in tail, word
    assert "`t2_cache`" in _read(ROOT, "README.md")


def test_a_null_ctx_is_an_argument_error(hip_lib_path):
    lib = ffi.load_library(hip_lib_path)
    assert lib.cellector_set_option(None, b"t2_cache", 1) == 1
