"""GPU: `host/cellector --gz_device true` on a block-compressed pair: the run inflates -a / -r (and --mix_alt / --mix_ref) on the GPU
and writes every output file byte for byte as the run without the flag does, under --matrix_pair aligned and join; `--gz_device
false` is the run without the flag; another word is a usage error.  The case is tests/test_gpu_cli_combine.py's."""
import os

import pytest

from cellector_amd import synth
from test_gpu_cli_combine import _run, inputs  # noqa: F401
from test_host_cli import host_bin  # noqa: F401


@pytest.fixture(scope="module")
def gz_inputs(inputs, tmp_path_factory):  # noqa: F811
    """the two datasets' pairs as BGZF files of small blocks beside the plain ones"""
    tmp = tmp_path_factory.mktemp("cli_gz_device")
    out = {}
    for key in ("first", "second"):
        alt, ref, bc = inputs[key]
        paths = []
        for name, src in (("alt", alt), ("ref", ref)):
            p = str(tmp / ("%s_%s.mtx.gz" % (key, name)))
            with open(p, "wb") as f:
                f.write(synth.bgzf_compress(open(src, "rb").read(), block=4000 if name == "alt" else 0xff00))
            paths.append(p)
        out[key] = (paths[0], paths[1], bc)
    return out


def _outputs(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [[], ["--matrix_pair", "join"], ["mix"]], ids=["aligned", "join", "mix"])
def test_outputs_do_not_depend_on_the_flag(host_bin, inputs, gz_inputs, tmp_path, extra):  # noqa: F811
    alt, ref, bc = gz_inputs["first"]
    if extra == ["mix"]:
        alt2, ref2, bc2 = gz_inputs["second"]
        extra = ["--mix_alt", alt2, "--mix_ref", ref2, "--mix_barcodes", bc2]
    runs = {}
    for key, flag in (("none", []), ("false", ["--gz_device", "false"]), ("true", ["--gz_device", "true"])):
        o = str(tmp_path / key)
        r = _run(host_bin, alt, ref, bc, inputs["vcf"], o, *extra, *flag)
        assert r.returncode == 0, r.stderr
        runs[key] = (_outputs(o), r.stdout)
    assert runs["none"][0] and runs["false"] == runs["none"]
    assert runs["true"][0].keys() == runs["none"][0].keys()
    for f, data in runs["none"][0].items():
        assert runs["true"][0][f] == data, f
    assert runs["true"][1] == runs["none"][1]


@pytest.mark.gpu
def test_usage_error(host_bin, inputs, gz_inputs, tmp_path):  # noqa: F811
    alt, ref, bc = gz_inputs["first"]
    r = _run(host_bin, alt, ref, bc, inputs["vcf"], str(tmp_path / "o"), "--gz_device", "maybe")
    assert r.returncode != 0 and "gz_device" in r.stderr and "expected true or false" in r.stderr
