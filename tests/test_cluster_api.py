"""CPU: the clustering calls are declared, exported and bound with the header's argument names; the header states the model; the
default parameters; a null ctx is refused; no kernel id was added."""
import ctypes
import os
import re

from cellector_amd import cluster as cl
from cellector_amd import ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "cellector_ffi.h")).read()

ARGS = {
    "cellector_cluster_default_params": ["out"],
    "cellector_cluster": ["ctx", "n_clusters", "n_restarts", "seed", "p", "mask", "labels", "ll", "posterior", "theta", "objective", "out"],
    "cellector_cluster_m_step": ["ctx", "w", "J", "mask", "theta_floor", "A", "T", "theta", "tab"],
    "cellector_cluster_e_step": ["ctx", "tab", "K", "R", "temp", "mask", "s", "w", "objective"],
}


def _declared_args(name):
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    m = re.search(r"cellector_status\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared"
    return [re.findall(r"[A-Za-z_][A-Za-z_0-9]*", a)[-1] for a in m.group(1).split(",")]


def test_declared_exported_and_bound(hip_lib_path):
    lib = ffi.load_library(hip_lib_path)
    for name, args in ARGS.items():
        assert _declared_args(name) == args, name
        assert hasattr(lib, name) and len(ffi.SIGNATURES[name][1]) == len(args), name
    for m in ("cluster", "cluster_m_step", "cluster_e_step", "cluster_default_params"):
        assert callable(getattr(ffi.Cellector, m))
    # behind the class-genotypes block, in front of what followed it
    at = [HEADER.index(s) for s in ("cellector_status cellector_class_genotypes(", "cellector_status cellector_cluster_default_params(",
                                    "cellector_status cellector_cluster(", "cellector_status cellector_cluster_m_step(",
                                    "cellector_status cellector_cluster_e_step(", "cellector_status cellector_final_allele_tallies(")]
    assert at == sorted(at)
    assert re.search(r"CELLECTOR_K_COUNT\s*=\s*7\b", HEADER)


def test_struct_layouts_and_defaults(hip_lib_path):
    lib = ffi.load_library(hip_lib_path)
    assert ctypes.sizeof(ffi.ClusterParams) == 40 and ffi.ClusterParams.min_loci.offset == 32
    assert ctypes.sizeof(ffi.ClusterSummary) == 16 + 64 + 128 + 8
    assert ffi.ClusterSummary.iterations_per_stage.offset == 16 and ffi.ClusterSummary.cluster_cells.offset == 80
    p = ffi.ClusterParams()
    assert lib.cellector_cluster_default_params(ctypes.byref(p)) == 0
    got = dict(theta_floor=p.theta_floor, anneal_base=p.anneal_base, tol=p.tol, anneal_steps=p.anneal_steps, max_iter=p.max_iter,
               min_loci=p.min_loci)
    assert got == dict(theta_floor=0.01, anneal_base=20.0, tol=0.01, anneal_steps=9, max_iter=50, min_loci=1) == cl.DEFAULTS
    assert lib.cellector_cluster_default_params(None) == 1


def test_null_ctx_is_refused(hip_lib_path):
    lib = ffi.load_library(hip_lib_path)
    assert lib.cellector_cluster(None, 3, 4, 1, None, None, None, None, None, None, None, None) == 1
    assert lib.cellector_cluster_m_step(None, None, 3, None, 0.01, None, None, None, None) == 1
    assert lib.cellector_cluster_e_step(None, None, 3, 1, None, None, None, None, None) == 1


def test_header_states_the_model():
    beg = HEADER.index("genotype clusters without labels")
    block = HEADER[beg:HEADER.index("cellector_status cellector_cluster_default_params(")]
    for word in ("theta_floor", "anneal", "ascending cell", "row order", "255", "CELLECTOR_ENOMEM", "mix64", "max_iter", "min_loci"):
        assert word in block, word
