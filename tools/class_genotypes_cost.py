#!/usr/bin/env python3
"""Cost of the class genotypes on a resident matrix (needs an MI355X): K = 3 with the labelling of tools/classes_cost.py (the
synthetic minority as class 1, a random 1 % of the cells as class 2, the rest class 0), and K = 16 with random labels.

  python tools/class_genotypes_cost.py [--cfg cfg4] [--reps 5] [--parent-lib PATH/libcellector_hip.so] [--out profiles/NAME.json]

Measured per K, best of --reps wall times of the calls (each ends synchronised):
  tally_pass       cellector_class_genotypes with no output asked for: the 1 B per cell of labels in, the memset of the (K + 1) x 2
                   planes and the one pass of k_genotype_tallies over the staged COO; nothing is copied out.  Reported beside it:
                   its ratio to the two-class call below, and the COO stream's floor (12 B x entries at 6.3 TB/s) over it
  tallies_out      the same with alt and ref copied out ((K + 1) x 2 x total_loci x 8 B)
  final_tallies    cellector_final_allele_tallies on the same ctx in the same process: the two-class kernel of the parent commit with
                   its memset and its copy of 4 x total_loci x 8 B out (the library has no call that runs it without the copy)
  host_rule        the genotype rule on one host thread in the library: a call with gt / gp / gp3 minus tallies_out
  em_iteration     the default EM iteration of the benchmark loop (ms per iteration, every repetition listed), with this
                   library and, with --parent-lib, with the library of the parent commit in a process of its own

One fresh process per measurement, run one after the other; a measurement that fails ends the run (nothing is tried again).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFGS = {"cfg3": (100_000, 200_000, 0.01), "cfg4": (200_000, 1_000_000, 0.01)}  # loci, cells, density (bench.py's shapes)
STREAM_BYTES_PER_ENTRY, STREAM_TBS = 12, 6.3


def _best(fn, reps):
    out = []
    for _ in range(reps + 1):  # (the first call allocates its scratch from the driver: dropped)
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out[1:]


def child_genotypes(cfg, reps):
    sys.path.insert(0, ROOT)
    import ctypes as C
    from cellector_amd import Cellector
    L, N, d = CFGS[cfg]
    g = Cellector(0)
    g.load_synthetic(L, N, d, seed=4, minority_fraction=0.05)
    g.run(5.0, 30)
    rng = np.random.default_rng(1)
    lab3 = np.where(g.excluded() != 0, 1, 0).astype(np.uint8)
    lab3[rng.random(N) < 0.01] = 2
    lab16 = rng.integers(0, 16, N).astype(np.uint8)
    n = C.c_uint64(0)
    g._ck(g._lib.cellector_staged_coo(g.h, C.byref(n), None, None, None, None, 0))
    entries = int(n.value)
    floor_ms = STREAM_BYTES_PER_ENTRY * entries / (STREAM_TBS * 1e12) * 1e3
    out = dict(cfg=cfg, cells=N, loci=L, loci_used=int(g.dims().loci_used), staged_entries=entries, coo_stream_floor_ms=floor_ms)
    out["final_tallies_ms"] = _best(g.final_allele_tallies, reps)
    for K, lab in ((3, lab3), (16, lab16)):
        p = lab.ctypes.data_as(C.c_void_p)
        none = lambda: g._ck(g._lib.cellector_class_genotypes(g.h, p, K, 0.03, 0.99, None, None, None, None, None, None))
        r = dict(class_cells=np.bincount(lab, minlength=K).tolist())
        r["tally_pass_ms"] = _best(none, reps)
        r["tallies_out_ms"] = _best(lambda: g.class_genotypes(lab, K, genotypes=False), reps)
        r["with_rule_ms"] = _best(lambda: g.class_genotypes(lab, K), reps)
        r["host_rule_ms"] = min(r["with_rule_ms"]) - min(r["tallies_out_ms"])
        r["tally_pass_over_final_tallies"] = min(r["tally_pass_ms"]) / min(out["final_tallies_ms"])
        r["floor_over_tally_pass"] = floor_ms / min(r["tally_pass_ms"])
        out[f"K{K}"] = r
    g.close()
    print(json.dumps(dict(config="class_genotypes", **out)), flush=True)


def child_em(cfg, reps):
    sys.path.insert(0, ROOT)
    from cellector_amd import Cellector, ffi
    if os.environ.get("CELLECTOR_HIP_LIB"):  # an older library: bind what it exports
        import ctypes
        try:
            import torch  # noqa: F401  (its HIP runtime first, as ffi.load_library does)
        except ImportError:
            pass
        probe = ctypes.CDLL(ffi.LIB_PATH)
        for name in [k for k in ffi.SIGNATURES if not hasattr(probe, k)]:
            del ffi.SIGNATURES[name]
    L, N, d = CFGS[cfg]
    g = Cellector(0)
    g.load_synthetic(L, N, d, seed=4, minority_fraction=0.05)
    per_iter = []
    for _ in range(reps + 1):
        g.em_reset()
        t0 = time.perf_counter()
        n = len(g.run(5.0, 30))
        per_iter.append((time.perf_counter() - t0) * 1e3 / n)
    g.close()
    print(json.dumps(dict(config="em_iteration", cfg=cfg, library=ffi.LIB_PATH if os.environ.get("CELLECTOR_HIP_LIB") else "this commit",
                          iterations=n, ms_per_iteration=per_iter[1:], ms_min=min(per_iter[1:]), ms_max=max(per_iter[1:]))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg4", choices=sorted(CFGS))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libcellector_hip.so built from the parent commit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=("genotypes", "em"))
    args = ap.parse_args()
    if args.child:
        (child_genotypes if args.child == "genotypes" else child_em)(args.cfg, args.reps)
        return
    jobs = [("genotypes", None), ("em", None)] + ([("em", args.parent_lib), ("em", None), ("em", args.parent_lib)] if args.parent_lib else [])
    runs = []
    for name, lib in jobs:
        env = dict(os.environ)
        env.pop("CELLECTOR_HIP_LIB", None)
        if lib:
            env["CELLECTOR_HIP_LIB"] = os.path.abspath(lib)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--cfg", args.cfg, "--reps", str(args.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
        if r.returncode != 0:
            sys.exit(f"{name} {args.cfg} failed (status {r.returncode}); stopping\n{r.stderr[-2000:]}")
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        runs.append(json.loads(line))
        if lib:
            runs[-1]["library"] = "parent commit"
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/class_genotypes_cost.py", runs=runs), f, indent=1)


if __name__ == "__main__":
    main()
