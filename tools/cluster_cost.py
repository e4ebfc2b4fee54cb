#!/usr/bin/env python3
"""Cost of the genotype clustering on a resident matrix (needs an MI355X), K = 3 with R = 1, 4 and 16 restarts.

  python tools/cluster_cost.py [--cfg cfg4] [--reps 5] [--restarts 1,4,16] [--max-iter 3] [--anneal-steps 3]
                               [--parent-lib PATH/libcellector_hip.so] [--out profiles/NAME.json]

Measured per R, from the library's own line under CELLECTOR_TIMING=1 (HIP events around every launch of the call; no kernel id of
cellector_kernel_time is used):
  e_step_ms / m_step_ms   GPU time of one E step (k_cluster_e + the objective fold) and one M step (k_cluster_m), mean over the call
  by_locus_list_s         wall time of the by-locus list (a stable sort of the by-cell CSR by locus), built once per call
  whole_call_s            wall time of the whole cellector_cluster with --max-iter iterations in each of --anneal-steps stages (the
                          defaults, 50 and 9, are what a user runs: pass them to measure that), and the iterations it ran
  em_iteration            the default EM iteration of the benchmark loop (ms per iteration, every repetition listed), with this
                          library and, with --parent-lib, with the library of the parent commit in a process of its own, alternating

One fresh process per measurement, run one after the other; a measurement that fails ends the run (nothing is tried again).
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFGS = {"cfg2": (50_000, 50_000, 0.01), "cfg3": (100_000, 200_000, 0.01), "cfg4": (200_000, 1_000_000, 0.01)}  # loci, cells, density
K = 3
LINE = re.compile(r"cluster: K (\d+) R (\d+) by-locus list ([\d.]+) s, E step ([\d.]+) ms x (\d+), M step ([\d.]+) ms x (\d+), whole call ([\d.]+) s")


def child_cluster(cfg, restarts, max_iter, anneal_steps):
    sys.path.insert(0, ROOT)
    from cellector_amd import Cellector
    L, N, d = CFGS[cfg]
    g = Cellector(0)
    g.load_synthetic(L, N, d, seed=4, minority_fraction=0.05)
    out = dict(cfg=cfg, cells=N, loci=L, loci_used=int(g.dims().loci_used), entries=int(g.dims().nnz_used), K=K, max_iter=max_iter,
               anneal_steps=anneal_steps, runs=[])
    for R in restarts:
        t0 = time.perf_counter()
        r = g.cluster(K, R, seed=1, max_iter=max_iter, anneal_steps=anneal_steps)
        out["runs"].append(dict(R=R, wall_s=time.perf_counter() - t0, iterations=int(r["summary"].iterations),
                                cluster_cells=list(r["summary"].cluster_cells)[:K]))
    g.close()
    print(json.dumps(dict(config="cluster", **out)), flush=True)


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
    ap.add_argument("--restarts", default="1,4,16")
    ap.add_argument("--max-iter", type=int, default=3)
    ap.add_argument("--anneal-steps", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="libcellector_hip.so built from the parent commit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=("cluster", "em"))
    args = ap.parse_args()
    restarts = [int(x) for x in args.restarts.split(",")]
    if args.child == "cluster":
        return child_cluster(args.cfg, restarts, args.max_iter, args.anneal_steps)
    if args.child == "em":
        return child_em(args.cfg, args.reps)
    jobs = [("cluster", None), ("em", None)] + ([("em", args.parent_lib), ("em", None), ("em", args.parent_lib)] if args.parent_lib else [])
    runs = []
    for name, lib in jobs:
        env = dict(os.environ)
        env.pop("CELLECTOR_HIP_LIB", None)
        env["CELLECTOR_TIMING"] = "1"
        if lib:
            env["CELLECTOR_HIP_LIB"] = os.path.abspath(lib)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--cfg", args.cfg, "--reps", str(args.reps), "--restarts",
               args.restarts, "--max-iter", str(args.max_iter), "--anneal-steps", str(args.anneal_steps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1100, env=env)
        if r.returncode != 0:
            sys.exit(f"{name} {args.cfg} failed (status {r.returncode}); stopping\n{r.stderr[-2000:]}")
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        if name == "cluster":
            for run, m in zip(rec["runs"], LINE.finditer(r.stderr)):
                assert int(m.group(2)) == run["R"]
                run.update(by_locus_list_s=float(m.group(3)), e_step_ms=float(m.group(4)), e_steps=int(m.group(5)),
                           m_step_ms=float(m.group(6)), m_steps=int(m.group(7)), whole_call_s=float(m.group(8)))
        if lib:
            rec["library"] = "parent commit"
        print(json.dumps(rec), flush=True)
        runs.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/cluster_cost.py", runs=runs), f, indent=1)


if __name__ == "__main__":
    main()
