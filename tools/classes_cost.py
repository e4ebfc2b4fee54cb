#!/usr/bin/env python3
"""Cost of the K-genotype class scoring on a resident matrix (needs an MI355X), K = 3: the synthetic minority as class 1, a random
1 % of the cells as class 2, the rest class 0.

  python tools/classes_cost.py [--cfg cfg4] [--reps 5] [--parent-lib PATH/libcellector_hip.so] [--out profiles/NAME.json]

Measured, best of --reps wall times of the calls (each ends synchronised):
  recount          cellector_class_tallies: the first recount (never walks class 0) and the copy of the K x L x 2 integers out
  refine_step      one whole step, cellector_refine_classes(max_iter = 1): recount, alpha / beta, three cell passes, finalize, the
                   read-back, and the copies of labels in and out; beside it the GPU time of its three cell passes (HIP events,
                   option timing) and the wall time of three cellector_cell_log_likelihoods calls
  delta_step       the second step of a refine that starts 0.1 % of the cells away from its fixed point: max_iter = 2 minus
                   max_iter = 1 with class_delta 1 (the moved rows only) and with class_delta 0 (a recount)
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
K = 3


def _best(fn, reps):
    out = []
    for _ in range(reps + 1):  # (the first call allocates its scratch from the driver: dropped)
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out[1:]


def child_classes(cfg, reps):
    sys.path.insert(0, ROOT)
    from cellector_amd import Cellector, ffi
    L, N, d = CFGS[cfg]
    g = Cellector(0)
    g.load_synthetic(L, N, d, seed=4, minority_fraction=0.05)
    g.run(5.0, 30)
    rng = np.random.default_rng(1)
    lab = np.where(g.excluded() != 0, 1, 0).astype(np.uint8)
    lab[rng.random(N) < 0.01] = 2
    sizes = np.bincount(lab, minlength=K).tolist()
    out = dict(cfg=cfg, cells=N, loci=L, loci_used=int(g.dims().loci_used), entries=int(g.dims().nnz_used), class_cells=sizes)
    out["recount_ms"] = _best(lambda: g.class_tallies(lab, K), reps)
    g.set_option("timing", 1)
    g.reset_timing()
    out["refine_step_ms"] = _best(lambda: g.refine_classes(lab, K, max_iter=1), reps)
    ms, launches = g.kernel_time(ffi.K_CELL_LL)
    out["refine_step_cell_pass_gpu_ms"] = ms / max(launches, 1) * K
    g.set_option("timing", 0)
    a, b = g.class_alpha_betas(lab, K)
    out["three_cell_log_likelihoods_ms"] = _best(lambda: [g.cell_log_likelihoods(a[k], b[k]) for k in range(K)], reps)
    fixed = g.refine_classes(lab, K, max_iter=30)
    out["refine_to_fixed_point"] = dict(iterations=fixed["summary"].iterations, converged=fixed["summary"].converged,
                                        n_moved_total=fixed["summary"].n_moved_total, n_recounts=fixed["summary"].n_recounts)
    start = fixed["labels"].copy()
    pick = rng.choice(N, N // 1000, replace=False)
    start[pick] = (start[pick] + 1) % 2  # 0.1 % of the cells, between the two large classes
    for delta in (1, 0):
        g.set_option("class_delta", delta)
        one = _best(lambda: g.refine_classes(start, K, max_iter=1), reps)
        two = _best(lambda: g.refine_classes(start, K, max_iter=2), reps)
        s = g.refine_classes(start, K, max_iter=2)["summary"]
        out[f"delta_step_class_delta_{delta}"] = dict(one_step_ms=one, two_steps_ms=two, second_step_ms=min(two) - min(one),
                                                      moved_first_step=s.n_moved_total - s.n_moved_last, n_recounts=s.n_recounts)
    g.close()
    print(json.dumps(dict(config="classes", **out)), flush=True)


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
    ap.add_argument("--child", default=None, choices=("classes", "em"))
    args = ap.parse_args()
    if args.child:
        (child_classes if args.child == "classes" else child_em)(args.cfg, args.reps)
        return
    jobs = [("classes", None), ("em", None)] + ([("em", args.parent_lib), ("em", None), ("em", args.parent_lib)] if args.parent_lib else [])
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
            json.dump(dict(tool="tools/classes_cost.py", runs=runs), f, indent=1)


if __name__ == "__main__":
    main()
