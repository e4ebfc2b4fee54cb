#!/usr/bin/env python3
"""Cost of the K-class doublet scoring on a resident matrix (needs an MI355X), K = 3 and K = 8: the synthetic minority as class 1,
random shares of the other cells as classes 2 .. K - 1, the rest class 0.

  python tools/class_doublets_cost.py [--cfg cfg4] [--reps 5] [--parent-lib PATH/libcellector_hip.so] [--out profiles/NAME.json]

Measured per K, best of --reps wall times of the calls (each ends synchronised):
  class_doublets   one cellector_class_doublets call without outputs (recount, alpha / beta, K + P cell passes each behind its
                   distribution, finalize); beside it the GPU time of its K + P cell passes (HIP events, option timing) and
                   (K + P) x the GPU time of one pass of cellector_cell_log_likelihoods
  outside_the_passes  the call's wall time minus its passes' GPU time: the copies of labels and flags in, the recount, the K + P
                   distributions, the column copies, the finalize and the launch gaps together (the finalize has no timer of its
                   own and is not separated from them)
  refine_step      the second step of a held-out refine that starts 0.1 % of the cells away from its fixed point: max_iter = 2
                   minus max_iter = 1 with class_delta 1 (the moved rows only) and with class_delta 0 (a recount)
  em_iteration     the default EM iteration of the benchmark loop (ms per iteration, every repetition listed), with this library
                   and, with --parent-lib, with the library of the parent commit, in alternating fresh processes

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
KS = (3, 8)


def _best(fn, reps):
    out = []
    for _ in range(reps + 1):  # (the first call allocates its scratch from the driver: dropped)
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out[1:]


def _none_out(g, lab, held, K, max_iter=None):
    """the raw call without outputs: what the device does, without the copies of K + P columns to the host"""
    from cellector_amd import ffi
    p = ffi._p
    if max_iter is None:
        g._ck(g._lib.cellector_class_doublets(g.h, p(lab), p(held), K, *([None] * 13)))
        return None
    l, h, s = lab.copy(), held.copy(), ffi.RefineDoubletsSummary()
    import ctypes
    g._ck(g._lib.cellector_refine_class_doublets(g.h, p(l), p(h), K, None, None, None, None, None, 0.5, max_iter, 1, ctypes.byref(s),
                                                 *([None] * 6)))
    return l, h, s


def child_doublets(cfg, reps):
    sys.path.insert(0, ROOT)
    from cellector_amd import Cellector, ffi
    L, N, d = CFGS[cfg]
    g = Cellector(0)
    g.load_synthetic(L, N, d, seed=4, minority_fraction=0.05)
    g.run(5.0, 30)
    rng = np.random.default_rng(1)
    runs = []
    for K in KS:
        P = K * (K - 1) // 2
        lab = np.where(g.excluded() != 0, 1, 0).astype(np.uint8)
        r = rng.random(N)
        for k in range(2, K):
            lab[(r >= 0.01 * (k - 2)) & (r < 0.01 * (k - 1))] = k
        held = np.zeros(N, np.uint8)
        out = dict(K=K, pairs=P, class_cells=np.bincount(lab, minlength=K).tolist())
        g.set_option("timing", 1)
        g.reset_timing()
        out["class_doublets_ms"] = _best(lambda: _none_out(g, lab, held, K), reps)
        ms, launches = g.kernel_time(ffi.K_CELL_LL)
        out["passes"] = launches // (reps + 1)
        out["class_doublets_passes_gpu_ms"] = ms / max(launches, 1) * (K + P)
        out["class_doublets_outside_the_passes_ms"] = min(out["class_doublets_ms"]) - out["class_doublets_passes_gpu_ms"]
        g.reset_timing()
        a, b = g.class_alpha_betas(lab, K)
        for _ in range(reps):
            g.cell_log_likelihoods(a[0], b[0])
        ms, launches = g.kernel_time(ffi.K_CELL_LL)
        out["one_cell_pass_gpu_ms"] = ms / max(launches, 1)
        out["k_plus_p_cell_passes_gpu_ms"] = out["one_cell_pass_gpu_ms"] * (K + P)
        g.set_option("timing", 0)
        fl, fh, fs = _none_out(g, lab, held, K, 30)
        out["refine_to_fixed_point"] = dict(iterations=fs.iterations, converged=fs.converged, n_moved_total=fs.n_moved_total,
                                            n_recounts=fs.n_recounts, n_held=fs.n_held)
        start = fl.copy()
        pick = rng.choice(N, N // 1000, replace=False)
        start[pick] = (start[pick] + 1) % 2  # 0.1 % of the cells, between the two large classes
        for delta in (1, 0):
            g.set_option("class_delta", delta)
            one = _best(lambda: _none_out(g, start, fh, K, 1), reps)
            two = _best(lambda: _none_out(g, start, fh, K, 2), reps)
            s = _none_out(g, start, fh, K, 2)[2]
            out[f"refine_step_class_delta_{delta}"] = dict(one_step_ms=one, two_steps_ms=two, second_step_ms=min(two) - min(one),
                                                           moved_first_step=s.n_moved_total - s.n_moved_last, n_recounts=s.n_recounts)
        g.set_option("class_delta", 1)
        runs.append(out)
    dims = dict(cfg=cfg, cells=N, loci=L, loci_used=int(g.dims().loci_used), entries=int(g.dims().nnz_used))
    g.close()
    print(json.dumps(dict(config="class_doublets", **dims, per_k=runs)), flush=True)


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
    ap.add_argument("--child", default=None, choices=("doublets", "em"))
    args = ap.parse_args()
    if args.child:
        (child_doublets if args.child == "doublets" else child_em)(args.cfg, args.reps)
        return
    jobs = [("doublets", None), ("em", None)] + ([("em", args.parent_lib), ("em", None), ("em", args.parent_lib)] if args.parent_lib else [])
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
            json.dump(dict(tool="tools/class_doublets_cost.py", runs=runs), f, indent=1)


if __name__ == "__main__":
    main()
