#!/usr/bin/env python3
"""Cost of DESIGN §3.2e at cfg4 (bench.py's synthetic 200k loci x 10^6 cells at 1 %; needs an MI355X), engine 2.  Every iteration
figure is the median of five device-synchronised EM iterations after a warm-up of four, each iteration timed on its own:

  default      the iteration with locus_moments 0, this commit's library;
  moments      the iteration with locus_moments 1 (k_lm_count over the new exclusion set's rows + k_lm_finalize behind the locus
               pass); the pass alone by kernel_time(CELLECTOR_K_LOCUS_MOM) per iteration under option timing 1, a loop of its own;
               and the one-off static build (the all-cells histogram and the far list): the wall time of the first
               cellector_locus_moments call of the process less that of a second, identical one;
  parent       with --parent-lib PATH/libcellector_hip.so (the parent commit's build): the default iteration of that library and of
               this one in alternating processes, --repeats of each.  The condition of the issue: this commit's median exceeds the
               parent's by no more than the spread (max - min) of the parent's own repeats.

  python tools/locus_moments_cost.py [--cfg cfg4] [--parent-lib PATH] [--repeats 3] [--out profiles/r8_locus_moments_cost.json]

Each measurement runs in a process of its own (the library is chosen by CELLECTOR_HIP_LIB before the package is imported), under
a time limit; the first that fails ends the run.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFGS = {"cfg1": (2_000, 1_000, 0.1), "cfg3": (100_000, 200_000, 0.01), "cfg4": (200_000, 1_000_000, 0.01)}  # loci, cells, density
WARMUP, TIMED = 4, 5
CHILD_LIMIT_S = 420


def child(what, cfg):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from cellector_amd import ffi
    if os.environ.get("CELLECTOR_HIP_LIB"):  # an older library: bind what it exports
        lib = ctypes.CDLL(ffi.LIB_PATH)
        for name in [n for n in ffi.SIGNATURES if not hasattr(lib, n)]:
            del ffi.SIGNATURES[name]
    from cellector_amd import Cellector
    L, N, d = CFGS[cfg]
    g = Cellector(0, stream=torch.cuda.current_stream().cuda_stream)
    g.set_option("engine", 2)
    g.set_option("keep_coo", 0)
    g.load_synthetic(L, N, d, seed=4, minority_fraction=0.05)
    torch.cuda.synchronize()
    res = dict(what=what, loci_used=int(g.dims().loci_used), nnz=int(g.dims().nnz_used))
    if what == "moments":  # the static build first, on the fresh ctx: first call less second call
        a, b = g.alpha_betas()
        flags = np.zeros(N, np.uint8)
        calls = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            g.locus_moments(a, b, None, flags)
            calls.append((time.perf_counter() - t0) * 1e3)
        counts = g.locus_total_counts()
        res.update(call_ms=calls, static_build_ms=calls[0] - calls[1], far_entries=int(counts[:, 18].sum()),
                   table_entries=int(counts[:, :18].sum()))
        g.set_option("locus_moments", 1)

    ms, s = [], None
    for i in range(WARMUP + TIMED):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s = g.em_iteration(5.0)
        torch.cuda.synchronize()
        if i >= WARMUP:
            ms.append((time.perf_counter() - t0) * 1e3)
    res.update(iteration_ms=ms, iteration_ms_median=statistics.median(ms), n_excluded=int(s.n_excluded))
    if what == "moments":  # the pass alone, by its event pair
        res["excluded_entries"] = int(g.entries_per_cell()[g.excluded() != 0].astype(np.int64).sum())
        g.set_option("timing", 1)
        per = []
        for _ in range(1 + TIMED):
            t0 = g.kernel_time(ffi.K_LOCUS_MOM)[0]
            g.em_iteration(5.0)
            torch.cuda.synchronize()
            per.append(g.kernel_time(ffi.K_LOCUS_MOM)[0] - t0)
        res.update(pass_ms=per[1:], pass_ms_median=statistics.median(per[1:]))
    g.close()
    print("RESULT " + json.dumps(res), flush=True)


def run_child(what, cfg, lib=None):
    env = dict(os.environ)
    env.pop("CELLECTOR_HIP_LIB", None)
    if lib:
        env["CELLECTOR_HIP_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, "--cfg", cfg], env=env, capture_output=True,
                       text=True, timeout=CHILD_LIMIT_S)
    if r.returncode != 0:
        sys.exit(f"locus_moments_cost: the '{what}' measurement failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    res = json.loads(line[len("RESULT "):])
    print(f"[{'parent' if lib else 'this'} {what}] iteration {res['iteration_ms_median']:.3f} ms", file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg4", choices=sorted(CFGS))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=["default", "moments"])
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.cfg)
    L, N, d = CFGS[args.cfg]
    res = dict(tool="tools/locus_moments_cost.py", cfg=args.cfg, cells=N, loci=L, density=d, engine=2, warmup_iterations=WARMUP,
               timed_iterations=TIMED)
    if args.parent_lib:
        parent, this = [], []
        for _ in range(args.repeats):  # alternating: parent, this, parent, this, ...
            parent.append(run_child("default", args.cfg, os.path.abspath(args.parent_lib)))
            this.append(run_child("default", args.cfg))
        pm, tm = [x["iteration_ms_median"] for x in parent], [x["iteration_ms_median"] for x in this]
        excess = statistics.median(tm) - statistics.median(pm)
        res["default_mode_parent_vs_this"] = dict(
            parent_medians_ms=pm, this_medians_ms=tm, parent_iterations_ms=[x["iteration_ms"] for x in parent],
            this_iterations_ms=[x["iteration_ms"] for x in this], parent_median_ms=statistics.median(pm),
            this_median_ms=statistics.median(tm), parent_spread_ms=[min(pm), max(pm)], difference_ms=excess,
            parent_spread_width_ms=max(pm) - min(pm), excess_inside_parent_spread=bool(excess <= max(pm) - min(pm)))
        default = this[-1]
    else:
        default = run_child("default", args.cfg)
    m = run_child("moments", args.cfg)
    lu = m["loci_used"]
    # the pass' algorithmic bytes: the CSR entries of the excluded rows once, the two histograms (written and read), the far list
    gb = (8.0 * m["excluded_entries"] + 2.0 * lu * 18 * 4 + 8.0 * m["far_entries"] + 8.0 * (lu + 1)) / 1e9
    floor_ms = gb / 6300.0 * 1e3  # at the 6.3 TB/s a plain streaming read reaches on this part
    # the one figure on scattered u32 atomics the repository has: k_t2_minority, 1.1e7 in 0.43 ms
    atomics_ms = m["excluded_entries"] / 1.1e7 * 0.43
    res.update(loci_used=lu, nnz=m["nnz"], default=default, moments=m, iteration_default_ms=default["iteration_ms_median"],
               iteration_moments_ms=m["iteration_ms_median"], moments_pass_ms=m["pass_ms_median"], static_build_ms=m["static_build_ms"],
               pass_algorithmic_gb=gb, pass_floor_ms_at_6300_gbs=floor_ms, pass_floor_share=floor_ms / m["pass_ms_median"],
               pass_atomics=m["excluded_entries"], pass_atomics_ms_at_t2_minority_rate=atomics_ms,
               pass_atomic_bound=bool(m["pass_ms_median"] < 3.0 * atomics_ms and atomics_ms > 3.0 * floor_ms))
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
