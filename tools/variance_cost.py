#!/usr/bin/env python3
"""Cost of DESIGN §3.2d at cfg4 (bench.py's synthetic 200k loci x 10^6 cells at 1 %; needs an MI355X), engine 2.  Every figure is
the median of five device-synchronised EM iterations after a warm-up of four, each iteration timed on its own:

  default      the iteration with normalization 0, this commit's library;
  zscore       the iteration with normalization 1 (the variance pass and the z-score kernel inside it);
  pass         the variance pass alone (k_var_tables + k_cell_variance, without k_zscore): kernel_time(CELLECTOR_K_CELL_VAR) per
               iteration under option timing 1, a loop of its own;
  parent       with --parent-lib PATH/libcellector_hip.so (the parent commit's build): the default iteration of that library and of
               this one in alternating processes, --repeats of each.  The condition of the issue: the difference of the two
               default-mode medians is no larger than the spread (max - min) of the parent's own repeats.

  python tools/variance_cost.py [--cfg cfg4] [--parent-lib PATH] [--repeats 3] [--out profiles/NAME.json]

Each measurement runs in a process of its own (the library is chosen by CELLECTOR_HIP_LIB before the package is imported).
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


def child(what, cfg):
    sys.path.insert(0, ROOT)
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
    if what == "zscore":
        g.set_option("normalization", 1)
    g.load_synthetic(L, N, d, seed=4, minority_fraction=0.05)
    torch.cuda.synchronize()

    def timed_iterations():
        ms, last = [], None
        for i in range(WARMUP + TIMED):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last = g.em_iteration(5.0)
            torch.cuda.synchronize()
            if i >= WARMUP:
                ms.append((time.perf_counter() - t0) * 1e3)
        return ms, last

    ms, s = timed_iterations()
    res = dict(what=what, iteration_ms=ms, iteration_ms_median=statistics.median(ms), n_excluded=int(s.n_excluded),
               loci_used=int(g.dims().loci_used), nnz=int(g.dims().nnz_used))
    if what == "zscore":  # the pass alone, by its event pair
        g.set_option("timing", 1)
        per = []
        for _ in range(1 + TIMED):
            t0 = g.kernel_time(ffi.K_CELL_VAR)[0]
            g.em_iteration(5.0)
            torch.cuda.synchronize()
            per.append(g.kernel_time(ffi.K_CELL_VAR)[0] - t0)
        res.update(pass_ms=per[1:], pass_ms_median=statistics.median(per[1:]))
    g.close()
    print("RESULT " + json.dumps(res), flush=True)


def run_child(what, cfg, lib=None):
    env = dict(os.environ)
    env.pop("CELLECTOR_HIP_LIB", None)
    if lib:
        env["CELLECTOR_HIP_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, "--cfg", cfg], env=env, capture_output=True,
                       text=True, timeout=420)
    if r.returncode != 0:
        sys.exit(f"variance_cost: the '{what}' measurement failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg4", choices=sorted(CFGS))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=["default", "zscore"])
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.cfg)
    L, N, d = CFGS[args.cfg]
    res = dict(tool="tools/variance_cost.py", cfg=args.cfg, cells=N, loci=L, density=d, engine=2, warmup_iterations=WARMUP,
               timed_iterations=TIMED)
    if args.parent_lib:
        parent, this = [], []
        for _ in range(args.repeats):  # alternating: parent, this, parent, this, ...
            parent.append(run_child("default", args.cfg, os.path.abspath(args.parent_lib)))
            this.append(run_child("default", args.cfg))
        pm, tm = [x["iteration_ms_median"] for x in parent], [x["iteration_ms_median"] for x in this]
        res["default_mode_parent_vs_this"] = dict(
            parent_medians_ms=pm, this_medians_ms=tm, parent_iterations_ms=[x["iteration_ms"] for x in parent],
            this_iterations_ms=[x["iteration_ms"] for x in this], parent_median_ms=statistics.median(pm),
            this_median_ms=statistics.median(tm), parent_spread_ms=[min(pm), max(pm)],
            difference_ms=statistics.median(tm) - statistics.median(pm), parent_spread_width_ms=max(pm) - min(pm),
            difference_inside_parent_spread=bool(abs(statistics.median(tm) - statistics.median(pm)) <= max(pm) - min(pm)))
        default = this[-1]
    else:
        default = run_child("default", args.cfg)
    z = run_child("zscore", args.cfg)
    nnz, lu = default["nnz"], default["loci_used"]
    gb = (8.0 * nnz + 144.0 * lu) / 1e9  # the pass' algorithmic bytes: the CSR entries once, the table once
    floor_ms = gb / 6300.0 * 1e3  # at the 6.3 TB/s a plain streaming read reaches on this part
    res.update(loci_used=lu, nnz=nnz, default=default, zscore=z, iteration_default_ms=default["iteration_ms_median"],
               iteration_zscore_ms=z["iteration_ms_median"], variance_pass_ms=z["pass_ms_median"], pass_algorithmic_gb=gb,
               pass_floor_ms_at_6300_gbs=floor_ms, pass_floor_share=floor_ms / z["pass_ms_median"])
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
