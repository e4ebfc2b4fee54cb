#!/usr/bin/env python3
"""Cost of placing the EM state on a resident matrix (needs an MI355X): wall time of cellector_em_reset,
cellector_set_loci_mask and cellector_set_excluded (a 5 % set — the benchmark's fixed point — and a 50 % set), beside the only
thing a ctx without them offers for the same purpose: a fresh load_synthetic of the same shape on a new ctx.

  python tools/state_cost.py [--cfgs cfg3,cfg4] [--reps 3] [--out profiles/NAME.json]

One fresh process per configuration, run one after the other; best of --reps calls; a configuration that fails ends the sweep
(nothing is tried again).  Prints one JSON line per configuration and writes them all to --out.  For the tally kernel's own
time run one configuration under the profiler, kernel trace only:

  rocprofv3 --kernel-trace --stats -d DIR -- python tools/state_cost.py --child set_excluded_5 --cfg cfg4
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
CONFIGS = ("reload", "em_reset", "set_loci_mask", "set_excluded_5", "set_excluded_50")


def child(name, cfg, reps):
    sys.path.insert(0, ROOT)
    from cellector_amd import Cellector
    L, N, d = CFGS[cfg]
    times, extra = [], {}
    if name == "reload":  # what the parent commit offers: the matrix again, on a new ctx
        g = Cellector(0)
        g.load_synthetic(L, N, d, seed=4, minority_fraction=0.05)  # (the process' first load pays the runtime's start-up: dropped)
        g.close()
        for _ in range(reps):
            t0 = time.perf_counter()
            g = Cellector(0)
            g.load_synthetic(L, N, d, seed=4, minority_fraction=0.05)
            times.append((time.perf_counter() - t0) * 1e3)
            g.close()
    else:
        g = Cellector(0)
        g.load_synthetic(L, N, d, seed=4, minority_fraction=0.05)
        iters = len(g.run(5.0, 30))
        fixed = g.excluded()
        extra = dict(em_iterations=iters, n_excluded_fixed_point=int(fixed.sum()))
        rng = np.random.default_rng(1)
        if name == "set_excluded_5":
            arg = fixed  # the benchmark's fixed point
        elif name == "set_excluded_50":
            arg = (rng.random(N) < 0.5).astype(np.uint8)
        elif name == "set_loci_mask":
            arg = (rng.random(g.dims().loci_used) < 0.8).astype(np.uint8)
        for _ in range(reps + 1):  # (the first call allocates its scratch from the driver: dropped)
            t0 = time.perf_counter()
            if name == "em_reset":
                g.em_reset()
            elif name == "set_loci_mask":
                g.set_loci_mask(arg)
            else:
                g.set_excluded(arg)
            times.append((time.perf_counter() - t0) * 1e3)
        times = times[1:]
        if name.startswith("set_excluded"):
            extra["n_placed"] = int(arg.sum())
            t0 = time.perf_counter()
            s = g.em_iteration(5.0)  # the iteration that follows recounts the kept counts
            extra["next_iteration_ms"] = (time.perf_counter() - t0) * 1e3
            extra["next_iteration"] = [int(s.n_new_excluded), int(s.n_rescued), int(s.n_excluded)]
        g.close()
    print(json.dumps(dict(config=name, cfg=cfg, cells=N, loci=L, ms=times, ms_min=min(times), **extra)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfgs", default="cfg3,cfg4")
    ap.add_argument("--cfg", default="cfg4", choices=sorted(CFGS), help="(with --child)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=CONFIGS)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.cfg, args.reps)
        return
    runs = []
    for cfg in args.cfgs.split(","):
        for name in CONFIGS:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--cfg", cfg, "--reps", str(args.reps)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.exit(f"{name} {cfg} failed (status {r.returncode}); stopping\n{r.stderr[-2000:]}")
            line = r.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            runs.append(json.loads(line))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/state_cost.py", runs=runs), f, indent=1)


if __name__ == "__main__":
    main()
