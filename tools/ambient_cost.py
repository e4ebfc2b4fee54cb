#!/usr/bin/env python3
"""Cost of the ambient calls on a resident matrix (needs an MI355X), S = 3 sources of random genotypes, every cell assigned.

  python tools/ambient_cost.py [--cfg cfg4] [--reps 5] [--grids 8,16,32] [--parent-lib PATH/libcellector_hip.so]
                               [--out profiles/NAME.json]

Measured, from the library's own lines under CELLECTOR_TIMING=1 (HIP events around the launches; no kernel id of
cellector_kernel_time is used) and the wall clock around the calls, the second of two calls:
  profile_pass_ms       per G: GPU time of k_ambient_e<GP> and the fold of one cellector_ambient_profile
  profile_call_s        per G: wall time of the whole call inside the library (the uploads, the packing, the tables, the pass, the folds
                        and the copies of the outputs asked for: the totals and, here, ll)
  estimate_s            wall time of one cellector_estimate_ambient with the defaults (3 rounds of 16 grid points, per-cell outputs)
  donor_route_s         per G: the route that existed before, G calls of cellector_donor_posteriors at the same S, one per grid point
                        (wall time of the calls, D columns of ll copied out each time); the tool asserts that column j of the
                        profile's ll is ll[c][assign[c]] of call j bit for bit
  profile_over_donor_route   profile_call_s / donor_route_s
  table_bytes           64 G bytes per used locus: what the cell pass reads its rows from
  em_iteration          the default EM iteration of the benchmark loop (ms per iteration, every repetition listed), with this library
                        and, with --parent-lib, with the library of the parent commit in a process of its own, alternating

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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from donors_cost import CFGS, child_em  # noqa: E402  (the same configurations and the same EM measurement)

S = 3
PASS_LINE = re.compile(r"ambient: S (\d+) G (\d+) cell pass and folds ([\d.]+) ms, whole call ([\d.]+) s")
EST_LINE = re.compile(r"ambient: S (\d+) G (\d+) rounds (\d+), whole call ([\d.]+) s")


def child_ambient(cfg, grids):
    sys.path.insert(0, ROOT)
    import numpy as np
    from cellector_amd import Cellector
    L, N, d = CFGS[cfg]
    g = Cellector(0)
    g.load_synthetic(L, N, d, seed=4, minority_fraction=0.05)
    TL, Lu = int(g.dims().total_loci), int(g.dims().loci_used)
    gt = np.random.default_rng(S).choice(4, (S, TL), p=[0.4, 0.3, 0.2, 0.1]).astype(np.uint8)
    assign = (np.arange(N) % S).astype(np.uint8)
    rows = np.arange(N)
    out = dict(cfg=cfg, cells=N, loci=L, loci_used=Lu, entries=int(g.dims().nnz_used), sources=S, runs=[])
    for G in grids:
        rho = np.linspace(0.0, 0.5, G)
        walls = []
        for _ in range(2):
            t0 = time.perf_counter()
            r = g.ambient_profile(gt, assign, rho)
            walls.append(time.perf_counter() - t0)
        same, t0 = True, time.perf_counter()
        for j in range(G):
            dp = g.donor_posteriors(gt, ambient=float(rho[j]))
            same = same and dp["ll"][rows, assign].tobytes() == r["ll"][:, j].tobytes()
            del dp
        route = time.perf_counter() - t0
        out["runs"].append(dict(G=G, profile_wall_s=walls, donor_route_s=route, ll_equals_donor_route=bool(same), table_bytes=64 * G * Lu))
        assert same, G
        del r
    walls = []
    for _ in range(2):
        t0 = time.perf_counter()
        e = g.estimate_ambient(gt, assign)
        walls.append(time.perf_counter() - t0)
    out["estimate"] = dict(wall_s=walls, rho=e["rho"], se=e["se"], rounds=int(e["rounds"]), grid=16)
    g.close()
    print(json.dumps(dict(config="ambient", **out)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg4", choices=sorted(CFGS))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--grids", default="8,16,32")
    ap.add_argument("--parent-lib", default=None, help="libcellector_hip.so built from the parent commit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=("ambient", "em"))
    args = ap.parse_args()
    grids = [int(x) for x in args.grids.split(",")]
    if any(G < 4 or G > 32 for G in grids):
        sys.exit("--grids: values in 4..32")
    if args.child == "ambient":
        return child_ambient(args.cfg, grids)
    if args.child == "em":
        return child_em(args.cfg, args.reps)
    jobs = [("ambient", None), ("em", None)] + ([("em", args.parent_lib), ("em", None), ("em", args.parent_lib)] if args.parent_lib else [])
    runs = []
    for name, lib in jobs:
        env = dict(os.environ)
        env.pop("CELLECTOR_HIP_LIB", None)
        env["CELLECTOR_TIMING"] = "1"
        if lib:
            env["CELLECTOR_HIP_LIB"] = os.path.abspath(lib)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--cfg", args.cfg, "--reps", str(args.reps), "--grids", args.grids]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1100, env=env)
        if r.returncode != 0:
            sys.exit(f"{name} {args.cfg} failed (status {r.returncode}); stopping\n{r.stderr[-2000:]}")
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        if name == "ambient":
            pl, el = PASS_LINE.findall(r.stderr), EST_LINE.findall(r.stderr)
            for i, run in enumerate(rec["runs"]):  # (two calls per G: the second counts)
                m = pl[2 * i + 1]
                assert int(m[1]) == run["G"]
                run.update(profile_pass_ms=float(m[2]), profile_call_s=float(m[3]), profile_over_donor_route=float(m[3]) / run["donor_route_s"])
            rec["estimate"]["estimate_s"] = float(el[-1][3])
        if lib:
            rec["library"] = "parent commit"
        print(json.dumps(rec), flush=True)
        runs.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/ambient_cost.py", runs=runs), f, indent=1)


if __name__ == "__main__":
    main()
