#!/usr/bin/env python3
"""Cost of cellector_donor_fit on a resident matrix (needs an MI355X), D = 8, 32 and 64 donors of random genotypes.

  python tools/donor_fit_cost.py [--cfg cfg4] [--reps 5] [--donors 8,32,64] [--parent-lib PATH/libcellector_hip.so]
                                 [--out profiles/NAME.json]

Measured per D, from the library's own line under CELLECTOR_TIMING=1 (HIP events around the launches), the second of two calls:
  singlet_pass_ms / pair_pass_ms   GPU time of k_donor_e<DP, false> and k_donor_e<DP, true> inside the fit call: the donor call it runs
  fit_pass_ms                      GPU time of k_donor_fit<DP> on the same ctx in the same call: one walk, four ordered sums per lane, a
                                   mom1 and a mom2 row per entry
  fit_over_singlet / fit_over_both fit_pass_ms / singlet_pass_ms and fit_pass_ms / (singlet_pass_ms + pair_pass_ms)
  whole_call_s                     wall time of the whole cellector_donor_fit inside the library: the donor call, the moment tables, the
                                   fit pass, the copies of every output to the host, the select over the keys and the flags
  em_iteration                     the default EM iteration of the benchmark loop (ms per iteration, every repetition listed), with
                                   this library and, with --parent-lib, with the library of the parent commit in a process of its
                                   own, alternating

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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from donors_cost import CFGS, child_em  # noqa: E402  (the same matrices and the same loop measurement)

FIT_LINE = re.compile(r"donor_fit: D (\d+) singlet pass ([\d.]+) ms, pair pass ([\d.]+) ms, fit pass ([\d.]+) ms, whole call ([\d.]+) s")


def child_fit(cfg, donors):
    sys.path.insert(0, ROOT)
    import numpy as np
    from cellector_amd import Cellector
    L, N, d = CFGS[cfg]
    g = Cellector(0)
    g.load_synthetic(L, N, d, seed=4, minority_fraction=0.05)
    TL = int(g.dims().total_loci)
    out = dict(cfg=cfg, cells=N, loci=L, loci_used=int(g.dims().loci_used), entries=int(g.dims().nnz_used), runs=[])
    for D in donors:
        gt = np.random.default_rng(D).choice(4, (D, TL), p=[0.4, 0.3, 0.2, 0.1]).astype(np.uint8)
        walls = []
        for _ in range(2):
            t0 = time.perf_counter()
            r = g.donor_fit(gt)
            walls.append(time.perf_counter() - t0)
        s = r["summary"]
        out["runs"].append(dict(D=D, wall_s=walls, n_keys=int(s.n_keys), threshold=float(s.threshold), n_unmatched=int(s.n_unmatched),
                                table_bytes_per_entry_at_most=8 * ((D + 31) // 32) + 4 * 16 + 16 * 16))
        del r
    g.close()
    print(json.dumps(dict(config="donor_fit", **out)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg4", choices=sorted(CFGS))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--donors", default="8,32,64")
    ap.add_argument("--parent-lib", default=None, help="libcellector_hip.so built from the parent commit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=("fit", "em"))
    args = ap.parse_args()
    donors = [int(x) for x in args.donors.split(",")]
    if args.child == "fit":
        return child_fit(args.cfg, donors)
    if args.child == "em":
        return child_em(args.cfg, args.reps)
    jobs = [("fit", None), ("em", None)] + ([("em", args.parent_lib), ("em", None), ("em", args.parent_lib)] if args.parent_lib else [])
    runs = []
    for name, lib in jobs:
        env = dict(os.environ)
        env.pop("CELLECTOR_HIP_LIB", None)
        env["CELLECTOR_TIMING"] = "1"
        if lib:
            env["CELLECTOR_HIP_LIB"] = os.path.abspath(lib)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--cfg", args.cfg, "--reps", str(args.reps), "--donors", args.donors]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1100, env=env)
        if r.returncode != 0:
            sys.exit(f"{name} {args.cfg} failed (status {r.returncode}); stopping\n{r.stderr[-2000:]}")
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        if name == "fit":
            fl = FIT_LINE.findall(r.stderr)
            for i, run in enumerate(rec["runs"]):  # (two calls per D: the second counts)
                m = fl[2 * i + 1]
                assert int(m[0]) == run["D"]
                sp, pp, fp = float(m[1]), float(m[2]), float(m[3])
                run.update(singlet_pass_ms=sp, pair_pass_ms=pp, fit_pass_ms=fp, whole_call_s=float(m[4]), fit_over_singlet=fp / sp,
                           fit_over_both=fp / (sp + pp))
        if lib:
            rec["library"] = "parent commit"
        print(json.dumps(rec), flush=True)
        runs.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/donor_fit_cost.py", runs=runs), f, indent=1)


if __name__ == "__main__":
    main()
