#!/usr/bin/env python3
"""Cost of the donor calls from genotype probabilities on a resident matrix (needs an MI355X), D = 8, 32 and 64 donors.

  python tools/donor_gp_cost.py [--cfg cfg4] [--reps 5] [--donors 8,32,64] [--parent-lib PATH/libcellector_hip.so]
                                [--out profiles/r18_donor_gp_cost.json]

Measured per D, from the library's own lines under CELLECTOR_TIMING=1 (HIP events around the launches), the second of two calls, all
in one process on the same random genotypes:
  hard       cellector_donor_posteriors(gt): k_donor_e<DP, false> / <DP, true>
  one_hot    cellector_donor_posteriors_gp(one-hot of gt): k_donor_gp_e, every row a lookup.  Its ll and pair_ll must equal the hard
             call's bit for bit; the tool asserts it
  soft_20    the same with 20 % of the called rows replaced by three positive weights
  soft_100   ... with all of them
  each: singlet_pass_ms, pair_pass_ms (GPU time), whole_call_s (the library's wall time: upload, weights, tables, both passes, every
  output copied to the host), and the ratios of the passes to the hard call's
  em_iteration   the default EM iteration of the benchmark loop (ms per iteration, every repetition listed), with this library and,
                 with --parent-lib, with the library of the parent commit in a process of its own, alternating

One fresh process per measurement, run one after the other; a measurement that fails ends the run (nothing is tried again).
"""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from donors_cost import CFGS, child_em  # noqa: E402  (the same configurations and the same EM measurement)

LINE = re.compile(r"donors( \(gp\))?: D (\d+) singlet pass ([\d.]+) ms, pair pass ([\d.]+) ms, whole call ([\d.]+) s")
VARIANTS = ("hard", "one_hot", "soft_20", "soft_100")


def child_gp(cfg, donors):
    sys.path.insert(0, ROOT)
    import numpy as np
    from cellector_amd import Cellector, donors as dn
    L, N, d = CFGS[cfg]
    g = Cellector(0)
    g.load_synthetic(L, N, d, seed=4, minority_fraction=0.05)
    TL = int(g.dims().total_loci)
    out = dict(cfg=cfg, cells=N, loci=L, loci_used=int(g.dims().loci_used), entries=int(g.dims().nnz_used), runs=[])
    for D in donors:
        rng = np.random.default_rng(D)
        gt = rng.choice(4, (D, TL), p=[0.4, 0.3, 0.2, 0.1]).astype(np.uint8)
        one = dn.one_hot(gt)
        soft = rng.dirichlet(np.ones(3) * 2.0, (D, TL)).astype(np.float32)
        pick = rng.random((D, TL))
        rec = dict(D=D)
        for name in VARIANTS:
            if name == "hard":
                call = lambda: g.donor_posteriors(gt)
            else:
                share = dict(one_hot=0.0, soft_20=0.2, soft_100=1.0)[name]
                gp = np.where(((gt < 3) & (pick < share))[..., None], soft, one)
                call = lambda: g.donor_posteriors_gp(gp)
            call()
            r = call()
            s = r["summary"]
            rec[name] = dict(status=[int(s.n_singlet), int(s.n_doublet), int(s.n_ambiguous), int(s.n_unassigned)])
            if name == "hard":
                hard = (r["ll"].tobytes(), r["pair_ll"].tobytes())
            if name == "one_hot":
                rec[name]["sums_equal_hard"] = bool((r["ll"].tobytes(), r["pair_ll"].tobytes()) == hard)
                assert rec[name]["sums_equal_hard"], D
            del r
        out["runs"].append(rec)
    g.close()
    print(json.dumps(dict(config="donor_gp", **out)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg4", choices=sorted(CFGS))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--donors", default="8,32,64")
    ap.add_argument("--parent-lib", default=None, help="libcellector_hip.so built from the parent commit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=("gp", "em"))
    args = ap.parse_args()
    donors = [int(x) for x in args.donors.split(",")]
    if args.child == "gp":
        return child_gp(args.cfg, donors)
    if args.child == "em":
        return child_em(args.cfg, args.reps)
    jobs = [("gp", None), ("em", None)] + ([("em", args.parent_lib), ("em", None), ("em", args.parent_lib)] if args.parent_lib else [])
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
        if name == "gp":
            lines = LINE.findall(r.stderr)
            assert len(lines) == 2 * len(VARIANTS) * len(rec["runs"]), len(lines)
            for i, run in enumerate(rec["runs"]):  # (two calls of each variant per D: the second counts)
                for j, v in enumerate(VARIANTS):
                    m = lines[2 * (len(VARIANTS) * i + j) + 1]
                    assert int(m[1]) == run["D"] and bool(m[0]) == (v != "hard")
                    run[v].update(singlet_pass_ms=float(m[2]), pair_pass_ms=float(m[3]), whole_call_s=float(m[4]))
                for v in VARIANTS[1:]:
                    run[v].update(singlet_over_hard=run[v]["singlet_pass_ms"] / run["hard"]["singlet_pass_ms"],
                                  pair_over_hard=run[v]["pair_pass_ms"] / run["hard"]["pair_pass_ms"])
        if lib:
            rec["library"] = "parent commit"
        print(json.dumps(rec), flush=True)
        runs.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/donor_gp_cost.py", runs=runs), f, indent=1)


if __name__ == "__main__":
    main()
