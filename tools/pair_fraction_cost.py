#!/usr/bin/env python3
"""Cost of the donor pair fractions on a resident matrix (needs an MI355X), D = 8 donors of random genotypes, every cell under a pair.

  python tools/pair_fraction_cost.py [--cfg cfg4] [--reps 5] [--grids 9,17,32] [--parent-lib PATH/libcellector_hip.so]
                                     [--out profiles/NAME.json]

Measured, from the library's own lines under CELLECTOR_TIMING=1 (HIP events around the launches; no kernel id of
cellector_kernel_time is used) and the wall clock around the calls, the second of two calls:
  pair_pass_ms          per G: GPU time of k_pair_fraction_e<GP> of one cellector_donor_pair_fractions
  pair_call_s           per G: wall time of the whole call inside the library (the uploads, the packing, the tables, the pass and the
                        copies of the outputs asked for: every per-cell output and ll)
  ambient_pass_ms       per G: GPU time of k_ambient_e<GP> and its folds at the same G on the same ctx, every cell under donor pair_a.
                        The two passes read the same bytes per entry (one table row of 16 G bytes); the pair pass extracts a second
                        genotype and indexes a table four times as large, the ambient pass folds the cells' rows afterwards
  pair_over_ambient     pair_pass_ms / ambient_pass_ms
  table_bytes           256 G bytes per used locus: what the cell pass reads its rows from
  identity              the columns at f = 1 and f = 0.5 (where the grid holds them) are ll[c][a] and pair_ll[c][b] of one
                        cellector_donor_posteriors under anchor = pair_a, bit for bit; the tool asserts it
  em_iteration          the default EM iteration of the benchmark loop (ms per iteration, every repetition listed), with this library
                        and, with --parent-lib, with the library of the parent commit in a process of its own, alternating, five
                        processes each

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

D = 8
PAIR_LINE = re.compile(r"pair fractions: D (\d+) G (\d+) cell pass ([\d.]+) ms, whole call ([\d.]+) s")
AMB_LINE = re.compile(r"ambient: S (\d+) G (\d+) cell pass and folds ([\d.]+) ms, whole call ([\d.]+) s")


def child_pairs(cfg, grids):
    sys.path.insert(0, ROOT)
    import numpy as np
    from cellector_amd import Cellector
    L, N, d = CFGS[cfg]
    g = Cellector(0)
    g.load_synthetic(L, N, d, seed=4, minority_fraction=0.05)
    TL, Lu = int(g.dims().total_loci), int(g.dims().loci_used)
    gt = np.random.default_rng(D).choice(4, (D, TL), p=[0.4, 0.3, 0.2, 0.1]).astype(np.uint8)
    c = np.arange(N)
    a = (c % D).astype(np.uint8)
    b = ((a + 1 + (c // D) % (D - 1)) % D).astype(np.uint8)
    dp = g.donor_posteriors(gt, anchor=a)
    s_a, p_b = dp["ll"][c, a].copy(), dp["pair_ll"][c, b].copy()
    del dp
    out = dict(cfg=cfg, cells=N, loci=L, loci_used=Lu, entries=int(g.dims().nnz_used), donors=D, runs=[])
    for G in grids:
        frac = np.arange(G) / float(G - 1)
        walls = []
        for _ in range(2):
            t0 = time.perf_counter()
            r = g.donor_pair_fractions(gt, a, b, frac)
            walls.append(time.perf_counter() - t0)
        same = r["ll"][:, G - 1].tobytes() == s_a.tobytes()
        if G % 2:
            same = same and r["ll"][:, G // 2].tobytes() == p_b.tobytes()
        s = r["summary"]
        kinds = dict(balanced=int(s.n_balanced), toward_a=int(s.n_toward_a), toward_b=int(s.n_toward_b), flat=int(s.n_flat), none=int(s.n_none))
        del r
        for _ in range(2):
            g.ambient_profile(gt, a, frac * 0.5)
        out["runs"].append(dict(G=G, pair_wall_s=walls, identity=bool(same), kinds=kinds, table_bytes=256 * G * Lu))
        assert same, G
    g.close()
    print(json.dumps(dict(config="pair_fractions", **out)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg4", choices=sorted(CFGS))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--grids", default="9,17,32")
    ap.add_argument("--parent-lib", default=None, help="libcellector_hip.so built from the parent commit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=("pairs", "em"))
    args = ap.parse_args()
    grids = [int(x) for x in args.grids.split(",")]
    if any(G < 4 or G > 32 for G in grids):
        sys.exit("--grids: values in 4..32")
    if args.child == "pairs":
        return child_pairs(args.cfg, grids)
    if args.child == "em":
        return child_em(args.cfg, args.reps)
    jobs = [("pairs", None)] + ([("em", lib) for _ in range(5) for lib in (None, args.parent_lib)] if args.parent_lib else [("em", None)])
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
        if name == "pairs":
            pl, al = PAIR_LINE.findall(r.stderr), AMB_LINE.findall(r.stderr)
            for i, run in enumerate(rec["runs"]):  # (two calls per G: the second counts)
                m, am = pl[2 * i + 1], al[2 * i + 1]
                assert int(m[1]) == run["G"] == int(am[1])
                run.update(pair_pass_ms=float(m[2]), pair_call_s=float(m[3]), ambient_pass_ms=float(am[2]),
                           pair_over_ambient=float(m[2]) / float(am[2]))
        if lib:
            rec["library"] = "parent commit"
        print(json.dumps(rec), flush=True)
        runs.append(rec)
    if args.parent_lib:
        best = {k: min(r["ms_min"] for r in runs if r["config"] == "em_iteration" and (r["library"] == "parent commit") == (k == "parent"))
                for k in ("this", "parent")}
        spread = [r["ms_min"] for r in runs if r["config"] == "em_iteration" and r["library"] == "parent commit"]
        runs.append(dict(config="em_summary", best_ms_this=best["this"], best_ms_parent=best["parent"], parent_process_min_ms=min(spread),
                         parent_process_max_ms=max(spread)))
        print(json.dumps(runs[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/pair_fraction_cost.py", runs=runs), f, indent=1)


if __name__ == "__main__":
    main()
