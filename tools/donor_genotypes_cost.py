#!/usr/bin/env python3
"""Cost of the donor genotype refinement on a resident matrix (needs an MI355X): D = 8 / 16 / 32 / 64 donors with random
assignments (5 % of the cells at 255) and a one-hot prior with a tenth of its rows blanked.

  python tools/donor_genotypes_cost.py [--cfg cfg4] [--reps 5] [--parts genotypes,em] [--parent-lib PATH/libcellector_hip.so]
                                       [--out profiles/r22_donor_genotypes_cost.json]

Measured per D, every repetition listed:
  tally_pass_ms      device time of the memset of the (D + 1) x 2 planes and k_dg_tallies over the staged COO (the call's own event pair)
  posterior_pass_ms  device time of k_dg_tables and k_dg_posterior behind it
  tally_only_wall_ms the wall time of a call that asks for no output (assign in, the tally pass, nothing copied out)
  floor_over_tally   the COO stream's floor (12 B x entries at 6.3 TB/s) over the best tally pass
In the same process, on the same labels: cellector_class_genotypes with no output asked for at K = 3 and K = 16 (wall time: the 1 B
per cell of labels in, its memset and the one pass of k_genotype_tallies), beside the new call's tally_only_wall_ms at D = 3 and
D = 16.  The requirement: at D <= 16 the new pass is not slower than the old one beyond the spread of the old one's repetitions.
No shuffled COO is measured: the call needs a loaded matrix, and the build behind every way of staging leaves the staged COO
locus-major (ingest_build sorts by locus whatever order cellector_ingest_coo was given), so the library cannot present one.
  em_iteration       the default EM iteration of the benchmark loop (ms per iteration, every repetition listed), with this library and,
                     with --parent-lib, with the library of the parent commit in a process of its own, alternating

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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from class_genotypes_cost import CFGS, STREAM_BYTES_PER_ENTRY, STREAM_TBS, _best, child_em  # noqa: E402

DS = (8, 16, 32, 64)


def _measure(g, N, reps):
    import ctypes as C
    rng = np.random.default_rng(1)
    TL = g.dims().total_loci
    n = C.c_uint64(0)
    g._ck(g._lib.cellector_staged_coo(g.h, C.byref(n), None, None, None, None, 0))
    entries = int(n.value)
    floor_ms = STREAM_BYTES_PER_ENTRY * entries / (STREAM_TBS * 1e12) * 1e3
    out = dict(cells=N, loci=TL, staged_entries=entries, coo_stream_floor_ms=floor_ms)
    for D in (3,) + DS:
        assign = rng.integers(0, D, N).astype(np.uint8)
        assign[rng.random(N) < 0.05] = 255
        p = assign.ctypes.data_as(C.c_void_p)
        r = {}
        new = lambda: g._ck(g._lib.cellector_donor_genotypes(g.h, p, None, D, *([None] * 10)))
        r["tally_only_wall_ms"] = _best(new, reps)
        if D <= 16:  # the old kernel on the same labels, in the same process
            old = lambda: g._ck(g._lib.cellector_class_genotypes(g.h, p, D, 0.03, 0.99, None, None, None, None, None, None))
            r["class_genotypes_tally_wall_ms"] = _best(old, reps)
            r["new_over_old"] = min(r["tally_only_wall_ms"]) / min(r["class_genotypes_tally_wall_ms"])
            r["old_spread"] = max(r["class_genotypes_tally_wall_ms"]) / min(r["class_genotypes_tally_wall_ms"])
        if D in DS:
            gt = rng.integers(0, 4, (D, TL)).astype(np.uint8)
            prior = (gt[..., None] == np.arange(3)).astype(np.float32)
            prior[gt == 3] = np.nan
            t, q = [], []
            for _ in range(reps + 1):
                ms = g.donor_genotypes(assign, prior, timing=True)["pass_ms"]
                t.append(float(ms[0])); q.append(float(ms[1]))
            r["tally_pass_ms"], r["posterior_pass_ms"] = t[1:], q[1:]
            r["floor_over_tally"] = floor_ms / min(t[1:])
        out[f"D{D}"] = r
    return out


def child_genotypes(cfg, reps):
    sys.path.insert(0, ROOT)
    from cellector_amd import Cellector
    L, N, d = CFGS[cfg]
    g = Cellector(0)
    g.load_synthetic(L, N, d, seed=4, minority_fraction=0.05)
    out = _measure(g, N, reps)
    g.close()
    print(json.dumps(dict(config="donor_genotypes", cfg=cfg, order="as staged (locus-major)", **out)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg4", choices=sorted(CFGS))
    ap.add_argument("--parts", default="genotypes,em", help="which measurements to run: genotypes, em")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libcellector_hip.so built from the parent commit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=("genotypes", "em"))
    args = ap.parse_args()
    if args.child == "em":
        return child_em(args.cfg, args.reps)
    if args.child:
        return child_genotypes(args.cfg, args.reps)
    parts = args.parts.split(",")
    jobs = [("genotypes", args.cfg, None)] if "genotypes" in parts else []
    if "em" in parts:
        jobs += [("em", args.cfg, None)]
        if args.parent_lib:
            jobs += [("em", args.cfg, args.parent_lib), ("em", args.cfg, None), ("em", args.cfg, args.parent_lib)]
    runs = []
    for name, cfg, lib in jobs:
        env = dict(os.environ)
        env.pop("CELLECTOR_HIP_LIB", None)
        if lib:
            env["CELLECTOR_HIP_LIB"] = os.path.abspath(lib)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--cfg", cfg, "--reps", str(args.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
        if r.returncode != 0:
            sys.exit(f"{name} {cfg} failed (status {r.returncode}); stopping\n{r.stderr[-2000:]}")
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        runs.append(json.loads(line))
        if lib:
            runs[-1]["library"] = "parent commit"
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(dict(tool="tools/donor_genotypes_cost.py", runs=runs), f, indent=1)


if __name__ == "__main__":
    main()
