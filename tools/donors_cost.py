#!/usr/bin/env python3
"""Cost of the donor calls on a resident matrix (needs an MI355X), D = 8, 32 and 64 donors of random genotypes.

  python tools/donors_cost.py [--cfg cfg4] [--reps 5] [--donors 8,32,64] [--parent-lib PATH/libcellector_hip.so]
                              [--out profiles/NAME.json]

Measured per D, from the library's own lines under CELLECTOR_TIMING=1 (HIP events around the launches; no kernel id of
cellector_kernel_time is used), the second of two calls:
  singlet_pass_ms / pair_pass_ms   GPU time of k_donor_e<DP, false> and k_donor_e<DP, true> (the pair pass with its softmax tail)
  whole_call_s                     wall time of the whole cellector_donor_posteriors inside the library: the upload of gt, the
                                   packing, the tables, both passes and the copies of every output to the host
  generic_e_step_ms                GPU time of cellector_cluster_e_step at J = D columns (K = D / R clusters x R restarts: 8 x 1,
                                   16 x 2, 16 x 4) on tables expanded from the same genotypes, tab[l][d] = tab1[l][g_d(l)]: the route
                                   that existed before, with the singlet sums only (it has no pair hypothesis); its s equals the
                                   donor call's ll bit for bit, which the tool asserts
  singlet_over_generic             singlet_pass_ms / generic_e_step_ms
  table_bytes_per_entry            what one entry's wave reads of tables and genotypes: 16 D generic; W 8 + 16 per distinct
                                   genotype among the D donors (at most 64) for the singlet pass
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
CFGS = {"cfg2": (50_000, 50_000, 0.01), "cfg3": (100_000, 200_000, 0.01), "cfg4": (200_000, 1_000_000, 0.01)}  # loci, cells, density
SPLIT = {8: (8, 1), 32: (16, 2), 64: (16, 4)}  # D -> (K, R) of the generic E step
DONOR_LINE = re.compile(r"donors: D (\d+) singlet pass ([\d.]+) ms, pair pass ([\d.]+) ms, whole call ([\d.]+) s")
E_LINE = re.compile(r"cluster_e_step: J (\d+) E step ([\d.]+) ms")


def child_donors(cfg, donors):
    sys.path.insert(0, ROOT)
    import numpy as np
    from cellector_amd import Cellector
    L, N, d = CFGS[cfg]
    g = Cellector(0)
    g.load_synthetic(L, N, d, seed=4, minority_fraction=0.05)
    TL, Lu = int(g.dims().total_loci), int(g.dims().loci_used)
    ids = g.locus_ids().astype(np.int64)
    out = dict(cfg=cfg, cells=N, loci=L, loci_used=Lu, entries=int(g.dims().nnz_used), runs=[])
    for D in donors:
        gt = np.random.default_rng(D).choice(4, (D, TL), p=[0.4, 0.3, 0.2, 0.1]).astype(np.uint8)
        walls = []
        for _ in range(2):
            t0 = time.perf_counter()
            r = g.donor_posteriors(gt, tables=True)
            walls.append(time.perf_counter() - t0)
        K, R = SPLIT[D]
        tab = np.ascontiguousarray(r["tab1"][np.arange(Lu)[:, None], gt[:, ids].T])  # [L, D, 2]
        for _ in range(2):
            e = g.cluster_e_step(tab, K, R)
        same = e["s"].tobytes() == r["ll"].tobytes()
        s = r["summary"]
        out["runs"].append(dict(D=D, generic_K=K, generic_R=R, wall_s=walls, generic_s_equals_ll=bool(same),
                                status=[int(s.n_singlet), int(s.n_doublet), int(s.n_ambiguous), int(s.n_unassigned)],
                                table_bytes_per_entry=dict(generic=16 * D, singlet_at_most=8 * ((D + 31) // 32) + 64,
                                                           pair_at_most=8 * ((D + 31) // 32) + 4 * 16)))
        del r, e, tab
    g.close()
    print(json.dumps(dict(config="donors", **out)), flush=True)


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
    ap.add_argument("--donors", default="8,32,64")
    ap.add_argument("--parent-lib", default=None, help="libcellector_hip.so built from the parent commit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=("donors", "em"))
    args = ap.parse_args()
    donors = [int(x) for x in args.donors.split(",")]
    if any(D not in SPLIT for D in donors):
        sys.exit(f"--donors: one of {sorted(SPLIT)}")
    if args.child == "donors":
        return child_donors(args.cfg, donors)
    if args.child == "em":
        return child_em(args.cfg, args.reps)
    jobs = [("donors", None), ("em", None)] + ([("em", args.parent_lib), ("em", None), ("em", args.parent_lib)] if args.parent_lib else [])
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
        if name == "donors":
            dl, el = DONOR_LINE.findall(r.stderr), E_LINE.findall(r.stderr)
            for i, run in enumerate(rec["runs"]):  # (two calls of each per D: the second counts)
                m, e = dl[2 * i + 1], el[2 * i + 1]
                assert int(m[0]) == run["D"] == int(e[0])
                run.update(singlet_pass_ms=float(m[1]), pair_pass_ms=float(m[2]), whole_call_s=float(m[3]), generic_e_step_ms=float(e[1]),
                           singlet_over_generic=float(m[1]) / float(e[1]))
        if lib:
            rec["library"] = "parent commit"
        print(json.dumps(rec), flush=True)
        runs.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/donors_cost.py", runs=runs), f, indent=1)


if __name__ == "__main__":
    main()
