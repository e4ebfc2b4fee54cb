#!/usr/bin/env python3
"""Cost of the donor panel on a resident matrix (needs an MI355X): cellector_donor_panel at D = 64, 256, 1024, 4096 donors of random
genotypes, shortlist 8, against the route that existed before, ceil(D / 64) calls of cellector_donor_posteriors on 64-donor slices of
the same gt, in the same process.

  python tools/donor_panel_cost.py [--cfg cfg4] [--rounds 3] [--donors 64,256,1024,4096] [--reps 5]
                                   [--parent-lib PATH/libcellector_hip.so] [--parent-tree DIR] [--out profiles/NAME.json]

One process holds the matrix; per round and per D the panel call and then the chunked calls run one after the other (interleaved
rounds; the median and the minimum over the rounds are reported, every round is listed).  GPU time comes from the library's own lines
under CELLECTOR_TIMING=1 (HIP events around the launches):
  panel_cell_pass_ms      k_donor_panel<Q>: the singlet sums of all D donors, the shortlist, the pair walk and the chain, one launch
                          (the kernel is fused: its singlet phase has no events of its own; panel_cell_pass_m1_ms, the same launch at
                          shortlist 1, bounds it from above)
  panel_whole_call_s      wall time of the whole call inside the library: the slab uploads, the packing, the tables, the pass, the copies
  chunked_singlet_ms      the sum over the slices of k_donor_e<64, false>'s GPU time; chunked_pair_ms likewise of <64, true>
  chunked_whole_call_s    the sum of the slices' whole calls
  cell_pass_ratio         (chunked_singlet_ms + chunked_pair_ms) / panel_cell_pass_ms; singlet_ratio = chunked_singlet_ms /
                          panel_cell_pass_m1_ms: above 1 = the panel pass is faster per donor
  pairs_per_s             entries x D / panel_cell_pass_m1_ms: (entry, donor) pairs per second
In the first round the tool asserts that the panel's ll equals the slices' ll bit for bit, column for column, at every D whose
ll [cells, D] stays below --check-bytes (4 GB) on the host; ll_checked lists those D.  The chunked calls ask for no other output, so
their whole-call time holds no copies the panel call does not make either.
em_iteration: the default EM iteration of the benchmark loop with this library and, with --parent-lib, with the parent commit's, each in
a process of its own, alternating (ms per iteration, every repetition listed).
bench: with --parent-tree, `bench.py --gpus 1 --steps 20 --warmup 5` of this tree and of a checkout of the parent commit (built),
alternating, two runs each; ms_per_step of every run.

A measurement that fails ends the run (nothing is tried again).
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFGS = {"cfg2": (50_000, 50_000, 0.01), "cfg3": (100_000, 200_000, 0.01), "cfg4": (200_000, 1_000_000, 0.01)}  # loci, cells, density
PANEL_LINE = re.compile(r"donor_panel: D (\d+) M (\d+) packing and tables ([\d.]+) ms, cell pass ([\d.]+) ms, whole call ([\d.]+) s")
DONOR_LINE = re.compile(r"donors: D (\d+) singlet pass ([\d.]+) ms, pair pass ([\d.]+) ms, whole call ([\d.]+) s")


def child_panel(cfg, donors, rounds, check_bytes):
    sys.path.insert(0, ROOT)
    import ctypes
    import numpy as np
    from cellector_amd import Cellector
    L, N, d = CFGS[cfg]
    g = Cellector(0)
    g.load_synthetic(L, N, d, seed=4, minority_fraction=0.05)
    TL = int(g.dims().total_loci)
    out = dict(cfg=cfg, cells=N, loci=L, loci_used=int(g.dims().loci_used), entries=int(g.dims().nnz_used), donors=donors, rounds=rounds,
               ll_checked=[], calls=[])
    codes = np.array([0, 0, 0, 0, 1, 1, 1, 2, 2, 3], np.uint8)  # (0.4 / 0.3 / 0.2 / 0.1, drawn as bytes: 4096 x 200 000 calls)
    gts = {D: codes[np.random.default_rng(D).integers(0, 10, (D, TL), dtype=np.uint8)] for D in donors}
    chunk_ll = np.zeros((N, 64), np.float64)

    def chunk(gt64, want_ll):
        """cellector_donor_posteriors on a slice, asking for ll alone or for nothing: the passes run either way"""
        gt64 = np.ascontiguousarray(gt64)
        none = [None] * 18
        if want_ll:
            none[4] = chunk_ll.ctypes.data_as(ctypes.c_void_p)  # (after p, log_prior, anchor, mask)
        g._ck(g._lib.cellector_donor_posteriors(g.h, gt64.ctypes.data_as(ctypes.c_void_p), gt64.shape[0], *none))

    g.donor_panel(gts[donors[0]][:64], 8)  # (warm: the first launch of a process pays for the code object)
    for rnd in range(rounds):
        for D in donors:
            gt = gts[D]
            check = rnd == 0 and N * D * 8 <= check_bytes
            r = g.donor_panel(gt, 8, ll=check)
            g.donor_panel(gt, 1)
            out["calls"] += [["panel", D, 8], ["panel", D, 1]]
            for s0 in range(0, D, 64):
                chunk(gt[s0:s0 + 64], check)
                out["calls"].append(["chunk", D, s0])
                if check:
                    assert r["ll"][:, s0:s0 + 64].tobytes() == chunk_ll.tobytes(), f"D {D}: the panel's singlet sums differ from the slice at {s0}"
            if check:
                out["ll_checked"].append(D)
            if rnd == 0:
                s = r["summary"]
                out.setdefault("status", {})[D] = [int(s.n_singlet), int(s.n_doublet), int(s.n_ambiguous), int(s.n_unassigned), int(s.n_present)]
            del r
    g.close()
    print(json.dumps(dict(config="donor_panel", **out)), flush=True)


def child_em(cfg, reps):
    sys.path.insert(0, ROOT)
    import time
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
    print(json.dumps(dict(config="em_iteration", cfg=cfg, library="parent commit" if os.environ.get("CELLECTOR_HIP_LIB") else "this commit",
                          iterations=n, ms_per_iteration=per_iter[1:], ms_min=min(per_iter[1:]), ms_max=max(per_iter[1:]))), flush=True)


def summarise(rec, stderr):
    """the timing lines of the child, in the order of its calls (the warm-up call's line first)"""
    lines = []
    for ln in stderr.splitlines():
        m = PANEL_LINE.search(ln)
        if m:
            lines.append(("panel", int(m.group(1)), float(m.group(4)), float(m.group(5)), float(m.group(3))))
        m = DONOR_LINE.search(ln)
        if m:
            lines.append(("chunk", int(m.group(1)), float(m.group(2)), float(m.group(3)), float(m.group(4))))
    lines = lines[1:]
    assert len(lines) == len(rec["calls"]), (len(lines), len(rec["calls"]))
    per = {D: [] for D in rec["donors"]}
    cur = None
    for (kind, D, arg), ln in zip(rec["calls"], lines):
        assert ln[0] == kind
        if kind == "panel" and arg == 8:
            cur = dict(panel_cell_pass_ms=ln[2], panel_whole_call_s=ln[3], panel_pack_tables_ms=ln[4], chunked_singlet_ms=0.0,
                       chunked_pair_ms=0.0, chunked_whole_call_s=0.0)
            per[D].append(cur)
        elif kind == "panel":
            cur["panel_cell_pass_m1_ms"] = ln[2]
        else:
            cur["chunked_singlet_ms"] += ln[2]
            cur["chunked_pair_ms"] += ln[3]
            cur["chunked_whole_call_s"] += ln[4]
    rec["results"] = []
    for D, rounds in per.items():
        for r in rounds:
            r["cell_pass_ratio"] = (r["chunked_singlet_ms"] + r["chunked_pair_ms"]) / r["panel_cell_pass_ms"]
            r["singlet_ratio"] = r["chunked_singlet_ms"] / r["panel_cell_pass_m1_ms"]
            r["pairs_per_s"] = rec["entries"] * D / (r["panel_cell_pass_m1_ms"] * 1e-3)
        keys = sorted(rounds[0])
        rec["results"].append(dict(D=D, Q=max(1, 1 << (((D + 63) // 64) - 1).bit_length()), rounds=rounds,
                                   median={k: statistics.median(r[k] for r in rounds) for k in keys},
                                   minimum={k: min(r[k] for r in rounds) for k in keys}))
    del rec["calls"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg4", choices=sorted(CFGS))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--donors", default="64,256,1024,4096")
    ap.add_argument("--parent-lib", default=None, help="libcellector_hip.so built from the parent commit")
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit, built: bench.py runs beside it")
    ap.add_argument("--check-bytes", type=float, default=4e9, help="the largest ll [cells, D] the bit check holds on the host")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=("panel", "em"))
    args = ap.parse_args()
    donors = [int(x) for x in args.donors.split(",")]
    if args.child == "panel":
        return child_panel(args.cfg, donors, args.rounds, args.check_bytes)
    if args.child == "em":
        return child_em(args.cfg, args.reps)
    jobs = [("panel", None), ("em", None)] + ([("em", args.parent_lib), ("em", None), ("em", args.parent_lib)] if args.parent_lib else [])
    runs = []
    for name, lib in jobs:
        env = dict(os.environ)
        env.pop("CELLECTOR_HIP_LIB", None)
        env["CELLECTOR_TIMING"] = "1"
        if lib:
            env["CELLECTOR_HIP_LIB"] = os.path.abspath(lib)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--cfg", args.cfg, "--reps", str(args.reps), "--donors", args.donors,
               "--rounds", str(args.rounds), "--check-bytes", str(args.check_bytes)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1100, env=env)
        if r.returncode != 0:
            sys.exit(f"{name} {args.cfg} failed (status {r.returncode}); stopping\n{r.stderr[-2000:]}")
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        if name == "panel":
            summarise(rec, r.stderr)
        print(json.dumps(rec), flush=True)
        runs.append(rec)
    if args.parent_tree:
        env = {k: v for k, v in os.environ.items() if k not in ("CELLECTOR_HIP_LIB", "CELLECTOR_TIMING")}
        for tree, name in [(ROOT, "this commit"), (os.path.abspath(args.parent_tree), "parent commit")] * 2:
            r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=tree, capture_output=True,
                               text=True, timeout=600, env=env)
            if r.returncode != 0:
                sys.exit(f"bench.py of {name} failed (status {r.returncode}); stopping\n{r.stderr[-2000:]}")
            b = json.loads(r.stdout.strip().splitlines()[-1])
            rec = dict(config="bench", library=name, steps=b["steps"], warmup=b["warmup"], ms_per_step=b["ms_per_step"], value=b["value"],
                       workload=b["config"]["workload"])
            print(json.dumps(rec), flush=True)
            runs.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/donor_panel_cost.py", runs=runs), f, indent=1)


if __name__ == "__main__":
    main()
