#!/usr/bin/env python3
"""Cost of the joined ingests (needs an MI355X).

  python tools/join_cost.py [--reps 5] [--parent-lib PATH/libcellector_hip.so] [--cfg4] [--out profiles/NAME.json]

coo    cfg3 (100 000 loci x 200 000 cells, 1 %): the synthetic matrix' staged COO split on the host into an alt stream (the entries
       with alt > 0) and a depth stream (every entry, alt + ref), through cellector_ingest_coo_joined (mode DEPTH), second of two
       calls.  From the library's line under CELLECTOR_TIMING=1: the phases and the join kernels' GPU time between their two
       events; floor_ms = the bytes the two passes move (pass 1 reads 8 B per entry of both streams, pass 2 12 B, and writes 12 B per
       staged entry) over 6.3 TB/s.  whole_call_s against cellector_ingest_coo of the same matrix in the same process; the same
       with the depth stream shuffled, which adds the sort.
text   50 000 x 50 000 at 1 %: the pair written by cellector_write_staged_mtx (complete: every key in both files, ascending),
       cellector_load_mtx_joined (mode REF) against cellector_load_mtx of the same two files, alternating, best of three each.
em     the default EM iteration (cfg4), ms per iteration, best of --reps in a fresh process, this library and with --parent-lib
       the parent commit's, alternating three times: the parent's own spread stands beside the difference.
bench  bench.py --gpus 1 --steps 20 --warmup 5 of this commit.
cfg4   (--cfg4) the coo measurement at 2e9 entries per side, only where the host has the memory for its arrays (about 130 GB);
       otherwise the file says so.

One fresh process per measurement, one after the other; a measurement that fails ends the run (nothing is tried again)."""
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

JOIN_LINE = re.compile(r"join: tokens FIRST ([\d.]+) s, tokens SECOND ([\d.]+) s, checks ([\d.]+) s, sorts ([\d.]+) s, join ([\d.]+) s "
                       r"\(its kernels ([\d.]+) ms\)")
HBM_STREAM = 6.3e12  # B/s a streaming kernel reaches on this part


def child_coo(cfg):
    sys.path.insert(0, ROOT)
    import numpy as np
    from cellector_amd import Cellector
    L, N, d = CFGS[cfg]
    g = Cellector(0)
    g.ingest_synthetic(L, N, d, seed=4, minority_fraction=0.05)
    l, c, a, r = g.staged_coo()
    nz = np.flatnonzero(a)
    first, second = (l[nz], c[nz], a[nz]), (l, c, a + r)
    del nz
    out = dict(config="coo", cfg=cfg, loci=L, cells=N, entries=int(len(l)), calls=[])

    def timed(name, fn):
        walls = []
        for _ in range(2):
            t0 = time.perf_counter()
            s = fn()
            walls.append(time.perf_counter() - t0)
        rec = dict(call=name, wall_s=walls)
        if s is not None:
            rec.update(s.as_dict())
            moved = 20 * (s.n_first + s.n_second) + 12 * s.n_out
            rec.update(bytes_moved=moved, floor_ms=moved / HBM_STREAM * 1e3)
        out["calls"].append(rec)
        print("#", json.dumps(rec), file=sys.stderr, flush=True)
    timed("ingest_coo", lambda: g.ingest_coo(L, N, l, c, a, r))
    timed("ingest_coo_joined", lambda: g.ingest_coo_joined(L, N, first, second, "depth"))
    p = np.random.default_rng(1).permutation(len(l))
    second = tuple(x[p] for x in second)
    del p
    timed("ingest_coo_joined, SECOND shuffled", lambda: g.ingest_coo_joined(L, N, first, second, "depth"))
    g.close()
    print(json.dumps(out), flush=True)


def child_text(workdir):
    sys.path.insert(0, ROOT)
    from cellector_amd import Cellector
    L, N, d = CFGS["cfg2"]
    os.makedirs(workdir, exist_ok=True)
    alt, ref = os.path.join(workdir, "alt.mtx"), os.path.join(workdir, "ref.mtx")
    g = Cellector(0)
    g.ingest_synthetic(L, N, d, seed=4, minority_fraction=0.05)
    g.write_staged_mtx(alt, ref)
    out = dict(config="text", loci=L, cells=N, bytes=[os.path.getsize(alt), os.path.getsize(ref)], aligned_s=[], joined_s=[])
    for _ in range(4):  # (the first round warms the page cache and the allocation cache: not counted)
        t0 = time.perf_counter()
        g.load_mtx(alt, ref)
        out["aligned_s"].append(time.perf_counter() - t0)
        want = int(g.dims().nnz_used)
        t0 = time.perf_counter()
        s = g.load_mtx_joined(alt, ref, "ref")
        out["joined_s"].append(time.perf_counter() - t0)
        assert int(g.dims().nnz_used) == want and s.n_both == s.n_out
    g.close()
    os.remove(alt); os.remove(ref)
    out.update(entries=int(s.n_out), aligned_best_s=min(out["aligned_s"][1:]), joined_best_s=min(out["joined_s"][1:]))
    out["joined_over_aligned"] = out["joined_best_s"] / out["aligned_best_s"]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libcellector_hip.so built from the parent commit")
    ap.add_argument("--cfg4", action="store_true")
    ap.add_argument("--workdir", default="/tmp/join_cost")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=("coo", "text", "em"))
    ap.add_argument("--cfg", default="cfg3")
    args = ap.parse_args()
    if args.child == "coo":
        return child_coo(args.cfg)
    if args.child == "text":
        return child_text(args.workdir)
    if args.child == "em":
        return child_em("cfg4", args.reps)
    jobs = [("coo", None, "cfg3"), ("text", None, "cfg2")]
    notes = {}
    if args.cfg4:
        avail = next(int(x.split()[1]) for x in open("/proc/meminfo") if x.startswith("MemAvailable")) * 1024
        need = 130 << 30  # four staged arrays of 2e9 u32, the two streams, one shuffled copy
        if avail >= need:
            jobs.append(("coo", None, "cfg4"))
        else:
            notes["cfg4"] = f"not measured: the COO route's host arrays need about {need >> 30} GB, the host has {avail >> 30} GB available"
    else:
        notes["cfg4"] = "not measured in this run (--cfg4 not given): no figure is extrapolated"
    jobs += [("em", None, "cfg4")] + ([("em", args.parent_lib, "cfg4"), ("em", None, "cfg4"), ("em", args.parent_lib, "cfg4"), ("em", None, "cfg4"),
                                       ("em", args.parent_lib, "cfg4")] if args.parent_lib else [])
    runs = []
    for name, lib, cfg in jobs:
        env = dict(os.environ)
        env.pop("CELLECTOR_HIP_LIB", None)
        env["CELLECTOR_TIMING"] = "1"
        if lib:
            env["CELLECTOR_HIP_LIB"] = os.path.abspath(lib)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--cfg", cfg, "--reps", str(args.reps), "--workdir", args.workdir]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1100, env=env)
        if r.returncode != 0:
            sys.exit(f"{name} {cfg} failed (status {r.returncode}); stopping\n{r.stderr[-3000:]}")
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        if name == "coo":
            lines = JOIN_LINE.findall(r.stderr)  # two calls per joined measurement: the second counts
            for call, m in zip(rec["calls"][1:], lines[1::2]):
                tf, ts, ck, so, jn, ms = (float(x) for x in m)
                call.update(tokens_first_s=tf, tokens_second_s=ts, checks_s=ck, sorts_s=so, join_s=jn, join_kernels_ms=ms,
                            join_kernels_over_floor=ms / call["floor_ms"], over_ingest_coo=call["wall_s"][1] / rec["calls"][0]["wall_s"][1])
        if name == "text":
            rec["joined_timing_lines"] = [dict(zip(("tokens_first_s", "tokens_second_s", "checks_s", "sorts_s", "join_s", "join_kernels_ms"),
                                                   (float(x) for x in m))) for m in JOIN_LINE.findall(r.stderr)]
        if lib:
            rec["library"] = "parent commit"
        print(json.dumps(rec), flush=True)
        runs.append(rec)
    bench = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], capture_output=True,
                           text=True, timeout=1100)
    if bench.returncode != 0:
        sys.exit(f"bench.py failed (status {bench.returncode})\n{bench.stderr[-2000:]}")
    runs.append(dict(config="bench.py --gpus 1 --steps 20 --warmup 5", result=json.loads(bench.stdout.strip().splitlines()[-1])))
    print(json.dumps(runs[-1]), flush=True)
    em = [r for r in runs if r.get("config") == "em_iteration"]
    if args.parent_lib and em:
        ours = [r["ms_min"] for r in em if r.get("library") != "parent commit"]
        theirs = [r["ms_min"] for r in em if r.get("library") == "parent commit"]
        med = lambda v: sorted(v)[len(v) // 2]
        notes["em_iteration"] = dict(this_commit_best_ms=ours, parent_best_ms=theirs, this_median=med(ours), parent_median=med(theirs),
                                     parent_spread_ms=max(theirs) - min(theirs), difference_ms=med(ours) - med(theirs),
                                     inside_parent_spread=abs(med(ours) - med(theirs)) <= max(theirs) - min(theirs))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/join_cost.py", notes=notes, runs=runs), f, indent=1)


if __name__ == "__main__":
    main()
