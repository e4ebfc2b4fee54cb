#!/usr/bin/env python3
"""Cost of cellector_combine at cfg4 (bench.py's synthetic 200k loci x 10^6 cells at 1 %; needs an MI355X), engine 2:
a 50 000-cell synthetic second matrix (seed 5) merged into the 10^6-cell one.  Every figure is the median of --runs (at least five)
wall times around the synchronous call, with the minimum and maximum beside it; one more run in front is a warm-up and is dropped.
Each run starts from a fresh cellector_ingest_synthetic of the large matrix; the second matrix is staged once.

  combine      (i) cellector_combine with all of src's cells, the identity map and rate 0, (ii) the cellector_ingest_finish behind
               it; the phases of the call as the library reports them under CELLECTOR_TIMING=1;
  traffic      (iii) bytes the merge must move — 12 B read per entry of either side, 12 B written per entry of the result, the
               partition's reads aside — over the time of the "merge" phase, as GB/s and as a fraction of the 6.3 TB/s the README
               calls achievable;
  upload       (iv) with --upload: the same matrix made the only way the library had before: the staged entries of both ctxs
               brought to the host, combine.combine_coo (numpy), cellector_ingest_coo of the result; every entry crosses the host
               link once more.  --upload-runs of it (default 1); the download is timed apart and NOT counted: a caller of that
               route has the arrays already.  It runs at --upload-cfg (default: --cfg) together with a combine measurement at that
               size: at cfg4 the host route holds some 150 GB of numpy arrays and its sort of 2.1e9 entries takes many minutes,
               so a smaller size can stand in and the file says which.  The combine must be faster than merge + ingest_coo in
               the same run: the tool exits non-zero otherwise;
  parent       (v) with --parent-lib PATH/libcellector_hip.so (the parent commit's build): the default EM iteration (median of five
               device-synchronised iterations after a warm-up of four) of that library and of this one in alternating processes,
               --repeats of each; this commit's median must not exceed the parent's by more than the spread of the parent's repeats.

  python tools/combine_cost.py [--cfg cfg4] [--runs 5] [--upload] [--upload-cfg cfg3] [--upload-runs 1] [--parent-lib PATH] [--repeats 3] [--out profiles/r10_combine_cost.json]

Each measurement runs in a process of its own under a time limit; the first that fails ends the run.
"""
import argparse
import ctypes
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFGS = {"cfg1": (2_000, 1_000, 0.1), "cfg3": (100_000, 200_000, 0.01), "cfg4": (200_000, 1_000_000, 0.01)}  # loci, cells, density
SRC_CELLS = {"cfg1": 50, "cfg3": 10_000, "cfg4": 50_000}
SRC_SEED = 5
WARMUP, TIMED = 4, 5
CHILD_LIMIT_S = 1500
ACHIEVABLE_GB_S = 6300.0


def _stat(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=xs)


def child(what, cfg, runs):
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
    res = dict(what=what)

    def timed(fn, *a, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(*a, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def count(x):
        n = ctypes.c_uint64(0)
        x._ck(x._lib.cellector_staged_coo(x.h, ctypes.byref(n), None, None, None, None, 0))
        return int(n.value)

    if what == "default":
        g.set_option("keep_coo", 0)
        g.load_synthetic(L, N, d, seed=4, minority_fraction=0.05)
        ms = [timed(g.em_iteration, 5.0)[0] for _ in range(WARMUP + TIMED)][WARMUP:]
        res.update(iteration_ms=ms, iteration_ms_median=statistics.median(ms))
        g.close()
    else:
        s = Cellector(0)
        s.ingest_synthetic(L, SRC_CELLS[cfg], d, SRC_SEED, 0.0)
        n_src = count(s)
        if what == "combine":
            ingest, comb, finish = [], [], []
            for _ in range(1 + runs):
                ingest.append(timed(g.ingest_synthetic, L, N, d, 4, 0.05)[0])
                n_ctx = count(g)
                comb.append(timed(g.combine, s)[0])
                finish.append(timed(g.ingest_finish)[0])
            dm = g.dims()
            res.update(entries_ctx=n_ctx, entries_src=n_src, entries_after=count(g), cells_after=int(dm.total_cells),
                       loci_used_after=int(dm.loci_used), ingest_synthetic_ms=_stat(ingest[1:]), combine_ms=_stat(comb[1:]),
                       finish_after_combine_ms=_stat(finish[1:]),
                       combine_plus_finish_ms=_stat([a + b for a, b in zip(comb[1:], finish[1:])]))
        else:  # upload: host merge of the twin + cellector_ingest_coo
            from cellector_amd import combine
            g.ingest_synthetic(L, N, d, 4, 0.05)
            t_down, (dst, src) = timed(lambda: (g.staged_coo(), s.staged_coo()))
            merge, upload = [], []
            for _ in range(runs):
                ms, t = timed(combine.combine_coo, dst, N, src, SRC_CELLS[cfg], None, None, L)
                merge.append(ms)
                upload.append(timed(g.ingest_coo, L, t[4], *t[:4])[0])
                res.update(entries_after=count(g), cells_after=int(g.dims().total_cells))
                del t
            res.update(download_ms_not_counted=t_down, host_merge_ms=_stat(merge), ingest_coo_ms=_stat(upload),
                       merge_plus_ingest_coo_ms=_stat([a + b for a, b in zip(merge, upload)]))
        s.close()
        g.close()
    print("RESULT " + json.dumps(res), flush=True)


def run_child(what, cfg, runs, lib=None):
    env = dict(os.environ)
    env.pop("CELLECTOR_HIP_LIB", None)
    if what == "combine":
        env["CELLECTOR_TIMING"] = "1"  # the phases of the combine on stderr (the ingest's too: a few device synchronisations more)
    if lib:
        env["CELLECTOR_HIP_LIB"] = lib
    # (a line on stderr every minute while the child works: the host route is silent for minutes)
    t0 = time.time()
    p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", what, "--cfg", cfg, "--runs", str(runs)], env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    while True:
        try:
            out, err = p.communicate(timeout=60)
            break
        except subprocess.TimeoutExpired:
            print(f"[{what} {cfg}] running, {time.time() - t0:.0f} s", file=sys.stderr, flush=True)
            if time.time() - t0 > CHILD_LIMIT_S:
                p.kill()
                p.communicate()
                sys.exit(f"combine_cost: the '{what}' measurement ran longer than {CHILD_LIMIT_S} s")
    r = subprocess.CompletedProcess(p.args, p.returncode, out, err)
    if r.returncode != 0:
        sys.exit(f"combine_cost: the '{what}' measurement failed ({r.returncode}):\n{r.stdout}\n{r.stderr[-4000:]}")
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    phases = {}  # "[timing]   combine: <phase>   <seconds> s", one per call; the warm-up call's dropped
    for name, sec in re.findall(r"^\[timing\]\s+combine: (.+?)\s+([0-9.]+) s$", r.stderr, flags=re.M):
        phases.setdefault(name, []).append(float(sec) * 1e3)
    if phases:
        res["combine_phases_ms"] = {k: _stat(v[1:]) for k, v in phases.items() if len(v) > 1}
    print(f"[{'parent' if lib else 'this'} {what}] done", file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg4", choices=sorted(CFGS))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--upload", action="store_true")
    ap.add_argument("--upload-cfg", default=None, choices=sorted(CFGS))
    ap.add_argument("--upload-runs", type=int, default=1)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=["default", "combine", "upload"])
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.cfg, args.runs)
    if args.runs < 5:
        sys.exit("combine_cost: --runs must be at least 5")
    L, N, d = CFGS[args.cfg]
    res = dict(tool="tools/combine_cost.py", cfg=args.cfg, cells=N, loci=L, density=d, src_cells=SRC_CELLS[args.cfg], src_seed=SRC_SEED,
               engine=2, runs=args.runs)

    def save():  # (after every stage: a later stage that fails leaves what was measured)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)

    c = run_child("combine", args.cfg, args.runs)
    res["combine"] = c
    gb = 12.0 * (c["entries_ctx"] + c["entries_src"] + c["entries_after"]) / 1e9
    merge = c["combine_phases_ms"].get("merge")
    rate = gb / (merge["median"] / 1e3) if merge else None
    res["merge_traffic"] = dict(algorithmic_gb=gb, gb_per_s_merge_phase=rate, gb_per_s_whole_call=gb / (c["combine_ms"]["median"] / 1e3),
                                fraction_of_achievable_6300_gb_s=rate / ACHIEVABLE_GB_S if rate else None)
    save()
    if args.parent_lib:
        parent, this = [], []
        for _ in range(args.repeats):  # alternating: parent, this, parent, this, ...
            parent.append(run_child("default", args.cfg, args.runs, os.path.abspath(args.parent_lib)))
            this.append(run_child("default", args.cfg, args.runs))
        pm, tm = [x["iteration_ms_median"] for x in parent], [x["iteration_ms_median"] for x in this]
        excess = statistics.median(tm) - statistics.median(pm)
        res["default_mode_parent_vs_this"] = dict(
            parent_medians_ms=pm, this_medians_ms=tm, parent_iterations_ms=[x["iteration_ms"] for x in parent],
            this_iterations_ms=[x["iteration_ms"] for x in this], parent_median_ms=statistics.median(pm),
            this_median_ms=statistics.median(tm), difference_ms=excess, parent_spread_width_ms=max(pm) - min(pm),
            excess_inside_parent_spread=bool(excess <= max(pm) - min(pm)))
    save()
    if args.upload:
        ucfg = args.upload_cfg or args.cfg
        cu = c if ucfg == args.cfg else run_child("combine", ucfg, args.runs)
        u = run_child("upload", ucfg, args.upload_runs)
        assert (u["entries_after"], u["cells_after"]) == (cu["entries_after"], cu["cells_after"]), "the two routes made other matrices"
        res["upload_route"] = dict(cfg=ucfg, cells=CFGS[ucfg][1], loci=CFGS[ucfg][0], src_cells=SRC_CELLS[ucfg],
                                   combine_at_this_cfg=cu if cu is not c else "the combine measurement above",
                                   host_merge_and_ingest_coo=u,
                                   combine_faster_than_upload_route=bool(cu["combine_ms"]["max"] < u["merge_plus_ingest_coo_ms"]["min"]))
    else:
        res["upload_route"] = "not measured in this run (--upload)"
    print(json.dumps(res), flush=True)
    save()
    # the two acceptance criteria: a run that misses one fails
    if args.upload and not res["upload_route"]["combine_faster_than_upload_route"]:
        sys.exit("combine_cost: cellector_combine is NOT faster than the host merge + cellector_ingest_coo route")
    if args.parent_lib and not res["default_mode_parent_vs_this"]["excess_inside_parent_spread"]:
        sys.exit("combine_cost: the default iteration exceeds the parent's by more than the parent's spread")


if __name__ == "__main__":
    main()
