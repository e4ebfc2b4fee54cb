#!/usr/bin/env python3
"""Cost of cellector_restage at cfg4 (bench.py's synthetic 200k loci x 10^6 cells at 1 %; needs an MI355X), engine 2.
Every figure is the median of --runs (at least five) wall times around the synchronous call, with the minimum and maximum beside
it; one more run in front is a warm-up and is dropped.  Each run starts from a fresh cellector_ingest_synthetic + finish, which is
itself figure (iv):

  peel         (i) cellector_restage dropping the fixed point's exclusion set, (iii) the cellector_ingest_finish behind it;
               the phases of the call as the library reports them under CELLECTOR_TIMING=1; the device memory in use while the
               warm-up call runs, sampled every millisecond by a thread beside it (hipMemGetInfo): the peak of (i);
  thin         (ii) the restage at rate 0.3 with all cells, (iii) the finish behind it;
  load         (iv) cellector_ingest_synthetic and cellector_ingest_finish of the full matrix, each run of the two above;
  traffic      (v) bytes the passes must move — 4 B per entry read by the count pass, 12 B read and 12 B per surviving entry
               written by the write pass (thin: 4 B read and 4 B written per entry, the two counts where they are) — over the time
               of those passes and over the whole call;
  parent       (vi) with --parent-lib PATH/libcellector_hip.so (the parent commit's build): the default EM iteration (median of five
               device-synchronised iterations after a warm-up of four) of that library and of this one in alternating processes,
               --repeats of each; this commit's median must not exceed the parent's by more than the spread of the parent's repeats.

  python tools/restage_cost.py [--cfg cfg4] [--runs 5] [--parent-lib PATH] [--repeats 3] [--out profiles/r9_restage_cost.json]

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
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFGS = {"cfg1": (2_000, 1_000, 0.1), "cfg3": (100_000, 200_000, 0.01), "cfg4": (200_000, 1_000_000, 0.01)}  # loci, cells, density
WARMUP, TIMED = 4, 5
CHILD_LIMIT_S = 420


def _stat(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=xs)


class MemSampler(threading.Thread):
    """device memory in use, sampled while a synchronous library call runs (ctypes releases the GIL)"""

    def __init__(self, torch):
        super().__init__(daemon=True)
        self.torch, self.stop, self.peak = torch, False, 0

    def run(self):
        while not self.stop:
            free, total = self.torch.cuda.mem_get_info()
            self.peak = max(self.peak, total - free)
            time.sleep(0.001)


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
        fn(*a, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    if what == "default":
        g.set_option("keep_coo", 0)
        g.load_synthetic(L, N, d, seed=4, minority_fraction=0.05)
        ms = [timed(g.em_iteration, 5.0) for _ in range(WARMUP + TIMED)][WARMUP:]
        res.update(iteration_ms=ms, iteration_ms_median=statistics.median(ms))
    else:
        ingest, finish, restage, refinish, used, peaks = [], [], [], [], [], []
        for i in range(1 + runs):
            ingest.append(timed(g.ingest_synthetic, L, N, d, 4, 0.05))
            finish.append(timed(g.ingest_finish))
            keep = None
            if what == "peel":
                g.run(5.0, 30)
                keep = g.excluded() == 0
            torch.cuda.synchronize()
            free, total = torch.cuda.mem_get_info()
            used.append(total - free)
            sampler = MemSampler(torch) if i == 0 else None  # (beside the warm-up call only: the timed calls run alone)
            if sampler:
                sampler.start()
            restage.append(timed(g.restage, keep, 0.3 if what == "thin" else 0.0, 4))
            if sampler:
                sampler.stop = True
                sampler.join()
                peaks.append(sampler.peak)
            n = ctypes.c_uint64(0)
            g._ck(g._lib.cellector_staged_coo(g.h, ctypes.byref(n), None, None, None, None, 0))
            refinish.append(timed(g.ingest_finish))
            res.update(cells_after=int(g.dims().total_cells), loci_used_after=int(g.dims().loci_used), entries_after=int(n.value),
                       cells_kept=int(N if keep is None else keep.sum()))
        for k, v in (("ingest_synthetic_ms", ingest), ("ingest_finish_ms", finish), ("restage_ms", restage),
                     ("finish_after_restage_ms", refinish)):
            res[k] = _stat(v[1:])
        res.update(load_ms=_stat([a + b for a, b in zip(ingest[1:], finish[1:])]),
                   restage_plus_finish_ms=_stat([a + b for a, b in zip(restage[1:], refinish[1:])]),
                   device_bytes_in_use_before_restage=max(used), device_bytes_peak_during_restage=max(peaks))
    g.close()
    print("RESULT " + json.dumps(res), flush=True)


def run_child(what, cfg, runs, lib=None):
    env = dict(os.environ)
    env.pop("CELLECTOR_HIP_LIB", None)
    if what != "default":
        env["CELLECTOR_TIMING"] = "1"  # the phases of the restage on stderr (the ingest's too: a few device synchronisations more)
    if lib:
        env["CELLECTOR_HIP_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, "--cfg", cfg, "--runs", str(runs)], env=env,
                       capture_output=True, text=True, timeout=CHILD_LIMIT_S)
    if r.returncode != 0:
        sys.exit(f"restage_cost: the '{what}' measurement failed ({r.returncode}):\n{r.stdout}\n{r.stderr[-4000:]}")
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    phases = {}  # "[timing]   restage: <phase>   <seconds> s", one per call; the warm-up call's dropped
    for name, sec in re.findall(r"^\[timing\]\s+restage: (.+?)\s+([0-9.]+) s$", r.stderr, flags=re.M):
        phases.setdefault(name, []).append(float(sec) * 1e3)
    res["restage_phases_ms"] = {k: _stat(v[1:]) for k, v in phases.items() if len(v) > 1}
    print(f"[{'parent' if lib else 'this'} {what}] done", file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg4", choices=sorted(CFGS))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=["default", "peel", "thin"])
    args = ap.parse_args()
    if args.runs < 5:
        sys.exit("restage_cost: --runs must be at least 5")
    if args.child:
        return child(args.child, args.cfg, args.runs)
    L, N, d = CFGS[args.cfg]
    res = dict(tool="tools/restage_cost.py", cfg=args.cfg, cells=N, loci=L, density=d, engine=2, runs=args.runs)
    peel = run_child("peel", args.cfg, args.runs)
    thin = run_child("thin", args.cfg, args.runs)
    res.update(peel=peel, thin=thin)
    n_in = thin["entries_after"]  # (thinning keeps every entry: the staged entries of the full matrix)
    res["entries"] = n_in
    for name, r, gb in (("peel", peel, (4.0 * n_in + 12.0 * n_in + 12.0 * peel["entries_after"]) / 1e9),
                        ("thin", thin, (4.0 * n_in + 4.0 * n_in) / 1e9)):
        passes = r["restage_phases_ms"].get("count + scan + write" if name == "peel" else "thin")
        res[name + "_traffic"] = dict(algorithmic_gb=gb, gb_per_s_whole_call=gb / (r["restage_ms"]["median"] / 1e3),
                                      gb_per_s_passes=gb / (passes["median"] / 1e3) if passes else None)
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
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
