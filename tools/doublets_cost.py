#!/usr/bin/env python3
"""Cost of cellector_add_doublets at cfg4 (bench.py's synthetic 200k loci x 10^6 cells at 1 %; needs an MI355X),
engine 2: 50 000 synthetic doublets, majority x minority parents by synth.cell_classes, added to the 10^6-cell matrix at
--doublet-rates (default 0 and 0.5).  Every figure is the median of --runs (at least five) wall times around the synchronous call,
with the minimum and maximum beside it; one more run in front is a warm-up and is dropped.  Each run starts from a fresh
cellector_ingest_synthetic of the matrix.

  doublets     (i) cellector_add_doublets, (ii) the cellector_ingest_finish behind it; the phases of the call as the library
               reports them under CELLECTOR_TIMING=1.  After the last run the loop runs to its fixed point and the fraction of the
               new cells that cellector_assign labels `doublet` is recorded — for information only, nothing is asserted on it;
  upload       (iii) with --upload: the same matrix made the only way the library had before: the staged entries brought to the
               host, doublets.add_doublets_coo (numpy), cellector_ingest_coo of the result.  --upload-runs of it (default 1); the
               download is timed apart and NOT counted: a caller of that route has the arrays already.  It runs at --upload-cfg
               (default: --cfg) together with a device measurement at that size, at the first of --doublet-rates: at cfg4 the host
               route holds some 150 GB of numpy arrays and sorts 2.1e9 entries, so a smaller size can stand in and the file says
               which.  The device call must be faster than twin + ingest_coo in the same run: the tool exits non-zero otherwise;
  parent       (iv) with --parent-lib PATH/libcellector_hip.so (the parent commit's build): the default EM iteration (median of five
               device-synchronised iterations after a warm-up of four) of that library and of this one in alternating processes,
               --repeats of each; this commit's median must not exceed the parent's by more than the spread of the parent's repeats.

  python tools/doublets_cost.py [--cfg cfg4] [--runs 5] [--upload] [--upload-cfg cfg3] [--upload-runs 1] [--parent-lib PATH] [--repeats 3] [--out profiles/r11_doublets_cost.json]

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
PAIRS = {"cfg1": 50, "cfg3": 10_000, "cfg4": 50_000}
PAIR_SEED = 5
SEED, MINORITY = 4, 0.05
WARMUP, TIMED = 4, 5
CHILD_LIMIT_S = 1500


def _stat(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=xs)


def pairs_for(cfg):
    """majority x minority parents, by the generator's own classes"""
    import numpy as np
    from cellector_amd import synth
    cls = synth.cell_classes(CFGS[cfg][1], seed=SEED, minority_fraction=MINORITY)
    rng = np.random.default_rng(PAIR_SEED)
    return rng.choice(np.flatnonzero(cls == 0), PAIRS[cfg]), rng.choice(np.flatnonzero(cls == 1), PAIRS[cfg])


def child(what, cfg, runs, rate):
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
    res = dict(what=what, rate=rate)

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
        g.load_synthetic(L, N, d, seed=SEED, minority_fraction=MINORITY)
        ms = [timed(g.em_iteration, 5.0)[0] for _ in range(WARMUP + TIMED)][WARMUP:]
        res.update(iteration_ms=ms, iteration_ms_median=statistics.median(ms))
    elif what == "doublets":
        a, b = pairs_for(cfg)
        ingest, add, finish = [], [], []
        for _ in range(1 + runs):
            ingest.append(timed(g.ingest_synthetic, L, N, d, SEED, MINORITY)[0])
            n_ctx = count(g)
            add.append(timed(g.add_doublets, a, b, rate, SEED)[0])
            finish.append(timed(g.ingest_finish)[0])
        dm = g.dims()
        res.update(entries_ctx=n_ctx, entries_after=count(g), cells_after=int(dm.total_cells), loci_used_after=int(dm.loci_used),
                   ingest_synthetic_ms=_stat(ingest[1:]), add_doublets_ms=_stat(add[1:]), finish_after_add_doublets_ms=_stat(finish[1:]),
                   add_doublets_plus_finish_ms=_stat([x + y for x, y in zip(add[1:], finish[1:])]))
        # for information only: how many of the doublets does the doublet posterior catch at this depth?
        iters = len(g.run(5.0, 100))
        pa = g.assign(0.999, 30)["posterior_assignment"]
        new = g.cell_source() == 1
        res.update(labels_for_information=dict(iterations=iters, doublets=int(new.sum()),
                                               doublets_labelled_doublet=int((pa[new] == 2).sum()),
                                               fraction_of_doublets_labelled_doublet=float((pa[new] == 2).mean()),
                                               other_cells_labelled_doublet=int((pa[~new] == 2).sum())))
    else:  # upload: the twin on the host + cellector_ingest_coo
        from cellector_amd import doublets
        a, b = pairs_for(cfg)
        g.ingest_synthetic(L, N, d, SEED, MINORITY)
        t_down, coo = timed(g.staged_coo)
        twin, upload = [], []
        for _ in range(runs):
            ms, t = timed(doublets.add_doublets_coo, coo, N, a, b, rate, SEED)
            twin.append(ms)
            upload.append(timed(g.ingest_coo, L, t[4], *t[:4])[0])
            res.update(entries_after=count(g), cells_after=int(g.dims().total_cells))
            del t
        res.update(download_ms_not_counted=t_down, host_twin_ms=_stat(twin), ingest_coo_ms=_stat(upload),
                   twin_plus_ingest_coo_ms=_stat([x + y for x, y in zip(twin, upload)]))
    g.close()
    print("RESULT " + json.dumps(res), flush=True)


def run_child(what, cfg, runs, rate=0.0, lib=None):
    env = dict(os.environ)
    env.pop("CELLECTOR_HIP_LIB", None)
    if what == "doublets":
        env["CELLECTOR_TIMING"] = "1"  # the phases of the call on stderr (the ingest's too: a few device synchronisations more)
    if lib:
        env["CELLECTOR_HIP_LIB"] = lib
    # (a line on stderr every minute while the child works: the host route is silent for minutes)
    t0 = time.time()
    p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", what, "--cfg", cfg, "--runs", str(runs), "--child-rate",
                          repr(rate)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    while True:
        try:
            out, err = p.communicate(timeout=60)
            break
        except subprocess.TimeoutExpired:
            print(f"[{what} {cfg}] running, {time.time() - t0:.0f} s", file=sys.stderr, flush=True)
            if time.time() - t0 > CHILD_LIMIT_S:
                p.kill()
                p.communicate()
                sys.exit(f"doublets_cost: the '{what}' measurement ran longer than {CHILD_LIMIT_S} s")
    if p.returncode != 0:
        sys.exit(f"doublets_cost: the '{what}' measurement failed ({p.returncode}):\n{out}\n{err[-4000:]}")
    res = json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    phases = {}  # "[timing]   add_doublets: <phase>   <seconds> s", one per call; the warm-up call's dropped
    for name, sec in re.findall(r"^\[timing\]\s+add_doublets: (.+?)\s+([0-9.]+) s$", err, flags=re.M):
        phases.setdefault(name, []).append(float(sec) * 1e3)
    if phases:
        res["add_doublets_phases_ms"] = {k: _stat(v[1:]) for k, v in phases.items() if len(v) > 1}
    print(f"[{'parent' if lib else 'this'} {what}] done", file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg4", choices=sorted(CFGS))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--doublet-rates", default="0,0.5")
    ap.add_argument("--upload", action="store_true")
    ap.add_argument("--upload-cfg", default=None, choices=sorted(CFGS))
    ap.add_argument("--upload-runs", type=int, default=1)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=["default", "doublets", "upload"])
    ap.add_argument("--child-rate", type=float, default=0.0)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.cfg, args.runs, args.child_rate)
    if args.runs < 5:
        sys.exit("doublets_cost: --runs must be at least 5")
    rates = [float(x) for x in args.doublet_rates.split(",")]
    L, N, d = CFGS[args.cfg]
    res = dict(tool="tools/doublets_cost.py", cfg=args.cfg, cells=N, loci=L, density=d, pairs=PAIRS[args.cfg], pair_seed=PAIR_SEED,
               parents="majority x minority by synth.cell_classes", engine=2, runs=args.runs, rates=rates)

    def save():  # (after every stage: a later stage that fails leaves what was measured)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)

    res["add_doublets"] = {}
    for rate in rates:
        res["add_doublets"][repr(rate)] = run_child("doublets", args.cfg, args.runs, rate)
        save()
    if args.parent_lib:
        parent, this = [], []
        for _ in range(args.repeats):  # alternating: parent, this, parent, this, ...
            parent.append(run_child("default", args.cfg, args.runs, lib=os.path.abspath(args.parent_lib)))
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
        first = res["add_doublets"][repr(rates[0])]
        cu = first if ucfg == args.cfg else run_child("doublets", ucfg, args.runs, rates[0])
        u = run_child("upload", ucfg, args.upload_runs, rates[0])
        assert (u["entries_after"], u["cells_after"]) == (cu["entries_after"], cu["cells_after"]), "the two routes made other matrices"
        res["upload_route"] = dict(cfg=ucfg, cells=CFGS[ucfg][1], loci=CFGS[ucfg][0], pairs=PAIRS[ucfg], rate=rates[0],
                                   add_doublets_at_this_cfg=cu if cu is not first else "the first measurement above",
                                   host_twin_and_ingest_coo=u,
                                   add_doublets_faster_than_upload_route=bool(cu["add_doublets_ms"]["max"] < u["twin_plus_ingest_coo_ms"]["min"]))
    else:
        res["upload_route"] = "not measured in this run (--upload)"
    print(json.dumps(res), flush=True)
    save()
    # the two acceptance criteria: a run that misses one fails
    if args.upload and not res["upload_route"]["add_doublets_faster_than_upload_route"]:
        sys.exit("doublets_cost: cellector_add_doublets is NOT faster than the host twin + cellector_ingest_coo route")
    if args.parent_lib and not res["default_mode_parent_vs_this"]["excess_inside_parent_spread"]:
        sys.exit("doublets_cost: the default iteration exceeds the parent's by more than the parent's spread")


if __name__ == "__main__":
    main()
