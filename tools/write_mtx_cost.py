#!/usr/bin/env python3
"""Cost of cellector_write_mtx (needs an MI355X).

  python tools/write_mtx_cost.py [--reps 5] [--parent-lib PATH/libcellector_hip.so] [--parent-tree DIR] [--workdir DIR] [--skip-cfg4]
                                [--out profiles/NAME.json]

write  cfg4 (200 000 loci x 1 000 000 cells, 1 %: 2e9 entries): the synthetic matrix' staged COO through cellector_write_mtx, mode
       ALIGNED, tabs, into --workdir (a page-cache path: /dev/shm by default).  From the library's line under CELLECTOR_TIMING=1:
       the GPU time of the length and the format kernels between their events, summed over the windows of both files, and the
       host's split of the call into formatting, waiting for the device-to-host copies and waiting for the file writes.
       floor_ms = the streaming floor of the pair, 12 B read per entry and file plus the body bytes written, over 6.3 TB/s;
       kernels_over_floor is the ratio.  Then cellector_load_mtx of the two files on a fresh ctx.  Measured only where the
       workdir has the room (about 16 B per entry and file); otherwise the file says so and nothing is extrapolated.
host   cfg3 (100 000 x 200 000, 1 %: 2e8 entries), in ONE process: cellector_write_mtx as above, and the route that existed
       before — cellector_staged_coo to the host, then the combiner's fprintf loop (host/combiner.cpp) on one host thread into the
       same directory.  The two pairs are compared byte for byte.
em     the default EM iteration (cfg4), ms per iteration, best of --reps in a fresh process, this library and with --parent-lib
       the parent commit's, alternating three times: the parent's own spread stands beside the difference.
bench  bench.py --gpus 1 --steps 20 --warmup 5 of this commit and, with --parent-tree, of a built checkout of the parent commit.

One fresh process per measurement, one after the other; a measurement that fails ends the run (nothing is tried again)."""
import argparse
import ctypes
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from donors_cost import CFGS, child_em  # noqa: E402  (the same matrices and the same loop measurement)

WRITE_LINE = re.compile(r"write_mtx: (\d+) entries, (\d+) windows per file: format ([\d.]+) s \(length kernels ([\d.]+) ms, format kernels ([\d.]+) ms\), "
                        r"waiting for copies ([\d.]+) s, for writes ([\d.]+) s")
HBM_STREAM = 6.3e12  # B/s a streaming kernel reaches on this part
HEADER_BYTES = len(b"%%MatrixMarket matrix coordinate real general\n% written by sprs\n")

FPRINTF_LOOP = r"""
#include <stdint.h>
#include <stdio.h>
/* the loop of host/combiner.cpp: one fprintf per line and file, one thread */
int host_write_pair(const char *alt_path, const char *ref_path, uint64_t total_loci, uint64_t total_cells, uint64_t n, const uint32_t *locus0,
                    const uint32_t *cell0, const uint32_t *alt, const uint32_t *ref)
{
    FILE *fa = fopen(alt_path, "w"), *fr = fopen(ref_path, "w");
    if (!fa || !fr) return 1;
    FILE *both[2] = {fa, fr};
    for (int k = 0; k < 2; k++)
        fprintf(both[k], "%%%%MatrixMarket matrix coordinate real general\n%% written by sprs\n%llu\t%llu\t%llu\n", (unsigned long long)total_loci,
                (unsigned long long)total_cells, (unsigned long long)n);
    for (uint64_t i = 0; i < n; i++) {
        fprintf(fa, "%llu\t%llu\t%llu\n", (unsigned long long)locus0[i] + 1, (unsigned long long)cell0[i] + 1, (unsigned long long)alt[i]);
        fprintf(fr, "%llu\t%llu\t%llu\n", (unsigned long long)locus0[i] + 1, (unsigned long long)cell0[i] + 1, (unsigned long long)ref[i]);
    }
    return (fclose(fa) != 0) | (fclose(fr) != 0);
}
"""


def _room(workdir, n_entries):
    st = os.statvfs(workdir)
    return st.f_bavail * st.f_frsize, 2 * 16 * n_entries


def _write(g, alt, ref):
    t0 = time.perf_counter()
    s = g.write_mtx(alt, ref, "aligned")
    return time.perf_counter() - t0, s.as_dict()


def child_write(cfg, workdir):
    sys.path.insert(0, ROOT)
    from cellector_amd import Cellector
    L, N, d = CFGS[cfg]
    os.makedirs(workdir, exist_ok=True)
    alt, ref = os.path.join(workdir, "alt.mtx"), os.path.join(workdir, "ref.mtx")
    out = dict(config="write", cfg=cfg, loci=L, cells=N, workdir=workdir)
    have, need = _room(workdir, int(L * N * d))
    if have < need:
        out["not_measured"] = f"{workdir} has {have >> 30} GB free, the pair needs about {need >> 30} GB"
        print(json.dumps(out), flush=True)
        return
    try:
        with Cellector(0) as g:
            g.ingest_synthetic(L, N, d, seed=4, minority_fraction=0.05)
            wall, s = _write(g, alt, ref)
            body = s["bytes_first"] + s["bytes_second"] - 2 * (HEADER_BYTES + len("%d\t%d\t%d\n" % (L, N, s["n_entries"])))
            out.update(entries=s["n_entries"], write_wall_s=wall, summary=s, floor_ms=(2 * 12 * s["n_entries"] + body) / HBM_STREAM * 1e3,
                       gb_per_s=(s["bytes_first"] + s["bytes_second"]) / wall / 1e9)
        with Cellector(0) as h:
            t0 = time.perf_counter()
            h.load_mtx(alt, ref)
            out["load_mtx_back_s"] = time.perf_counter() - t0
            out["load_mtx_back_nnz_used"] = int(h.dims().nnz_used)
    finally:
        for p in (alt, ref):
            if os.path.exists(p):
                os.remove(p)
    print(json.dumps(out), flush=True)


def child_host(cfg, workdir):
    sys.path.insert(0, ROOT)
    from cellector_amd import Cellector
    L, N, d = CFGS[cfg]
    os.makedirs(workdir, exist_ok=True)
    src = os.path.join(tempfile.gettempdir(), "host_write_pair.c")
    lib = os.path.join(tempfile.gettempdir(), "libhost_write_pair.so")
    open(src, "w").write(FPRINTF_LOOP)
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-o", lib, src])
    host = ctypes.CDLL(lib)
    host.host_write_pair.argtypes = [ctypes.c_char_p, ctypes.c_char_p] + [ctypes.c_uint64] * 3 + [ctypes.c_void_p] * 4
    paths = [os.path.join(workdir, n) for n in ("gpu_alt.mtx", "gpu_ref.mtx", "host_alt.mtx", "host_ref.mtx")]
    out = dict(config="host route", cfg=cfg, loci=L, cells=N, workdir=workdir)
    have, need = _room(workdir, 2 * int(L * N * d))
    if have < need:
        out["not_measured"] = f"{workdir} has {have >> 30} GB free, the two pairs need about {need >> 30} GB"
        print(json.dumps(out), flush=True)
        return
    try:
        with Cellector(0) as g:
            g.ingest_synthetic(L, N, d, seed=4, minority_fraction=0.05)
            _write(g, paths[0], paths[1])  # (the first call maps the pinned buffers)
            wall, s = _write(g, paths[0], paths[1])
            t0 = time.perf_counter()
            coo = g.staged_coo()
            t1 = time.perf_counter()
            rc = host.host_write_pair(paths[2].encode(), paths[3].encode(), L, N, len(coo[0]), *[a.ctypes.data for a in coo])
            t2 = time.perf_counter()
            assert rc == 0
        same = all(subprocess.run(["cmp", "-s", a, b]).returncode == 0 for a, b in ((paths[0], paths[2]), (paths[1], paths[3])))
        out.update(entries=s["n_entries"], write_mtx_s=wall, staged_coo_s=t1 - t0, fprintf_loop_s=t2 - t1, host_route_s=t2 - t0,
                   host_route_over_write_mtx=(t2 - t0) / wall, files_identical=same, summary=s)
    finally:
        for p in paths:
            if os.path.exists(p):
                os.remove(p)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libcellector_hip.so built from the parent commit")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: its bench.py is run as well")
    ap.add_argument("--workdir", default="/dev/shm/write_mtx_cost")
    ap.add_argument("--skip-cfg4", action="store_true")
    ap.add_argument("--skip-em", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=("write", "host", "em"))
    ap.add_argument("--cfg", default="cfg4")
    args = ap.parse_args()
    if args.child == "write":
        return child_write(args.cfg, args.workdir)
    if args.child == "host":
        return child_host(args.cfg, args.workdir)
    if args.child == "em":
        return child_em("cfg4", args.reps)
    notes = {}
    jobs = [("write", None, "cfg3"), ("host", None, "cfg3")]
    if args.skip_cfg4:
        notes["cfg4"] = "not measured in this run (--skip-cfg4): no figure is extrapolated"
    else:
        jobs.insert(0, ("write", None, "cfg4"))
    if not args.skip_em:
        jobs += [("em", None, "cfg4")] + ([("em", args.parent_lib, "cfg4"), ("em", None, "cfg4"), ("em", args.parent_lib, "cfg4"), ("em", None, "cfg4"),
                                           ("em", args.parent_lib, "cfg4")] if args.parent_lib else [])
    runs = []

    def save():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(dict(tool="tools/write_mtx_cost.py", notes=notes, runs=runs), f, indent=1)

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
        lines = WRITE_LINE.findall(r.stderr)
        if name in ("write", "host") and lines:
            m = lines[-1]
            rec["timing_line"] = dict(windows_per_file=int(m[1]), format_s=float(m[2]), length_kernels_ms=float(m[3]), format_kernels_ms=float(m[4]),
                                      waiting_for_copies_s=float(m[5]), waiting_for_writes_s=float(m[6]))
            if "floor_ms" in rec:
                rec["kernels_ms"] = float(m[3]) + float(m[4])
                rec["kernels_over_floor"] = rec["kernels_ms"] / rec["floor_ms"]
        if lib:
            rec["library"] = "parent commit"
        print(json.dumps(rec), flush=True)
        runs.append(rec)
        save()
    for tree in [ROOT] + ([os.path.abspath(args.parent_tree)] if args.parent_tree else []):
        env = dict(os.environ)
        env.pop("CELLECTOR_HIP_LIB", None)
        bench = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], capture_output=True,
                               text=True, timeout=1100, env=env, cwd=tree)
        if bench.returncode != 0:
            sys.exit(f"bench.py failed (status {bench.returncode})\n{bench.stderr[-2000:]}")
        runs.append(dict(config="bench.py --gpus 1 --steps 20 --warmup 5", library="this commit" if tree == ROOT else "parent commit",
                         result=json.loads(bench.stdout.strip().splitlines()[-1])))
        print(json.dumps(runs[-1]), flush=True)
        save()
    em = [r for r in runs if r.get("config") == "em_iteration"]
    if args.parent_lib and em:
        ours = [r["ms_min"] for r in em if r.get("library") != "parent commit"]
        theirs = [r["ms_min"] for r in em if r.get("library") == "parent commit"]
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        notes["em_iteration"] = dict(this_commit_best_ms=ours, parent_best_ms=theirs, this_median=med(ours), parent_median=med(theirs),
                                     parent_spread_ms=max(theirs) - min(theirs), difference_ms=med(ours) - med(theirs),
                                     inside_parent_spread=abs(med(ours) - med(theirs)) <= max(theirs) - min(theirs))
    save()


if __name__ == "__main__":
    main()
