#!/usr/bin/env python3
"""Cost of cellector_write_mtx_bgzf against cellector_write_mtx (needs an MI355X).

  python tools/write_bgzf_cost.py [--reps 5] [--parent-lib PATH/libcellector_hip.so] [--parent-tree DIR] [--workdir DIR] [--skip-cfg4]
                                 [--skip-em] [--out profiles/NAME.json]

pair   cfg3 (100 000 loci x 200 000 cells, 1 %: 2e8 entries) and cfg4 (200 000 x 1 000 000: 2e9), each in ONE process and into one
       file system (--workdir, a page-cache path: /dev/shm by default): the synthetic matrix' staged COO through cellector_write_mtx
       and then through cellector_write_mtx_bgzf, mode ALIGNED, tabs.  Per call, from the library's lines under CELLECTOR_TIMING=1:
       the whole call, the kernels' GPU time between their events (length + format; for the BGZF call also block + compaction), the
       host's wait for the device-to-host copies and for write(2).  write_wait_ratio = the plain call's wait for writes over the
       BGZF call's, byte_ratio = text bytes over file bytes: the expectation to confirm or refute is that the two agree.
       sample: the first 256 MB of the first file's text through zlib levels 1 and 6 on one host thread and through
       cellector_bgzf_compress: bytes and seconds.
       load: cellector_load_mtx of the plain pair and of the .gz pair, each on a fresh ctx.
       floor_ms: the compress kernels' streaming floor, the text read once and the compressed bytes written once, over 6.3 TB/s;
       compress_kernels_over_floor is the ratio.
       Measured only where the workdir has the room (about 20 B per entry and file); otherwise the file says so and nothing is
       extrapolated.
em     the default EM iteration (cfg4), ms per iteration, best of --reps in a fresh process, this library and with --parent-lib the
       parent commit's, alternating three times: the parent's own spread stands beside the difference.
bench  bench.py --gpus 1 --steps 20 --warmup 5 of this commit and, with --parent-tree, of a built checkout of the parent commit.

One fresh process per measurement, one after the other; a measurement that fails ends the run (nothing is tried again)."""
import argparse
import json
import os
import re
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from donors_cost import CFGS, child_em  # noqa: E402  (the same matrices and the same loop measurement)

WRITE_LINE = re.compile(r"write_mtx: (\d+) entries, (\d+) windows per file: format ([\d.]+) s \(length kernels ([\d.]+) ms, format kernels ([\d.]+) ms\), "
                        r"waiting for copies ([\d.]+) s, for writes ([\d.]+) s")
BGZF_LINE = re.compile(r"write_mtx_bgzf: .*?block kernels ([\d.]+) ms, compaction kernels ([\d.]+) ms")
HBM_STREAM = 6.3e12  # B/s a streaming kernel reaches on this part
SAMPLE = 256 << 20


def child_pair(cfg, workdir):
    sys.path.insert(0, ROOT)
    from cellector_amd import Cellector
    L, N, d = CFGS[cfg]
    os.makedirs(workdir, exist_ok=True)
    plain = [os.path.join(workdir, n) for n in ("alt.mtx", "ref.mtx")]
    packed = [p + ".gz" for p in plain]
    out = dict(config="pair", cfg=cfg, loci=L, cells=N, workdir=workdir)
    st = os.statvfs(workdir)
    have, need = st.f_bavail * st.f_frsize, 2 * 20 * int(L * N * d)
    if have < need:
        out["not_measured"] = f"{workdir} has {have >> 30} GB free, the two pairs need about {need >> 30} GB"
        print(json.dumps(out), flush=True)
        return
    try:
        with Cellector(0) as g:
            g.ingest_synthetic(L, N, d, seed=4, minority_fraction=0.05)
            t0 = time.perf_counter()
            s = g.write_mtx(*plain, "aligned").as_dict()
            t1 = time.perf_counter()
            z = g.write_mtx_bgzf(*packed, "aligned").as_dict()
            t2 = time.perf_counter()
            assert z["text"] == s
            text, files = s["bytes_first"] + s["bytes_second"], z["file_bytes_first"] + z["file_bytes_second"]
            out.update(entries=s["n_entries"], write_mtx_s=t1 - t0, write_mtx_bgzf_s=t2 - t1, text_bytes=text, file_bytes=files,
                       byte_ratio=text / files, summary=z, floor_ms=(text + files) / HBM_STREAM * 1e3)
            sample = open(plain[0], "rb").read(SAMPLE)
            rec = dict(bytes=len(sample))
            for level in (1, 6):
                t0 = time.perf_counter()
                rec["zlib_%d_bytes" % level] = len(zlib.compress(sample, level))
                rec["zlib_%d_s" % level] = time.perf_counter() - t0
            t0 = time.perf_counter()
            rec["bgzf_bytes"] = len(g.bgzf_compress(sample))
            rec["bgzf_compress_s"] = time.perf_counter() - t0  # (two calls of the entry point: the sizes, then the bytes)
            for level in (1, 6):
                rec["bgzf_over_zlib_%d" % level] = rec["bgzf_bytes"] / rec["zlib_%d_bytes" % level]
            out["sample"] = rec
            del sample
        for name, pair in (("plain", plain), ("gz", packed)):
            with Cellector(0) as h:
                t0 = time.perf_counter()
                h.load_mtx(*pair)
                out["load_mtx_%s_s" % name] = time.perf_counter() - t0
                out["load_mtx_%s_nnz_used" % name] = int(h.dims().nnz_used)
    finally:
        for p in plain + packed:
            if os.path.exists(p):
                os.remove(p)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libcellector_hip.so built from the parent commit")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: its bench.py is run as well")
    ap.add_argument("--workdir", default="/dev/shm/write_bgzf_cost")
    ap.add_argument("--skip-cfg4", action="store_true")
    ap.add_argument("--skip-em", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=("pair", "em"))
    ap.add_argument("--cfg", default="cfg4")
    args = ap.parse_args()
    if args.child == "pair":
        return child_pair(args.cfg, args.workdir)
    if args.child == "em":
        return child_em("cfg4", args.reps)
    notes = {}
    jobs = [("pair", None, "cfg3")]
    if args.skip_cfg4:
        notes["cfg4"] = "not measured in this run (--skip-cfg4): no figure is extrapolated"
    else:
        jobs.append(("pair", None, "cfg4"))
    if not args.skip_em:
        jobs += [("em", None, "cfg4")] + ([("em", args.parent_lib, "cfg4"), ("em", None, "cfg4"), ("em", args.parent_lib, "cfg4"), ("em", None, "cfg4"),
                                           ("em", args.parent_lib, "cfg4")] if args.parent_lib else [])
    runs = []

    def save():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(dict(tool="tools/write_bgzf_cost.py", notes=notes, runs=runs), f, indent=1)

    def phases(m):
        return dict(windows_per_file=int(m[1]), format_s=float(m[2]), length_kernels_ms=float(m[3]), format_kernels_ms=float(m[4]),
                    waiting_for_copies_s=float(m[5]), waiting_for_writes_s=float(m[6]))

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
        lines, zline = WRITE_LINE.findall(r.stderr), BGZF_LINE.findall(r.stderr)
        if name == "pair" and len(lines) == 2 and len(zline) == 1:  # the plain call's line, then the BGZF call's two
            rec["write_mtx"], rec["write_mtx_bgzf"] = phases(lines[0]), phases(lines[1])
            rec["write_mtx_bgzf"].update(block_kernels_ms=float(zline[0][0]), compaction_kernels_ms=float(zline[0][1]))
            rec["compress_kernels_ms"] = float(zline[0][0]) + float(zline[0][1])
            rec["compress_kernels_over_floor"] = rec["compress_kernels_ms"] / rec["floor_ms"]
            waits = rec["write_mtx"]["waiting_for_writes_s"], rec["write_mtx_bgzf"]["waiting_for_writes_s"]
            rec["write_wait_ratio"] = waits[0] / waits[1] if waits[1] > 0 else None
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
