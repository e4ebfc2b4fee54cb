#!/usr/bin/env python3
"""Cost of option gz_device: cellector_load_mtx of a BGZF pair inflated on the device against the host inflate (needs an MI355X).

  python tools/gz_device_cost.py [--reps 5] [--parent-lib PATH/libcellector_hip.so] [--parent-tree DIR] [--workdir DIR] [--skip-cfg4]
                                 [--skip-em] [--out profiles/NAME.json]

pair   cfg3 (100 000 loci x 200 000 cells, 1 %: 2e8 entries) and cfg4 (200 000 x 1 000 000: 2e9), each in ONE process on one GPU with
       the files in one file system (--workdir, a page-cache path: /dev/shm by default).  The synthetic matrix' staged COO is written
       as the plain pair (cellector_write_mtx), as the library's own BGZF pair (cellector_write_mtx_bgzf) and as a bgzip-like pair
       (zlib level 6 in blocks of 65280 bytes, made by a pool of host processes from the plain pair).  Then cellector_load_mtx, each
       on a fresh ctx: the plain pair once per round, and each .gz pair with gz_device 0 and 1, alternating, --reps rounds: the best
       of each, gz_device_speedup = best(0) / best(1), and both against the plain pair.  From the library's lines under
       CELLECTOR_TIMING=1 of the best gz_device 1 load: members, bytes in and out, the inflate kernel's GPU time between events,
       text_rate_GBps = bytes out / that time, and the two "(upload + tokens)" phases; upload_share = compressed bytes / text bytes.
       Measured only where the workdir has the room (about 25 B per entry and file); otherwise the file says so and nothing is
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from donors_cost import CFGS, child_em  # noqa: E402  (the same matrices and the same loop measurement)

INFLATE_LINE = re.compile(r"inflate on the device: (\S+): (\d+) members, (\d+) -> (\d+) bytes, inflate kernel ([\d.]+) ms")
PHASE_LINE = re.compile(r"\[timing\]\s+(alt|ref) file \(upload \+ tokens\)\s+([\d.]+) s")
BLOCK = 65280
PIECE = BLOCK * 512


def _bgzip_piece(args):
    sys.path.insert(0, ROOT)
    from cellector_amd import synth
    path, at, n = args
    with open(path, "rb") as f:
        f.seek(at)
        return synth.bgzf_compress(f.read(n), block=BLOCK, eof_block=False)


def bgzip_like(src, dst, procs=16):
    """src as a BGZF file of zlib level 6 members of 65280 bytes of text"""
    import multiprocessing as mp
    from cellector_amd import bgzf
    size = os.path.getsize(src)
    with mp.Pool(procs) as pool, open(dst, "wb") as out:
        for blob in pool.imap(_bgzip_piece, [(src, at, min(PIECE, size - at)) for at in range(0, size, PIECE)]):
            out.write(blob)
        out.write(bgzf.EOF)


def child_pair(cfg, workdir, reps):
    sys.path.insert(0, ROOT)
    import tempfile
    from cellector_amd import Cellector
    L, N, d = CFGS[cfg]
    os.makedirs(workdir, exist_ok=True)
    plain = [os.path.join(workdir, n) for n in ("alt.mtx", "ref.mtx")]
    ours = [os.path.join(workdir, "lib_" + n + ".gz") for n in ("alt.mtx", "ref.mtx")]
    theirs = [os.path.join(workdir, "zlib_" + n + ".gz") for n in ("alt.mtx", "ref.mtx")]
    out = dict(config="pair", cfg=cfg, loci=L, cells=N, workdir=workdir, reps=reps)
    st = os.statvfs(workdir)
    have, need = st.f_bavail * st.f_frsize, 2 * 25 * int(L * N * d)
    if have < need:
        out["not_measured"] = f"{workdir} has {have >> 30} GB free, the three pairs need about {need >> 30} GB"
        print(json.dumps(out), flush=True)
        return

    def stderr_of(fn):
        """fn() with the process' stderr (the library's timing lines) captured"""
        sys.stderr.flush()
        with tempfile.TemporaryFile() as tmp:
            saved = os.dup(2)
            os.dup2(tmp.fileno(), 2)
            try:
                fn()
            finally:
                os.dup2(saved, 2)
                os.close(saved)
            tmp.seek(0)
            return tmp.read().decode(errors="replace")

    def load(pair, gz_device):
        rec = {}
        def run():
            with Cellector(0) as h:
                h.set_option("gz_device", gz_device)
                t0 = time.perf_counter()
                h.load_mtx(*pair)
                rec["s"] = time.perf_counter() - t0
                rec["nnz_used"] = int(h.dims().nnz_used)
        rec["stderr"] = stderr_of(run)
        return rec

    try:
        with Cellector(0) as g:
            g.ingest_synthetic(L, N, d, seed=4, minority_fraction=0.05)
            s = g.write_mtx(*plain, "aligned").as_dict()
            z = g.write_mtx_bgzf(*ours, "aligned").as_dict()
        for a, b in zip(plain, theirs):
            bgzip_like(a, b)
        out.update(entries=s["n_entries"], text_bytes=s["bytes_first"] + s["bytes_second"],
                   lib_gz_bytes=z["file_bytes_first"] + z["file_bytes_second"], zlib_gz_bytes=sum(os.path.getsize(p) for p in theirs))
        best = {}
        for rep in range(reps):
            for key, pair, gz_device in (("plain", plain, 0), ("lib_gz_0", ours, 0), ("lib_gz_1", ours, 1), ("zlib_gz_0", theirs, 0),
                                         ("zlib_gz_1", theirs, 1)):
                rec = load(pair, gz_device)
                out.setdefault("load_mtx_s", {}).setdefault(key, []).append(rec["s"])
                if key not in best or rec["s"] < best[key]["s"]:
                    best[key] = rec
        nnz = {k: v["nnz_used"] for k, v in best.items()}
        assert len(set(nnz.values())) == 1, nnz
        out["nnz_used"] = nnz["plain"]
        out["best_s"] = {k: v["s"] for k, v in best.items()}
        for kind in ("lib", "zlib"):
            b0, b1 = best[kind + "_gz_0"]["s"], best[kind + "_gz_1"]["s"]
            rec = dict(gz_device_speedup=b0 / b1, gz_device_0_over_plain=b0 / best["plain"]["s"], gz_device_1_over_plain=b1 / best["plain"]["s"])
            files = INFLATE_LINE.findall(best[kind + "_gz_1"]["stderr"])
            if files:
                ms = sum(float(f[4]) for f in files)
                rec.update(members=sum(int(f[1]) for f in files), bytes_in=sum(int(f[2]) for f in files), bytes_out=sum(int(f[3]) for f in files),
                           inflate_kernel_ms=ms, text_rate_GBps=sum(int(f[3]) for f in files) / (ms * 1e-3) / 1e9 if ms else None)
                rec["upload_share"] = rec["bytes_in"] / rec["bytes_out"]
            for setting in ("0", "1"):
                rec["upload_tokens_s_gz_device_" + setting] = {k: float(v) for k, v in PHASE_LINE.findall(best[kind + "_gz_" + setting]["stderr"])}
            out[kind + "_gz"] = rec
    finally:
        for p in plain + ours + theirs:
            if os.path.exists(p):
                os.remove(p)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libcellector_hip.so built from the parent commit")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: its bench.py is run as well")
    ap.add_argument("--workdir", default="/dev/shm/gz_device_cost")
    ap.add_argument("--skip-cfg4", action="store_true")
    ap.add_argument("--skip-em", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=("pair", "em"))
    ap.add_argument("--cfg", default="cfg4")
    args = ap.parse_args()
    if args.child == "pair":
        return child_pair(args.cfg, args.workdir, args.reps)
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
                json.dump(dict(tool="tools/gz_device_cost.py", notes=notes, runs=runs), f, indent=1)

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
