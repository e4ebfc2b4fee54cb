#!/usr/bin/env python3
"""Cost of the two paths of DESIGN §3.2c at cfg4 (bench.py's synthetic 200k loci x 10^6 cells; needs an MI355X), engine 2:

  masked     cellector_cell_log_likelihoods under a random 30 % mask: kernel_time(CELLECTOR_K_CELL_LL) (option timing 1) of each of
             five calls after one warm-up, and their median.  Run it once with this commit's library and once with the parent
             commit's (CELLECTOR_HIP_LIB=path/to/parent/libcellector_hip.so): there the call runs the CSR kernel.
  cell_pmfs  at the loop's fixed point: Cellector.cell_pmfs of the ~5 % excluded cells, all six columns: wall time of the two calls
             (count, fill), best of three after one warm-up.

  python tools/pmfs_cost.py masked|cell_pmfs [--cfg cfg4] [--out profiles/NAME.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFGS = {"cfg1": (2_000, 1_000, 0.1), "cfg3": (100_000, 200_000, 0.01), "cfg4": (200_000, 1_000_000, 0.01)}  # loci, cells, density


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["masked", "cell_pmfs"])
    ap.add_argument("--cfg", default="cfg4", choices=sorted(CFGS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    from cellector_amd import Cellector, ffi
    L, N, d = CFGS[args.cfg]
    g = Cellector(0)
    g.set_option("engine", 2)
    g.load_synthetic(L, N, d, seed=4, minority_fraction=0.05)
    Lu = g.dims().loci_used
    res = dict(tool="tools/pmfs_cost.py", what=args.what, cfg=args.cfg, cells=N, loci_used=int(Lu), nnz=int(g.dims().nnz_used),
               library=os.path.basename(os.path.dirname(os.path.dirname(ffi.LIB_PATH))) if os.environ.get("CELLECTOR_HIP_LIB") else "this commit")
    if args.what == "masked":
        g.set_option("timing", 1)
        a, b = g.alpha_betas()
        mask = (np.random.default_rng(1).random(Lu) >= 0.3).astype(np.uint8)
        ms, tile = [], []
        for _ in range(6):
            t0, n0 = g.kernel_time(ffi.K_CELL_LL)
            k0 = g.kernel_time(ffi.K_TILE_LL)[1]
            w0 = time.perf_counter()
            g.cell_log_likelihoods(a, b, mask)
            wall = (time.perf_counter() - w0) * 1e3
            t1, n1 = g.kernel_time(ffi.K_CELL_LL)
            ms.append(dict(cell_ll_ms=t1 - t0, regions=int(n1 - n0), wall_ms=wall))
            tile.append(int(g.kernel_time(ffi.K_TILE_LL)[1] - k0))
        ms = ms[1:]
        res.update(calls=ms, cell_ll_ms_median=statistics.median(x["cell_ll_ms"] for x in ms), tile_kernel_launches_per_call=tile[1:])
    else:
        iters = len(g.run(5.0, 30))
        cells = np.nonzero(g.excluded())[0]
        times = []
        for _ in range(4):
            t0 = time.perf_counter()
            r = g.cell_pmfs(cells)
            times.append((time.perf_counter() - t0) * 1e3)
        res.update(em_iterations=iters, n_cells_listed=int(len(cells)), records=int(r["rec_ptr"][-1]), wall_ms=times[1:],
                   wall_ms_min=min(times[1:]))
    g.close()
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
