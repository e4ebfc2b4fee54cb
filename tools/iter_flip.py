#!/usr/bin/env python3
"""Wall time of single EM iterations of the default bench workload (cfg4) while the exclusion set keeps MOVING: the run is taken
to its fixed point, then before every timed iteration k random cells are flipped with set_excluded, for k = 0, 1, 10, 100, and
the all-dirty case is timed as the first iteration after em_reset.  Beside each time the share of loci whose (alpha, beta) bits
differ from the pass before (alpha_betas() read outside the timed window) — the loci option t2_cache has to gather again.
One library per process: CELLECTOR_HIP_LIB picks it, a shell loop alternates two builds.  The last line is one JSON object.
usage: python3 tools/iter_flip.py [reps] [k=v ...]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from bench import WORKLOADS
from cellector_amd import Cellector

reps = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 12
N, L, d, pct = WORKLOADS[os.environ.get("CELLECTOR_BENCH_WORKLOAD", "cfg4")]
g = Cellector(0, stream=torch.cuda.current_stream().cuda_stream)
g.set_option("keep_coo", 0)
for kv in [a for a in sys.argv[1:] if "=" in a]:
    k, v = kv.split("=")
    g.set_option(k, int(v))
g.set_option("synth_continue_pct", pct)
free0 = torch.cuda.mem_get_info()[0]
g.ingest_synthetic(L, N, d, seed=4, minority_fraction=0.05, doublet_fraction=0.0)
g.ingest_finish(4, 4)
torch.cuda.synchronize()
held = free0 - torch.cuda.mem_get_info()[0]


def ab_bits():
    a, b = g.alpha_betas()
    return np.stack([a.view(np.uint64), b.view(np.uint64)])


def timed():
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s = g.em_iteration(5.0)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, s


def stats(ms, dirty):
    ms = sorted(ms)
    return dict(median=ms[len(ms) // 2], min=ms[0], max=ms[-1], n=len(ms), dirty_fraction=float(np.mean(dirty)))


out = dict(lib=os.environ.get("CELLECTOR_HIP_LIB", "built"), device_bytes_after_ingest=int(held), cases={})
first_ms, _ = timed()
out["first_iteration_after_ingest_ms"] = first_ms
n_conv = 1
while g.em_iteration(5.0).any_change and n_conv < 200:
    n_conv += 1
out["iterations_to_fixed_point"] = n_conv
rng = np.random.default_rng(7)
prev = ab_bits()
for k in (0, 1, 10, 100, 0):
    ms, dirty = [], []
    for r in range(reps + 2):
        if k:
            f = g.excluded()
            f[rng.choice(f.size, k, replace=False)] ^= 1
            g.set_excluded(f)
        now = ab_bits()
        t, s = timed()
        if r >= 2:  # (the first two of a case carry the case before)
            ms.append(t)
            dirty.append((now != prev).any(axis=0).mean())
        prev = now
    name = f"flip_{k}" if f"flip_{k}" not in out["cases"] else f"flip_{k}_again"
    out["cases"][name] = stats(ms, dirty)
    print(name, out["cases"][name])
ms, dirty = [], []
for r in range(max(3, reps // 2)):
    g.em_reset()
    now = ab_bits()
    t, s = timed()
    ms.append(t)
    dirty.append((now != prev).any(axis=0).mean())
    t2, _ = timed()  # the second iteration of a run: every locus moves again
    prev = ab_bits()
out["cases"]["all_dirty_after_em_reset"] = stats(ms, dirty)
print("all_dirty_after_em_reset", out["cases"]["all_dirty_after_em_reset"])
g.close()
print(json.dumps(out))
