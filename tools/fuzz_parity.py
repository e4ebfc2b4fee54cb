#!/usr/bin/env python3
"""Randomised parity sweep (needs an MI355X): whole runs of the HIP path against the CPU oracle on matrices of random shape,
density, minority share and count distribution — the checks of tests/test_gpu_parity.py on inputs nobody picked by hand.

  python tools/fuzz_parity.py [--cases 40] [--seed 1] [--max-cells 60000] [--resolve-ties] [--resolve-posteriors] [--warm-start]

Every case: ingest (device generator, then counts widened at random so that all overflow tiers occur), both engines or
engine 2 with a random option set (locus-pass form, overlap, two shards), EM loop until the oracle stops, posteriors,
assignments.  Prints one line per case and a summary; exits non-zero on the first mismatch.

--resolve-ties: every single-device case runs a second time with option resolve_ties (set before the ingest) and must then
match the oracle exactly in every iteration — median, iqr, threshold bits, exclusion flags, change counts — including the
cases the plain comparison reports as undecidable (cells on the threshold to 1e-9); the summary counts both.

--resolve-posteriors: every single-device case runs again with resolve_ties and resolve_posteriors both on (mode 1, then mode 2):
labels, anomaly flags and quals of cellector_assign must equal the oracle's and the evaluated cells' posterior, doublet
posterior and LLs must be its bits, for 0.999 and a few random thresholds, some taken from a cell's own posterior.

--warm-start: every case runs again from a random initial exclusion set of random size (0 ... N), placed with
cellector_set_excluded (a single-device ctx, or one ctx over two logical shards for the two-shard cases) and in the oracle with
Oracle.set_excluded: alpha/beta of the placed set exact, then every iteration as in the plain run, then posteriors."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=40)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--max-cells", type=int, default=60000)
    ap.add_argument("--resolve-ties", action="store_true", help="also run every single-device case with option resolve_ties")
    ap.add_argument("--resolve-posteriors", action="store_true",
                    help="also run every single-device case with resolve_ties and resolve_posteriors on (modes 1 and 2)")
    ap.add_argument("--warm-start", action="store_true",
                    help="also run every case from a random initial exclusion set (cellector_set_excluded)")
    args = ap.parse_args()
    from cellector_amd import Cellector, ffi, synth
    from oracle import binding as ob
    import test_gpu_parity as T  # the checkers

    ob.build()
    ob.set_threads(ob.host_threads())
    mods = dict(ffi=ffi, synth=synth, ob=ob, engine=2)
    rng = np.random.default_rng(args.seed)
    t_all = time.time()
    n_resolved = n_resolved_undecidable = 0
    n_assign = n_assign_evaluated = n_assign_cells = 0
    n_warm = n_warm_undecidable = 0
    for case in range(args.cases):
        N = int(rng.choice([1, 3, 70, 700, 1100, 5000, 20000, args.max_cells]))
        L = int(rng.choice([50, 400, 1500, 4200, 9000]))  # (one or two loci: every cell ties with thousands of others)
        dens = float(rng.choice([0.005, 0.02, 0.1, 0.5]))
        if N * L * dens > 6e6:
            dens = max(0.002, 6e6 / (N * L))
        # keep a locus' totals moderate: the ORACLE's ln_gamma differences (the reference's formula) lose ~1e-8 per entry
        # at alpha + beta ~ 1e6, which would drown the comparison, not the device's product form
        dens = min(dens, 3000.0 / N)
        minority = float(rng.choice([0.0, 0.02, 0.08, 0.2, 0.45]))
        doublet = float(rng.choice([0.0, 0.03]))
        seed = int(rng.integers(1, 1 << 30))
        lo, ce, al, re = synth.generate_coo(L, N, dens, seed=seed, minority_fraction=minority, doublet_fraction=doublet)
        if len(lo) and rng.random() < 0.6:  # widen counts: overflow tiers (totals 5..8, 9..17, above), zero/zero entries
            big = rng.random(len(al)) < rng.choice([0.02, 0.2])
            f = rng.integers(1, int(rng.choice([4, 12, 60])), len(al))
            al = np.where(big, al * f, al).astype(np.uint32)
            re = np.where(big, re * f, re).astype(np.uint32)
            zero = rng.random(len(al)) < 0.002
            al = np.where(zero, 0, al).astype(np.uint32)
            re = np.where(zero, 0, re).astype(np.uint32)
        min_alt, min_ref = (int(x) for x in rng.choice([[0, 0], [1, 1], [4, 4]]))
        engine = int(rng.choice([2, 2, 2, 1]))
        opts = {}
        if engine == 2:
            opts = {"locus_mode": int(rng.choice([0, 0, 1, 2])), "overlap": int(rng.choice([1, 1, 0, 2])),
                    "compact_bits": int(rng.choice([0, 0, 32])), "side_lds": int(rng.choice([-1, -1, 5000])),
                    "ovf_deep": int(rng.choice([-1, -1, 0, 1])), "ovf_deep_wide": int(rng.choice([1, 1, 0])), "t2": int(rng.choice([-1, -1, 0, 1])),
                    "bank_order": int(rng.choice([1, 1, 1, 0])), "t2_tiles": int(rng.choice([-1, -1, 0, 6, 8]))}
        two_shards = engine == 2 and N >= 2 and rng.random() < 0.25
        desc = f"case {case}: N={N} L={L} d={dens:.3g} min={minority} dbl={doublet} nnz={len(lo)} engine={engine} {opts}" \
               f"{' 2 shards' if two_shards else ''} filter=({min_alt},{min_ref})"
        t0 = time.time()
        o = ob.Oracle.from_coo(L, N, lo, ce, al, re, min_alt, min_ref)
        if two_shards:
            ok = run_two_shards(Cellector, ffi, o, L, N, lo, ce, al, re, min_alt, min_ref, opts)
        else:
            g = Cellector(0)
            g.set_option("engine", engine)
            for k, v in opts.items():
                g.set_option(k, v)
            g.load_coo(L, N, lo, ce, al, re, min_alt, min_ref)
            T._check_matrix(g, o)
            ok = True
            if o.loci_used and N:
                mods["engine"] = engine
                try:
                    T._run_both(g, o)
                    T._check_posteriors(mods, g, o)
                except AssertionError as e:
                    if "near-tie" not in str(e):
                        raise
                    ok = None  # cells sit on the threshold to 1e-9: the comparison cannot decide, not a mismatch
            g.close()
        o.close()
        res = ""
        if args.resolve_ties and not two_shards and ok is not False:
            res_ok = run_resolved(Cellector, ob, engine, opts, L, N, lo, ce, al, re, min_alt, min_ref)
            n_resolved += 1
            n_resolved_undecidable += ok is None
            res = "; resolve_ties: " + ("exact" if res_ok else "MISMATCH")
            if not res_ok:
                ok = False
        if args.resolve_posteriors and not two_shards and ok is not False:
            a_ok, n_ev, n_cells = run_resolved_posteriors(Cellector, ob, engine, opts, L, N, lo, ce, al, re, min_alt, min_ref,
                                                          np.random.default_rng(args.seed * 1000003 + case))
            n_assign += 1
            n_assign_evaluated += n_ev
            n_assign_cells += n_cells
            res += "; resolve_posteriors: " + ("exact" if a_ok else "MISMATCH")
            if not a_ok:
                ok = False
        if args.warm_start and ok is not False:
            w_ok = run_warm_start(Cellector, ffi, synth, ob, T, engine, opts, two_shards, L, N, lo, ce, al, re, min_alt, min_ref,
                                  np.random.default_rng(args.seed * 7919 + case))
            n_warm += 1
            n_warm_undecidable += w_ok is None
            res += "; warm start: " + ("exact" if w_ok else ("undecidable (near-ties)" if w_ok is None else "MISMATCH"))
            if w_ok is False:
                ok = False
        print(f"{desc}: {'ok' if ok else ('undecidable (near-ties)' if ok is None else 'MISMATCH')}{res} ({time.time() - t0:.1f} s)",
              flush=True)
        if ok is False:
            sys.exit(1)
    print(f"{args.cases} cases ok in {time.time() - t_all:.0f} s")
    if args.resolve_ties:
        print(f"resolve_ties: {n_resolved} cases exact, {n_resolved_undecidable} of them undecidable without the option")
    if args.warm_start:
        print(f"warm start: {n_warm} cases, {n_warm - n_warm_undecidable} matched the oracle, {n_warm_undecidable} undecidable "
              f"(near-ties), 0 mismatches")
    if args.resolve_posteriors:
        print(f"resolve_posteriors: {n_assign} cases exact (modes 1 and 2); mode 1 evaluated {n_assign_evaluated} of "
              f"{n_assign_cells} cells x thresholds")


def run_warm_start(Cellector, ffi, synth, ob, T, engine, opts, two_shards, L, N, lo, ce, al, re, min_alt, min_ref, rng):
    """the case again from a random initial exclusion set of random size.  True / None (near-ties: undecidable) / False"""
    flags = np.zeros(N, np.uint8)
    flags[rng.choice(N, int(rng.integers(0, N + 1)), replace=False)] = 1
    o = ob.Oracle.from_coo(L, N, lo, ce, al, re, min_alt, min_ref)
    g = Cellector(devices=[0, 0]) if two_shards else Cellector(0)
    g.set_option("engine", engine)
    for k, v in opts.items():
        g.set_option(k, v)
    g.load_coo(L, N, lo, ce, al, re, min_alt, min_ref)
    g.set_excluded(flags)
    o.set_excluded(flags)
    ok = bool(np.array_equal(g.excluded(), flags))
    (ag, bg), (ao, bo) = g.alpha_betas(), o.alpha_betas()
    ok = ok and bool(np.array_equal(ag, ao) and np.array_equal(bg, bo))
    if not ok:
        print(f"  warm start: the placed state differs ({int(flags.sum())} of {N} cells)", flush=True)
    elif o.loci_used and N:
        try:
            T._run_both(g, o)
            T._check_posteriors(dict(ffi=ffi, synth=synth, ob=ob, engine=engine), g, o)
        except AssertionError as e:
            if "near-tie" not in str(e):
                print(f"  warm start from {int(flags.sum())} of {N} cells: {str(e)[:300]}", flush=True)
                ok = False
            else:
                ok = None
    g.close()
    o.close()
    return ok


def run_resolved_posteriors(Cellector, ob, engine, opts, L, N, lo, ce, al, re, min_alt, min_ref, rng):
    """one device, both resolve options at 1 and then at 2: cellector_assign against the oracle for several thresholds.
    Returns (ok, cells mode 1 evaluated, cells x thresholds)."""
    n_ev = n_cells = 0
    for mode in (1, 2):
        o = ob.Oracle.from_coo(L, N, lo, ce, al, re, min_alt, min_ref)
        g = Cellector(0)
        g.set_option("engine", engine)
        for k, v in opts.items():
            g.set_option(k, v)
        g.set_option("resolve_ties", mode)
        g.set_option("resolve_posteriors", mode)
        g.load_coo(L, N, lo, ce, al, re, min_alt, min_ref)
        ok = True
        if o.loci_used and N:
            for _ in range(30):
                g.em_iteration(5.0)
                if not o.em_iteration(5.0).any_change:
                    break
            ok = bool(np.array_equal(g.excluded(), o.excluded()))
            po = o.posteriors()
            own = po["posterior"][(po["posterior"] > 0.0) & (po["posterior"] < 1.0)]
            ts = [0.999] + rng.uniform(0.5, 1.0, 2).tolist()
            if own.size:
                q = float(rng.choice(own))
                ts += [q, float(np.nextafter(q, 0.0))]
            for T in ts:
                if not ok:
                    break
                r = g.assign(T, 30)
                want = o.assignments(po["posterior"], po["doublet_posterior"], T, 30)
                ev = g.assign_resolved_cells()
                ok = (np.array_equal(r["posterior_assignment"], want[0]) and np.array_equal(r["anomaly_assignment"], want[1])
                      and np.array_equal(r["qual"], want[2]) and (mode == 1 or ev.size == N)
                      and all(np.array_equal(r[k][ev].view(np.uint64), po[k][ev].view(np.uint64))
                              for k in ("posterior", "doublet_posterior", "ll_majority", "ll_minority")))
                if mode == 1:
                    n_ev += int(ev.size)
                    n_cells += N
                if not ok:
                    print(f"  resolve_posteriors mismatch: mode {mode}, threshold {T!r}", flush=True)
        g.close()
        o.close()
        if not ok:
            return False, n_ev, n_cells
    return True, n_ev, n_cells


def run_resolved(Cellector, ob, engine, opts, L, N, lo, ce, al, re, min_alt, min_ref):
    """one device, option resolve_ties: median / iqr / threshold bits, flags and change counts of every iteration are the oracle's"""
    o = ob.Oracle.from_coo(L, N, lo, ce, al, re, min_alt, min_ref)
    g = Cellector(0)
    g.set_option("engine", engine)
    for k, v in opts.items():
        g.set_option(k, v)
    g.set_option("resolve_ties", 1)
    g.load_coo(L, N, lo, ce, al, re, min_alt, min_ref)
    ok = True
    if o.loci_used and N:
        for _ in range(30):
            sg, so = g.em_iteration(5.0), o.em_iteration(5.0)
            if not ((sg.median, sg.iqr, sg.threshold) == (so.median, so.iqr, so.threshold)
                    and np.array_equal(g.excluded(), o.excluded())
                    and (sg.any_change, sg.n_new_excluded, sg.n_rescued) == (so.any_change, so.n_new_excluded, so.n_rescued)):
                print(f"  resolve_ties mismatch: device {(sg.median, sg.iqr, sg.threshold)} oracle {(so.median, so.iqr, so.threshold)}",
                      flush=True)
                ok = False
                break
            if not so.any_change:
                break
    g.close()
    o.close()
    return ok


def run_two_shards(Cellector, ffi, o, L, N, lo, ce, al, re, min_alt, min_ref, opts):
    """two shard contexts driven through the exchange buffers on one GPU (host-summed), against the oracle"""
    cut = int(np.random.default_rng(N * 7919 + L).choice([0, N // 3, N // 2, N]))  # an empty shard now and then
    gs = []
    for cb, cend in ((0, cut), (cut, N)):
        g = Cellector(0)
        for k, v in opts.items():
            g.set_option(k, v)
        g.set_shard(cb, cend)
        g.ingest_coo(L, N, lo, ce, al, re)
        gs.append(g)
    import test_gpu_parity as T
    hip = T._hip()
    T._allreduce(hip, gs, ffi.XCHG_PASS1)
    for g in gs:
        g.ingest_finish(min_alt, min_ref)
    if not (o.loci_used and N):
        for g in gs:
            g.close()
        return True
    for _ in range(30):
        so = o.em_iteration(5.0)
        for g in gs:
            g.em_begin()
        T._allreduce(hip, gs, ffi.XCHG_NORM)
        for g in gs:
            g.em_threshold(5.0)
        T._allreduce(hip, gs, ffi.XCHG_LOCUS)
        outs = [g.em_finish() for g in gs]
        s = outs[0]
        exc = np.concatenate([g.excluded() for g in gs])
        if not (np.array_equal(exc, o.excluded()) and abs(s.threshold - so.threshold) < 1e-9
                and (s.any_change, s.n_new_excluded, s.n_rescued) == (so.any_change, so.n_new_excluded, so.n_rescued)
                and np.array_equal(gs[0].loci_mask(), o.loci_mask())):
            return False
        if not so.any_change:
            break
    po = o.posteriors()
    post = np.concatenate([g.posteriors()["posterior"] for g in gs])
    ok = bool(np.allclose(post, po["posterior"], rtol=0, atol=1e-6))
    for g in gs:
        g.close()
    return ok


if __name__ == "__main__":
    main()
