"""GPU: the locus pass (tiled_locus_pass / k_locus_finalize, csrc/kernels_tiled.hip; k_locus_stats, csrc/kernels_em.hip, for
engine 1) swept over its dispatch space against an exact sum.

The other GPU files hold contrib_min / contrib_maj to the oracle at 1e-7 .. 1e-9 — the ORACLE's ln_gamma cancellation — on matrices
that reach whichever value paths the generator happens to draw.  Here every case is a matrix built by hand (tests/locus_reference.py:
the builders, the 80-bit reference and the derivation of the device's bound, all held on the CPU by tests/test_locus_reference.py), the
case asserts that it has the layout it was built for, and EVERY locus is held to

  * contrib_min and contrib_maj within locus_bound (~1e-13 .. 1e-12; ~5e-11 on the prefix-sum path at alpha + beta ~ 1e6; a zero
    bound — no entries on that side, only 0/0 entries, a masked locus — wants the device exact);
  * the six integer columns exactly (zeros at a masked locus, like the oracle), and the allele tallies of EVERY locus, masked ones
    included, through alpha_betas() after the iteration;
  * the -80 filter: no locus lies within its bound / cells_min of -80 (asserted on the reference alone), so the next loci_mask()
    and n_loci_filtered must be the reference's decision.

The inputs: set_excluded(A) and set_loci_mask(M) place the state, alpha_betas() and loci_mask() are read BEFORE the iteration and must
be the whole numbers the matrix gives for A, the new set B is placed by overwriting the NORM exchange buffer between em_begin and
em_threshold (test_gpu_tally_capacity._place), excluded() and locus_outputs() are read after it: the log-pmfs are A's, under M, split
by B (quirk Q9).  A ctx of logical shards cannot have its buffer placed: B is what a real em_iteration makes of A.

Worst observed / bound ratios are printed per case (pytest -s).
"""
import ctypes as C

import numpy as np
import pytest

import locus_reference as lr
from test_gpu_tally_capacity import _place

pytestmark = pytest.mark.gpu

LM_NUM, LM_DEN = 1, 8  # csrc/tiled.h: minority-driven when n_min / nloc <= LM_NUM / LM_DEN


@pytest.fixture(scope="module")
def mods(oracle_lib, hip_lib_path):
    from cellector_amd import Cellector, ffi
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpy.restype = C.c_int
    return dict(Cellector=Cellector, ffi=ffi, hip=hip)


# ---- references: one per (matrix, first set, mask, new set), shared by every ctx that runs it --------------------------------------
_refs = {}


def _reference(case, A, mask, B):
    key = (id(case), A.tobytes(), np.asarray(mask, np.uint8).tobytes(), B.tobytes())
    if key not in _refs:
        alpha, beta = lr.alpha_beta_of(case, A)
        _refs[key] = (alpha, beta, lr.locus_reference(case["L"], *case["coo"], alpha, beta, B, mask))
    return _refs[key]


def _form(opts):
    o = dict(opts)
    return dict(engine=o.get("engine", 2), t2=o.get("t2", 1) != 0, deep=o.get("ovf_deep", 0) != 0, shards=o.get("shards", 1))


def _load(mods, case, opts, devices=None):
    """a ctx with the options set before the ingest; t2 and ovf_deep are always forced, and the ctx must have built that form (once a
    matrix is loaded the option accepts the value that was built and refuses the other)"""
    o = dict(opts)
    g = mods["Cellector"](devices=devices) if devices else mods["Cellector"](0)
    engine = o.get("engine", 2)
    g.set_option("engine", engine)
    if engine == 2:
        o.setdefault("t2", 1)
        o.setdefault("ovf_deep", 0)
    for k, v in o.items():
        if k not in ("engine", "shards"):
            g.set_option(k, v)
    L, N = case["L"], case["N"]
    g.load_coo(L, N, *(np.ascontiguousarray(x, np.uint32) for x in case["coo"]), 0, 0)
    d = g.dims()
    assert (d.loci_used, d.total_cells, d.nnz_used) == (L, N, len(case["coo"][0]))
    if not devices:
        info = g.engine_info()
        assert info.engine == engine
        if engine == 2:
            tot = case["coo"][2] + case["coo"][3]
            n_reg = int(((tot >= 1) & (tot <= 4)).sum())
            assert (info.nnz_regular, info.nnz_overflow, info.locus_chunks) == (n_reg, len(tot) - n_reg, -(-L // lr.T_BLU))
            for key in ("t2", "ovf_deep"):
                g.set_option(key, o[key])
                with pytest.raises(mods["ffi"].CellectorError):
                    g.set_option(key, 1 - o[key])
    return g


def _state(g, case, A, mask):
    """place (A, mask); what the iteration will compute with must be what the matrix gives for A"""
    if A.any():
        g.set_excluded(A.astype(np.uint8))
    if not np.asarray(mask).all():
        g.set_loci_mask(mask)
    _assert_state(g, case, A, mask)


def _assert_state(g, case, A, mask):
    alpha, beta = lr.alpha_beta_of(case, A)
    a, b = g.alpha_betas()
    assert np.array_equal(a, alpha) and np.array_equal(b, beta) and np.array_equal(g.loci_mask(), np.asarray(mask, np.uint8))
    assert np.array_equal(g.excluded(), A.astype(np.uint8))


def _check(tag, g, case, A, mask, B, form, summary):
    """the iteration that just ran (state (A, mask), new set B) against the reference; returns (outputs, mask after the filter)"""
    alpha, beta, ref = _reference(case, A, mask, B)
    L = case["L"]
    assert np.array_equal(g.excluded(), B.astype(np.uint8))
    out = g.locus_outputs()
    live = ref["live"]
    for k in lr.KEYS:
        want = np.where(live, ref[k], 0).astype(np.uint64)
        bad = np.nonzero(out[k] != want)[0]
        assert bad.size == 0, (f"{tag}: {k} differs at {bad.size} loci, first {bad[:5]}: device {out[k][bad[:5]]}, reference {want[bad[:5]]}, "
                               f"paths {[lr.path_of_locus(ref, form, l) for l in bad[:5]]}")
    # the tallies count at masked loci too: the next alpha / beta are formed from them
    a, b = g.alpha_betas()
    for got, s, k in ((a, ref["alt_min"] + ref["alt_maj"], "alt_min"), (b, ref["ref_min"] + ref["ref_maj"], "ref_min")):
        want = (s.astype(np.float64) + 1.0) - ref[k].astype(np.float64)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, f"{tag}: {k} as alpha_betas() shows it differs at {bad[:5]} (masked: {~live[bad[:5]]})"
    worst = 0.0
    for side, bound in zip(("min", "maj"), lr.locus_bound(ref, form)):
        got, want = out["contrib_" + side], ref["contrib_" + side]
        assert np.isfinite(got).all(), tag
        d = np.abs(got - want)
        bad = np.nonzero(d > bound)[0]
        assert bad.size == 0, (f"{tag}: contrib_{side} beyond its bound at {bad.size} of {L} loci; " + "; ".join(
            f"locus {l} ({lr.path_of_locus(ref, form, l)}): device {got[l]!r}, reference {want[l]!r}, bound {bound[l]:.3e}" for l in bad[:6]))
        nz = bound > 0
        if nz.any():
            worst = max(worst, float((d[nz] / bound[nz]).max()))
    # the -80 filter (main.rs:428-451): decided outside the band of the device's error at every locus
    cm = ref["cells_min"].astype(np.float64)
    band = lr.locus_bound(ref, form)[0] / np.maximum(cm, 1.0)
    assert (np.abs(ref["per_cell"] + 80.0) > band).all()
    drop = ref["per_cell"] < -80.0
    mask_next = np.where(drop, 0, np.asarray(mask, np.uint8)).astype(np.uint8)
    assert np.array_equal(g.loci_mask(), mask_next), (tag, np.nonzero(g.loci_mask() != mask_next)[0][:8])
    assert summary.n_loci_filtered == int(drop.sum()), (tag, summary.n_loci_filtered, int(drop.sum()))
    print(f"  {tag}: worst |contrib - ref| / bound = {worst:.3f} (largest bound min {lr.locus_bound(ref, form)[0].max():.2e}, "
          f"maj {lr.locus_bound(ref, form)[1].max():.2e}); {int(drop.sum())} loci filtered, {int((~live).sum())} masked")
    return out, mask_next, worst


def _run(mods, tag, case, opts, A=None, mask=None, B=None):
    """load, place (A, mask), one iteration with the new set B, check; returns the outputs"""
    A = case["A"] if A is None else A
    mask = case["mask"] if mask is None else mask
    B = case["B"] if B is None else B
    g = _load(mods, case, opts)
    _state(g, case, A, mask)
    s = _place(mods, g, B, case["N"], quiet_filter=False)
    out, _, _ = _check(tag, g, case, A, mask, B, _form(opts), s)
    g.close()
    return out


def _same(a, b, tag):
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{tag}: {k} differs at {np.nonzero(a[k] != b[k])[0][:8]}"


def _within_both_bounds(case, a, fa, b, fb, tag):
    _, _, ref = _reference(case, case["A"], case["mask"], case["B"])
    for i, side in enumerate(("min", "maj")):
        bound = lr.locus_bound(ref, fa)[i] + lr.locus_bound(ref, fb)[i]
        d = np.abs(a["contrib_" + side] - b["contrib_" + side])
        assert (d <= bound).all(), (tag, side, np.nonzero(d > bound)[0][:8])
    for k in lr.KEYS:
        assert np.array_equal(a[k], b[k]), (tag, k)


# ---- the cases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", lr.GEOMETRY_L)
def test_locus_geometry(mods, L):
    """L around the 16-lane groups of k_locus_finalize (1, 15, 16, 17: a ragged last group, lanes clamped to locus L - 1), around the
    chunks of the regular table (638 .. 640, 1278: the first locus of the second and third chunk) and around the 4096-locus ranges of the
    minority-driven count (4095 .. 4099); loci 0, 638, 639, 640, L - 1 and both sides of 4096 carry every regular code on both sides,
    listed entries and tier-2 pairs (asserted by tests/test_locus_reference.py on the same matrices).  Tier-2 tables and the all-listed
    prefix-sum form."""
    case = lr.sweep_case("geometry-%d" % L)
    lo = case["coo"][0]
    for l in case["edges"]:
        assert (lo == l).sum() > 80
    assert -(-L // lr.LR_LOCI) == (2 if L > 4096 else 1)
    _run(mods, f"geometry L={L} t2", case, (("t2", 1),))
    _run(mods, f"geometry L={L} all listed", case, (("t2", 0),))


VALUE_FORMS = [(("t2", 1), ("ovf_deep", 0)), (("t2", 0), ("ovf_deep", 0)), (("t2", 1), ("ovf_deep", 1)), (("t2", 0), ("ovf_deep", 1))]


@pytest.mark.parametrize("name", ["features", "iteration0"])
def test_value_paths(mods, name):
    """One matrix through every value path: tier-2 tables + k_ovx_values, k_ovf_values' prefix sums, and both inline forms of
    k_locus_finalize<true>; overlap 1 / 0 / 2 where a kernel of its own stores the listed values (same kernels, same arithmetic: to
    the bit).  The feature matrix (tests/locus_reference.py: feature_matrix) carries every listed count around the 4 x 16 stride on
    either side and mixed, every total around OV_NT / OV_NE with every split (a locus whose only listed total is 5, 8 or 17: the fill
    limit of its prefix row; one whose listed totals are all >= 18 or 0: an empty row), every tier-2 pair at one locus and single pairs
    at others, alpha + beta ~ 1e6 and 1.0 beside 2.4e5, and the same block masked locus by locus and inside a masked chunk.
    "iteration0" is the same block under an empty first set: alpha / beta are totals + 1."""
    case = lr.sweep_case(name)
    n = case["coo"][2] + case["coo"][3]
    # (one feature block: 270 entries of tier-2 totals, 976 of 9..17, 160 of 0/0, thousands above 17)
    assert ((n >= 5) & (n <= 8)).sum() >= 270 and ((n > 8) & (n < 18)).sum() >= 976 and (n >= 18).sum() > 1000 and (n == 0).sum() >= 160
    assert case["A"].any() == (name == "features")
    outs = {}
    for opts in VALUE_FORMS:
        tag = f"{name} " + ",".join(f"{k}={v}" for k, v in opts)
        outs[opts] = _run(mods, tag, case, opts)
        if dict(opts)["ovf_deep"] == 0:
            for overlap in (0, 2):
                _same(outs[opts], _run(mods, f"{tag},overlap={overlap}", case, opts + (("overlap", overlap),)), f"{tag}: overlap {overlap}")
    base = VALUE_FORMS[0]
    for opts in VALUE_FORMS[1:]:
        _within_both_bounds(case, outs[base], _form(base), outs[opts], _form(opts), f"{name}: {opts} against {base}")


def _tally_plan(mode, valid, n_min, n_add, n_res, nloc, cap):
    """tally_plan (csrc/kernels_tiled.hip) restated: which form counts the exclusion set"""
    if valid:
        chg = n_add + n_res
        if chg == 0:
            return "kept"
        if chg <= n_min and chg * LM_DEN <= nloc * LM_NUM and n_add <= cap and n_res <= cap:
            return "delta"
    if n_min <= cap and (mode == 2 or (mode == 0 and n_min * LM_DEN <= nloc * LM_NUM)):
        return "fresh"
    return "stream"


@pytest.mark.parametrize("name", ["geometry-4099", "features"])
def test_exclusion_set_forms(mods, name):
    """Four iterations on six ctxs (locus_mode 1 / 2 / 0 x tally_delta 1 / 0): the matrix' set B (160 cells, below N / 8); B less 15
    cells plus 25 others (a change of 40: a signed delta on the kept counts where they are kept); 400 other cells (above N / 8, a change
    larger than the set: a recount); the same 400 again (no change: the kept counts as they are).  Which form counts is decided on
    the device; tally_plan is restated here and the arms each ctx takes are asserted to be the intended ones.  Every iteration of every
    ctx against the reference; the outputs of all six ctxs to the bit (k_locus_finalize: "both forms end here, so they agree to
    the bit")."""
    case = lr.sweep_case(name)
    N, L = case["N"], case["L"]
    rng = np.random.default_rng(3)
    B1 = case["B"]
    B2 = B1.copy()
    B2[rng.choice(np.nonzero(B1)[0], 15, replace=False)] = False
    B2[rng.choice(np.nonzero(~B1[:lr.POOL] & ~case["A"][:lr.POOL])[0], 25, replace=False)] = True
    B3 = np.zeros(N, bool)
    B3[rng.choice(np.nonzero(~B2[:lr.POOL])[0], 400, replace=False)] = True
    sets = [B1, B2, B3, B3]
    assert B1.sum() * LM_DEN < N < B3.sum() * LM_DEN and B3.sum() < N / 4
    # a subset of k_minority_ranges holds at most 65535 / (the most lines a pair has) cells, and there is at least one: every set fits
    lo, ce = case["coo"][0], case["coo"][1]
    cap = 65535 // int(np.unique(lo * N + ce, return_counts=True)[1].max())
    assert cap > 400
    want_arms = {(1, 1): ["stream", "delta", "stream", "kept"], (2, 1): ["fresh", "delta", "fresh", "kept"],
                 (0, 1): ["fresh", "delta", "stream", "kept"], (1, 0): ["stream"] * 4, (2, 0): ["fresh"] * 4,
                 (0, 0): ["fresh", "fresh", "stream", "stream"]}
    ctxs = {}
    for mode in (1, 2, 0):
        for delta in (1, 0):
            g = _load(mods, case, (("locus_mode", mode), ("tally_delta", delta)))
            _state(g, case, case["A"], case["mask"])
            ctxs[(mode, delta)] = g
    prev, mask = case["A"], case["mask"]
    for it, B in enumerate(sets):
        outs = {}
        for (mode, delta), g in ctxs.items():
            arm = _tally_plan(mode, delta and it > 0, int(B.sum()), int((B & ~prev).sum()), int((prev & ~B).sum()), N, cap)
            assert arm == want_arms[(mode, delta)][it], (mode, delta, it, arm)
            _assert_state(g, case, prev, mask)
            s = _place(mods, g, B, N, quiet_filter=False)
            assert (s.n_new_excluded, s.n_rescued) == (int((B & ~prev).sum()), int((prev & ~B).sum()))
            outs[(mode, delta)], mask_next, _ = _check(f"{name} iteration {it} locus_mode {mode} tally_delta {delta} ({arm})", g, case, prev,
                                                        mask, B, _form(()), s)
        for key, o in outs.items():
            _same(outs[(1, 1)], o, f"{name} iteration {it}: locus_mode / tally_delta {key} against (1, 1)")
        prev, mask = B, mask_next
    for g in ctxs.values():
        g.close()


def test_entry_width_and_filter_placement(mods):
    """compact_bits 32 (the 32-bit compact entries k_locus_stats2<true, 32> decodes) against the default 24 under the streamed count,
    and the -80 filter as a kernel of its own (fuse_filter 0) against the fused one: each against the reference, all to the bit.  The
    filter's cases are the feature matrix': a locus far below -80, one that would be but is masked already (it stays masked and is not
    counted again), one without minority entries (per_cell 0)."""
    case = lr.sweep_case("features")
    _, _, ref = _reference(case, case["A"], case["mask"], case["B"])
    below = case["roles"]["below_filter"]
    assert ref["per_cell"][below[0]] < -150 and not case["mask"][below[1]] and ref["cells_min"][below[1]] == 0
    assert ref["cells_min"][case["roles"]["no_minority"][0]] == 0 and (ref["per_cell"][case["mask"] != 0] > -80.0).sum() > 100
    base = _run(mods, "features locus_mode=1", case, (("locus_mode", 1),))
    for opts in ((("locus_mode", 1), ("compact_bits", 32)), (("locus_mode", 1), ("fuse_filter", 0)), (("fuse_filter", 0), ("compact_bits", 32))):
        tag = "features " + ",".join(f"{k}={v}" for k, v in opts)
        _same(base, _run(mods, tag, case, opts), tag)


@pytest.mark.parametrize("name", lr.SWEEP_CASES)
def test_engine_1(mods, name):
    """k_locus_stats: a wave per locus, every entry in product form, ceil(n / 64) additions a lane and a 6-step butterfly"""
    case = lr.sweep_case(name)
    _run(mods, f"{name} engine 1", case, (("engine", 1),))


@pytest.mark.parametrize("name", ["geometry-4099", "features"])
def test_logical_shards(mods, name):
    """Cellector(devices=[0, 0, 0]): three shards of the cells on one GPU, the locus sums all-reduced (one more addition per shard in
    the bound), the filter after the exchange.  The NORM buffer of such a ctx cannot be placed: the new set is what a real iteration
    makes of A, read back with excluded().  (On the MI355X that iteration excludes 16 cells of the L = 4099 matrix and none of the
    feature matrix: there every entry is on the majority side, the minority sums must be exactly zero.)"""
    case = lr.sweep_case(name)
    g = _load(mods, case, (), devices=[0, 0, 0])
    A, mask = case["A"], case["mask"]
    _state(g, case, A, mask)
    s = g.em_iteration(5.0)
    B = g.excluded() != 0
    print(f"  {name}: the iteration excluded {int(B.sum())} cells ({s.n_new_excluded} new, {s.n_rescued} rescued)")
    _check(f"{name} three shards", g, case, A, mask, B, _form((("shards", 3),)), s)
    g.close()
