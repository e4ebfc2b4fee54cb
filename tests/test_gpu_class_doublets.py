"""GPU: K-class doublet scoring (cellector_class_pair_alpha_betas / _class_doublets / cellector_refine_class_doublets; the second
half of csrc/kernels_classes.hip) on both engines, against tests/class_doublet_reference.py and the numpy twin
cellector_amd/classes.py.

Pair alpha / beta are exact claims (np.array_equal), for K = 2 with reference_doublet_scales the bits of
posterior_alpha_betas(2).  Every ll_k and ll_ab is held to the bound of its sum, every posterior and doublet_posterior to its
relative bound (class_doublet_reference's docstring derives them; tests/test_class_doublet_reference.py shows on the CPU what
they let be seen and that the inputs leave at most 1 cell in 1000 out of a comparison); best, best_pair, call and qual are exact
outside their bands.  K = 2 is also held against cellector_posteriors on the same ctx within the two bounds added.

Refine: labels, held flags and summaries after max_iter = 0, 1, ... from one start equal the twin's trajectory driven by the 80-bit
sums, step by step (no cell of any step is inside a band: the CPU test); class_delta 0 and 1 give the same bits, n_recounts
apart.  What share of the planted doublets the twin holds is measured on the CPU; the comparison here is with the twin.
"""
import numpy as np
import pytest

import class_doublet_reference as dr
import class_reference as cr
import posterior_reference as pr
import test_gpu_classes as TC
import test_gpu_posterior_sweep as PS
import test_gpu_tile_sweep as S

pytestmark = pytest.mark.gpu

ENGINES = TC.ENGINES
OUT = ("ll", "ll_pair", "posterior", "doublet_posterior", "best", "best_pair", "call", "qual")


@pytest.fixture(scope="module")
def mods(oracle_lib, hip_lib_path):
    import torch
    from cellector_amd import Cellector, classes, ffi
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    return dict(Cellector=Cellector, ffi=ffi, cl=classes, ob=oracle_lib, ncu=ncu)


def _same(a, b, tag, keys=OUT):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), (tag, k)


# ---- pair alpha / beta: exact ----------------------------------------------------------------------------------------------------
def _states(N, seed):
    """(name, K, labels, held): a held set, an empty class in the middle, K = 16, K = 1"""
    rng = np.random.default_rng(seed)
    out = []
    for K in (1, 2, 3, 16):
        lab = rng.integers(0, K, N).astype(np.uint8)
        lab[rng.random(N) < 0.1] = cr.UNLABELLED
        held = (rng.random(N) < 0.2).astype(np.uint8)
        if (dr.unheld(lab, held) == cr.UNLABELLED).all():
            lab[0], held[0] = 0, 0
        out.append((f"K{K} draw, held set", K, lab, held))
        out.append((f"K{K} draw, none held", K, lab, None))
    mid = np.where(np.arange(N) % 3 == 0, 0, 2).astype(np.uint8)
    out.append(("empty class in the middle", 3, mid, None))
    # class 1 exists only in held cells: dead once they are out
    lab = (np.arange(N) % 3).astype(np.uint8)
    out.append(("a class that is held away", 3, lab, (lab == 1).astype(np.uint8)))
    return out


@ENGINES
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_pair_alpha_betas_are_exact(mods, engine, N):
    L, N, coo = TC._row_matrix(N, seed=N)
    g = TC._make(mods, engine, L, N, coo)
    Lu, coo_u = TC._used(g, L, coo)
    cl = mods["cl"]
    scale = [1.0, 0.01, 0.07] + [0.5] * 13
    for name, K, lab, held in _states(N, seed=11 * N):
        tag = f"{N} cells, engine {engine}, {name}"
        cells, alt, ref = cr.tallies(Lu, coo_u, dr.unheld(lab, held), K)
        for ps in (None, scale[:K]):
            got = g.class_pair_alpha_betas(lab, K, held=held, pair_scale=ps)
            assert got["alpha"].shape == (dr.n_pairs(K), Lu)
            used = dr.default_pair_scales(cells, K) if ps is None else ps
            want = dr.pair_alpha_betas(alt[:K], ref[:K], used)
            for p in range(dr.n_pairs(K)):
                assert np.array_equal(got["alpha"][p], want[p][0]) and np.array_equal(got["beta"][p], want[p][1]), (tag, p)
            ta, tb = cl.class_pair_alpha_betas(alt[:K], ref[:K], cl.balanced_pair_scales(cells[:K]) if ps is None else ps)
            assert np.array_equal(got["alpha"], ta) and np.array_equal(got["beta"], tb), tag
        if held is None and N >= 63:  # the singlet columns are class_posteriors' bits
            d, c = g.class_doublets(lab, K, scale=scale[:K]), g.class_posteriors(lab, K, scale[:K])
            assert d["ll"].tobytes() == c["ll"].tobytes(), tag
    g.close()


# ---- every cell against the reference ------------------------------------------------------------------------------------------------
def _call(g, ref, K):
    a = ref["args"]
    return g.class_doublets(ref["labels"], K, held=a["held"], scale=a["scale"], pair_scale=a["pair_scale"], log_prior=a["log_prior"],
                            log_pair_prior=a["log_pair_prior"], mask=a["mask"])


@pytest.mark.parametrize("mname,engine,opts", PS.SWEEP,
                         ids=[f"{m}-engine{e}" + "".join(f"-{k}{v}" for k, v in o if k != "ovf_deep") for m, e, o in PS.SWEEP])
def test_every_cell_against_the_reference(mods, mname, engine, opts):
    """One ctx per (matrix, engine, options).  K = 2 from the matrix' exclusion sets with reference_scales and
    reference_doublet_scales, K = 3 and K = 5 from seeded draws with 5 % unlabelled and 5 % held, each with all loci and under a
    mask; K = 16 (120 pairs) once per engine, on row-lengths; forced tile_sb 2 / 4: the same bits."""
    g, G = PS._load(mods, mname, engine, opts)
    L, N, coo, _ = pr.matrix(mname)
    worst = {}
    for K, which in dr.case_names(mname):
        for masked in (False, True):
            ref = dr.case(mname, K, which, masked)
            tag = f"{mname} engine {engine} {dict(opts).get('t2_tiles', '')} K {K} {which} {'masked' if masked else 'all loci'}"
            got = _call(g, ref, K)
            res = dr.compare(ref, got, G)
            print(f"  {tag}: worst observed / bound " + ", ".join(f"{k} {res[k][0]:.3f}" for k in OUT[:4]) + f"; compared: best "
                  f"{res['best'][0]}, best_pair {res['best_pair'][0]}, call {res['call'][0]}, qual {res['qual'][0]} of {N} cells (qual on "
                  f"an integer edge in {res['qual_edges']}); left out of a comparison {res['left_out']}")
            assert dr.ok(res), f"{tag}: " + dr.describe(ref, got, res)
            for k in OUT[:4]:
                worst[k] = max(worst.get(k, 0.0), res[k][0])
            if engine == 2 and K != 16:
                for sb in (2, 4, 0):
                    g.set_option("tile_sb", sb)
                    _same(got, _call(g, ref, K), f"{tag}: tile_sb {sb}")
            if K == 2 and not masked:  # calculate_posteriors on the same ctx: the same model, another order of operations
                g.set_excluded(ref["labels"] == 0)
                two, tref = g.posteriors(), pr.case(mname, which)
                ps, lpp = mods["cl"].reference_doublet_scales(int((ref["labels"] == 0).sum()), N)
                assert list(ps) == ref["ps"] and abs(lpp[0] - ref["lpp"][0]) <= np.spacing(abs(lpp[0]))
                pa, pb = g.posterior_alpha_betas(2)
                pab = g.class_pair_alpha_betas(ref["labels"], 2, pair_scale=ps)
                assert np.array_equal(pab["alpha"][0], pa) and np.array_equal(pab["beta"][0], pb), tag
                b, b2 = dr.bounds(ref, G), pr.bounds(tref, G)
                for name, mine, rel, want in (("posterior", got["posterior"][0], b["rel"][0] + b2["rel_p"], ref["chain"]["posterior"][0]),
                                              ("doublet_posterior", got["doublet_posterior"], b["rel_d"] + b2["rel_d"],
                                               ref["chain"]["doublet_posterior"])):
                    seen = want >= pr.OBSERVABLE
                    d = np.abs(mine - two[name])[seen] / want[seen].astype(np.float64)
                    assert (d <= rel[seen]).all(), (tag, name, float((d / rel[seen]).max()))
                    assert (two[name][~seen] < pr.UNOBSERVED_BELOW).all() and (mine[~seen] < pr.UNOBSERVED_BELOW).all()
    print(f"  {mname} engine {engine} {dict(opts)}: G = {G}; worst over the cases " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    g.close()


@ENGINES
def test_dead_class_dead_pairs_and_k1(mods, engine):
    L, N, coo, _ = pr.matrix("tier2")
    g = TC._make(mods, engine, L, N, coo)
    lab = np.where(np.arange(N) % 5 == 0, 0, 2).astype(np.uint8)
    lab[3::11] = cr.UNLABELLED
    held = (np.arange(N) % 17 == 0).astype(np.uint8)
    ref = dr.reference(L, N, coo, lab, 3, held)
    got = g.class_doublets(lab, 3, held=held)
    assert np.isneginf(got["ll"][1]).all() and (got["posterior"][1] == 0).all() and not (got["best"] == 1).any()
    assert np.isneginf(got["ll_pair"][0]).all() and np.isneginf(got["ll_pair"][2]).all() and np.isfinite(got["ll_pair"][1]).all()
    assert (got["best_pair"] == [0, 2]).all()
    res = dr.compare(ref, got, cr.g_any(L))
    assert dr.ok(res), dr.describe(ref, got, res)
    # class 1 lives in held cells only: dead all the same
    lab1 = lab.copy()
    lab1[held != 0] = 1
    got1 = g.class_doublets(lab1, 3, held=held)
    assert np.isneginf(got1["ll"][1]).all() and got1["ll"].tobytes() == got["ll"].tobytes()
    _same(got, got1, "held away")
    r = g.refine_class_doublets(lab, 3, held=held, max_iter=3)
    assert r["summary"].class_cells[1] == 0 and not (r["labels"] == 1).any()
    # K = 1: no pair
    one = np.zeros(N, np.uint8)
    k1 = g.class_doublets(one, 1)
    assert k1["ll_pair"].shape == (0, N) and (k1["doublet_posterior"] == 0).all() and (k1["best_pair"] == 255).all()
    assert (k1["call"] == 0).all() and (k1["posterior"] == 1.0).all() and (k1["qual"] == 255).all()
    assert k1["ll"].tobytes() == g.class_posteriors(one, 1)["ll"].tobytes()
    assert g.class_pair_alpha_betas(one, 1)["alpha"].shape == (0, L)
    r1 = g.refine_class_doublets(one, 1, max_iter=2)
    assert r1["summary"].converged == 1 and r1["summary"].n_held == 0 and not r1["held"].any()
    with pytest.raises(mods["ffi"].CellectorError, match="every labelled cell is held"):
        g.class_doublets(lab, 3, held=np.ones(N, np.uint8))
    g.close()


# ---- refine ------------------------------------------------------------------------------------------------------------------------
_twins = {}


def _twin(mods, which, rate, max_iter, min_loci=1, class_delta=True):
    key = (which, rate, max_iter, min_loci, class_delta)
    if key not in _twins:
        L, N, coo, _, _ = dr.doublet_mixture(rate)
        start, K = dr.doublet_start(which, rate)
        _twins[key] = mods["cl"].refine_doublets(L, coo, start, K, cr.ll_fn_80bit(N, coo), max_iter=max_iter, min_loci=min_loci,
                                                 class_delta=class_delta)
    return _twins[key]


def _summary(s):
    return dict(iterations=s.iterations, converged=s.converged, n_moved_last=s.n_moved_last, n_moved_total=s.n_moved_total,
                n_recounts=s.n_recounts, class_cells=list(s.class_cells), n_held=s.n_held)


def _twin_summary(tw):
    return dict(tw["summary"], class_cells=[int(x) for x in tw["summary"]["class_cells"]])


REFINE_OUT = ("ll", "ll_pair", "posterior", "doublet_posterior", "best_pair", "qual")


@ENGINES
@pytest.mark.parametrize("rate", dr.RATES)
@pytest.mark.parametrize("which", dr.DOUBLET_STARTS)
def test_refine_follows_the_twin(mods, engine, which, rate):
    """class_reference.mixture() (three genotypes, 900 cells x 600 loci, six one-entry cells) plus 60 synthetic cross-genotype
    doublets whose parents are thinned at `rate`, from the truth and from a noisy labelling.  What the twin finds at the fixed
    point is in tests/test_class_doublet_reference.py's docstring."""
    L, N, coo, _, _ = dr.doublet_mixture(rate)
    start, K = dr.doublet_start(which, rate)
    g = TC._make(mods, engine, L, N, coo)
    assert g.dims().loci_used == L
    full = _twin(mods, which, rate, 20)
    n_steps = full["summary"]["iterations"]
    for max_iter in list(range(0, n_steps + 1)) + [20]:
        tw = _twin(mods, which, rate, max_iter)
        for delta in (1, 0):
            g.set_option("class_delta", delta)
            r = g.refine_class_doublets(start, K, max_iter=max_iter)
            want = _twin_summary(_twin(mods, which, rate, max_iter, class_delta=bool(delta)))
            assert _summary(r["summary"]) == want, (which, rate, engine, max_iter, delta, _summary(r["summary"]), want)
            assert np.array_equal(r["labels"], tw["labels"]) and np.array_equal(r["held"], tw["held"]), (which, rate, engine, max_iter, delta)
            if delta:
                first = r
            else:  # a recount every step: the same integers, so the same bits everywhere
                _same(r, first, (which, rate, max_iter), REFINE_OUT)
                assert np.array_equal(r["labels"], first["labels"]) and np.array_equal(r["held"], first["held"])
                if max_iter >= 2:
                    assert r["summary"].n_recounts == r["summary"].iterations > first["summary"].n_recounts == 1
        # the last step's outputs: those of class_doublets on the (labels, held) that step started from
        last = g.class_doublets(tw["steps"][-1]["labels_in"], K, held=tw["steps"][-1]["held_in"])
        _same(first, last, (which, rate, max_iter), REFINE_OUT)
    # min_loci 2: the one-entry cells keep their labels and flags; the twin agrees
    g.set_option("class_delta", 1)
    r2, t2 = g.refine_class_doublets(start, K, max_iter=20, min_loci=2), _twin(mods, which, rate, 20, min_loci=2)
    one = slice(cr.MIX_N, cr.MIX_N + 6)
    assert np.array_equal(r2["labels"], t2["labels"]) and np.array_equal(r2["held"], t2["held"])
    assert np.array_equal(r2["labels"][one], start[one]) and not r2["held"][one].any()
    assert _summary(r2["summary"]) == _twin_summary(t2)
    assert np.array_equal(start, dr.doublet_start(which, rate)[0])  # the caller's array is not written
    # the caller's arrays are not written on a refusal (the raw ABI writes into what it is given)
    lib, ffi = mods["ffi"].load_library(), mods["ffi"]
    lab, held = start.copy(), np.zeros(N, np.uint8)
    held[5] = 7
    st = lib.cellector_refine_class_doublets(g.h, ffi._p(lab), ffi._p(held), K, None, None, None, None, None, 1.5, 3, 1,
                                             None, None, None, None, None, None, None)
    assert st == 1 and b"doublet_threshold" in lib.cellector_last_error(g.h)
    assert np.array_equal(lab, start) and held[5] == 7 and held.sum() == 7
    g.close()


# ---- independence from the existing calls ------------------------------------------------------------------------------------------------
@ENGINES
def test_refine_classes_is_unchanged_by_a_doublet_call(mods, engine):
    L, N, coo, _ = cr.mixture()
    start, K = cr.refine_start("noisy")
    g = TC._make(mods, engine, L, N, coo)
    before = g.refine_classes(start, K, max_iter=20)
    held = (np.arange(N) % 7 == 0).astype(np.uint8)
    g.class_doublets(start, K, held=held)
    g.refine_class_doublets(start, K, held=held, max_iter=2)
    g.class_pair_alpha_betas(start, K, held=held)
    after = g.refine_classes(start, K, max_iter=20)
    for k in ("labels", "ll", "posterior", "qual"):
        assert before[k].tobytes() == after[k].tobytes(), k
    assert bytes(before["summary"]) == bytes(after["summary"])
    g.close()


@ENGINES
@pytest.mark.parametrize("mname", ["tier2", "row-lengths"])
def test_doublet_calls_leave_the_loop_alone(mods, mname, engine):
    opts = PS.DEEP[8] if (engine == 2 and mname == "tier2") else ()
    L, N, coo, _ = pr.matrix(mname)
    x, y = TC._make(mods, engine, L, N, coo, opts), TC._make(mods, engine, L, N, coo, opts)
    want = x.run(5.0, 40)
    assert not want[-1].any_change
    want.append(x.em_iteration(5.0))  # (one more at the fixed point: at least two iterations in all)
    lab, held = dr.case_inputs(mname, 3, "draw")[:2]
    got = []
    for it in range(len(want)):
        got.append(y.em_iteration(5.0))
        if it == 1:
            state = (y.excluded(), y.loci_mask())
            y.class_doublets(lab, 3, held=held, mask=cr.case_mask(mname))
            y.refine_class_doublets(lab, 3, held=held, max_iter=2)
            y.class_pair_alpha_betas(lab, 3, held=held)
            assert np.array_equal(y.excluded(), state[0]) and np.array_equal(y.loci_mask(), state[1])
    assert [bytes(s) for s in got] == [bytes(s) for s in want], (mname, engine)
    assert np.array_equal(x.excluded(), y.excluded()) and np.array_equal(x.loci_mask(), y.loci_mask())
    for k, v in x.cell_outputs().items():
        assert v.tobytes() == y.cell_outputs()[k].tobytes(), k
    x.close(); y.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(mods):
    ffi = mods["ffi"]
    L, N, coo = TC._row_matrix(65, seed=65)
    lab = (np.arange(N) % 3).astype(np.uint8)

    def refused(fn, match):
        with pytest.raises(ffi.CellectorError, match=match) as e:
            fn()
        assert e.value.status == 1

    def every_call(g, match, n=N):
        l = lab[:n]
        refused(lambda: g.class_pair_alpha_betas(l, 3), match)
        refused(lambda: g.class_doublets(l, 3), match)
        refused(lambda: g.refine_class_doublets(l, 3), match)

    g = TC._make(mods, 2, L, N, coo)
    for K in (0, 17):
        refused(lambda: g.class_pair_alpha_betas(np.zeros(N, np.uint8), K), "1..16 are supported")
        refused(lambda: g.refine_class_doublets(np.zeros(N, np.uint8), K), "1..16 are supported")
    bad = lab.copy()
    bad[5], bad[9] = 3, 200
    for fn in (g.class_pair_alpha_betas, g.class_doublets, g.refine_class_doublets):
        refused(lambda: fn(bad, 3), "cell 5 has label 3")
    for s in ([1.0, -0.5, 1.0], [1.0, np.inf, 1.0], [np.nan, 1.0, 1.0]):
        refused(lambda: g.class_pair_alpha_betas(lab, 3, pair_scale=s), r"pair_scale\[\d\]")
        refused(lambda: g.class_doublets(lab, 3, pair_scale=s), r"pair_scale\[\d\]")
        refused(lambda: g.refine_class_doublets(lab, 3, pair_scale=s), r"pair_scale\[\d\]")
        refused(lambda: g.class_doublets(lab, 3, scale=s), r" scale\[\d\]")
    refused(lambda: g.class_doublets(lab, 3, log_pair_prior=[0.0, 0.0, np.nan]), r"log_pair_prior\[2\] is NaN")
    refused(lambda: g.refine_class_doublets(lab, 3, log_pair_prior=[np.nan, 0.0, 0.0]), r"log_pair_prior\[0\] is NaN")
    refused(lambda: g.class_doublets(lab, 3, log_prior=[0.0, np.nan, 0.0]), r"log_prior\[1\] is NaN")
    for t in (-0.1, 1.5, np.nan):
        refused(lambda: g.refine_class_doublets(lab, 3, doublet_threshold=t), "doublet_threshold")
    refused(lambda: g.refine_class_doublets(lab, 3, min_loci=0), "min_loci")
    refused(lambda: g.class_doublets(lab, 3, held=np.ones(N, np.uint8)), "every labelled cell is held")
    lib = ffi.load_library()
    assert lib.cellector_class_doublets(g.h, None, None, 3, *([None] * 13)) == 1 and b"null labels" in lib.cellector_last_error(g.h)
    g.em_begin()
    every_call(g, "in flight")
    g.em_threshold(5.0)
    every_call(g, "in flight")
    g.em_finish()
    # usable afterwards: -inf priors are legal (those terms are exactly 0); thresholds 0 and 1 are legal
    out = g.class_doublets(lab, 3, log_pair_prior=[0.0, -np.inf, 0.0], log_prior=[0.0, -np.inf, 0.0])
    assert (out["posterior"][1] == 0).all() and np.isfinite(out["doublet_posterior"]).all() and bad[5] == 3
    assert g.refine_class_doublets(lab, 3, max_iter=2, doublet_threshold=1.0)["summary"].n_held == 0
    assert g.refine_class_doublets(lab, 3, max_iter=1, doublet_threshold=0.0)["summary"].iterations == 1
    g.close()
    g = mods["Cellector"](0)
    every_call(g, "no matrix loaded")
    g.close()
    m = mods["Cellector"](devices=[0, 0])
    m.load_coo(L, N, *S._u32(coo), 0, 0)
    every_call(m, "single-device")
    assert m.em_iteration(5.0) is not None
    m.close()
    g = mods["Cellector"](0)
    g.set_shard(10, 40)
    g.load_coo(L, N, *S._u32(coo), 0, 0)
    every_call(g, "set_shard", n=30)
    g.close()
