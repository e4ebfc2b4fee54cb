"""GPU: K-genotype class scoring (cellector_class_tallies / _class_alpha_betas / _class_posteriors / cellector_refine_classes;
csrc/kernels_classes.hip) on both engines, against tests/class_reference.py and the numpy twin cellector_amd/classes.py.

Tallies and alpha / beta are exact claims (np.array_equal).  Every ll_k is held to the bound of its sum and every posterior to
its relative bound (class_reference's docstring derives both; tests/test_class_reference.py shows on the CPU what they let be
seen); best and qual are exact outside the margin band.  K = 2 with reference_scales is also held against cellector_posteriors on
the same ctx: ll_minority / ll_majority come out bit-identical to the two class columns on engine 1 and on engine 2 (the same
tables, the same tile pass), which is what is asserted.

Refine: the labels after max_iter = 1, 2, ... from one start equal the twin's trajectory driven by the 80-bit sums, step by step
(no cell of any step is inside the band: tests/test_class_reference.py), and so does the summary; class_delta 0 and 1 give the same
labels, ll bits and summaries, n_recounts apart.  The twin's final labels equal the planted truth in every labelled cell (share
1.0, measured on the CPU); the comparison here is with the twin, not with a threshold.
"""
import os

import numpy as np
import pytest

import class_reference as cr
import posterior_reference as pr
import test_gpu_posterior_sweep as PS
import test_gpu_tile_sweep as S

pytestmark = pytest.mark.gpu

ENGINES = pytest.mark.parametrize("engine", [2, 1], ids=["tiled", "csr"])
ROW_LENGTHS = (0, 1, 63, 64, 65, 200)


@pytest.fixture(scope="module")
def mods(oracle_lib, hip_lib_path):
    import torch
    from cellector_amd import Cellector, classes, ffi
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    return dict(Cellector=Cellector, ffi=ffi, cl=classes, ob=oracle_lib, ncu=ncu)


def _make(mods, engine, L, N, coo, opts=(), min_alt=0, min_ref=0):
    g = mods["Cellector"](0)
    g.set_option("engine", engine)
    for k, v in opts:
        g.set_option(k, v)
    g.load_coo(L, N, *S._u32(coo), min_alt, min_ref)
    return g


def _used(g, L, coo):
    """the COO over the ctx's used loci (compact index), and their number"""
    ids = g.locus_ids().astype(np.int64)
    to_used = np.full(L, -1, np.int64)
    to_used[ids] = np.arange(len(ids))
    lo, ce, al, re = (np.asarray(x, np.int64) for x in coo)
    keep = to_used[lo] >= 0
    return len(ids), [to_used[lo[keep]], ce[keep], al[keep], re[keep]]


# ---- tallies and alpha / beta: exact ---------------------------------------------------------------------------------------------
def _row_matrix(N, seed):
    """cell i has ROW_LENGTHS[(i + 1) % 6] entries over 200 loci (cell 0: one entry), one (locus, cell) pair of cell 2 repeated"""
    L = 200
    rng = np.random.default_rng(seed)
    lo, ce = [], []
    for i in range(N):
        k = ROW_LENGTHS[(i + 1) % 6]
        lo.append(np.sort(rng.choice(L, k, replace=False)))
        ce.append(np.full(k, i))
    lo, ce = np.concatenate(lo), np.concatenate(ce)
    if N > 2:  # cell 2 has 64 entries: its first line once more, with other counts
        j = np.nonzero(ce == 2)[0][0]
        lo, ce = np.concatenate([lo, [lo[j]]]), np.concatenate([ce, [2]])
    tot = rng.geometric(0.5, len(lo))
    al = rng.binomial(tot, 0.4)
    return L, N, [lo, ce, al, tot - al]


def _labellings(N, seed):
    rng = np.random.default_rng(seed)
    out = []
    for K in (1, 2, 3, 16):
        lab = rng.integers(0, K, N).astype(np.uint8)
        lab[rng.random(N) < 0.1] = cr.UNLABELLED
        if (lab == cr.UNLABELLED).all():
            lab[0] = 0
        out.append((f"K{K} draw", K, lab))
    out.append(("all in class 1", 3, np.full(N, 1, np.uint8)))  # the class that is not walked carries everything
    one = np.full(N, cr.UNLABELLED, np.uint8)
    one[N // 2] = 2
    out.append(("all unlabelled but one", 3, one))
    out.append(("empty class in the middle", 3, np.where(np.arange(N) % 3 == 0, 0, 2).astype(np.uint8)))
    return out


def _check_tallies(tag, g, Lu, coo_u, K, lab, cl):
    cells, alt, ref = g.class_tallies(lab, K)
    wc, wa, wr = cr.tallies(Lu, coo_u, lab, K)
    assert np.array_equal(cells, wc[:K].astype(np.uint64)), tag
    assert np.array_equal(alt, wa[:K]) and np.array_equal(ref, wr[:K]), tag
    lc = g.locus_counts()  # (sum ref, sum alt): the conservation law, slot K from the reference
    assert np.array_equal(alt.sum(axis=0) + wa[K], lc[:, 1].astype(np.uint64)), tag
    assert np.array_equal(ref.sum(axis=0) + wr[K], lc[:, 0].astype(np.uint64)), tag
    scale = [1.0, 0.01, 0.07] + [0.5] * 13
    a, b = g.class_alpha_betas(lab, K, scale[:K])
    for k, (wa_k, wb_k) in enumerate(cr.alpha_betas(wa[:K], wr[:K], scale[:K])):
        assert np.array_equal(a[k], wa_k) and np.array_equal(b[k], wb_k), (tag, k)
    ta, tb = cl.class_alpha_betas(alt, ref, scale[:K])
    assert np.array_equal(a, ta) and np.array_equal(b, tb), tag
    a1, b1 = g.class_alpha_betas(lab, K)
    assert np.array_equal(a1, alt.astype(np.float64) + 1.0) and np.array_equal(b1, ref.astype(np.float64) + 1.0), tag


@ENGINES
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_tallies_and_alpha_betas_are_exact(mods, engine, N):
    L, N, coo = _row_matrix(N, seed=N)
    g = _make(mods, engine, L, N, coo)
    Lu, coo_u = _used(g, L, coo)
    assert g.dims().nnz_used == len(coo_u[0]) == len(coo[0])
    for name, K, lab in _labellings(N, seed=7 * N):
        _check_tallies(f"{N} cells, engine {engine}, {name}", g, Lu, coo_u, K, lab, mods["cl"])
    g.close()


@ENGINES
def test_a_tally_beyond_32_bits(mods, engine):
    """140 000 cells with alt = 65535 at locus 0 and a few ordinary loci.  A WALKED class of 66 000 cells sums to 4.3e9 > 2^32 by
    atomics (beside a larger class that is not walked), and the class that is not walked passes 2^33 by the subtraction."""
    N, L = 140_000, 5
    rng = np.random.default_rng(3)
    lo = np.concatenate([np.zeros(N, np.int64), rng.integers(1, L, 3 * N)])
    ce = np.concatenate([np.arange(N), rng.integers(0, N, 3 * N)])
    al = np.concatenate([np.full(N, 65535), rng.integers(0, 4, 3 * N)])
    re = np.concatenate([np.ones(N, np.int64), rng.integers(0, 4, 3 * N)])
    order = np.lexsort((ce, lo))
    coo = [x[order] for x in (lo, ce, al, re)]
    g = _make(mods, engine, L, N, coo, min_alt=4, min_ref=4)
    Lu, coo_u = _used(g, L, coo)
    assert Lu == L
    walked = np.full(N, cr.UNLABELLED, np.uint8)
    walked[rng.permutation(N)[:70_500]] = 0
    walked[np.nonzero(walked == cr.UNLABELLED)[0][:66_000]] = 1
    nearly_all = np.zeros(N, np.uint8)
    nearly_all[::1400] = 1
    draw = rng.choice(3, N, p=[0.2, 0.2, 0.6]).astype(np.uint8)
    draw[rng.random(N) < 0.02] = cr.UNLABELLED
    for name, K, lab in (("walked", 2, walked), ("nearly all", 2, nearly_all), ("draw", 3, draw)):
        cells, alt, ref = g.class_tallies(lab, K)
        wc, wa, wr = cr.tallies(Lu, coo_u, lab, K)
        assert np.array_equal(alt, wa[:K]) and np.array_equal(ref, wr[:K]) and np.array_equal(cells, wc[:K].astype(np.uint64)), name
        assert int(alt[:, 0].sum() + wa[K, 0]) == N * 65535, name
    cells, alt, _ = g.class_tallies(walked, 2)
    assert cells.tolist() == [70_500, 66_000] and int(alt[1, 0]) == 66_000 * 65535 > 2 ** 32
    assert int(g.class_tallies(nearly_all, 2)[1][0, 0]) == (N - 100) * 65535 > 2 ** 33
    g.close()


# ---- class_posteriors on the hand-built matrices ---------------------------------------------------------------------------------
def _got(res):
    return dict(ll=res["ll"], posterior=res["posterior"], best=res["best"], qual=res["qual"])


def _same(a, b, tag):
    for k in ("ll", "posterior", "best", "qual"):
        assert a[k].tobytes() == b[k].tobytes(), (tag, k)


@pytest.mark.parametrize("mname,engine,opts", PS.SWEEP,
                         ids=[f"{m}-engine{e}" + "".join(f"-{k}{v}" for k, v in o if k != "ovf_deep") for m, e, o in PS.SWEEP])
def test_every_cell_against_the_reference(mods, mname, engine, opts):
    """One ctx per (matrix, engine, options); K = 2 from the matrix' exclusion sets with reference_scales, K = 3 and K = 16 from a
    seeded draw with 5 % unlabelled, each with all loci and under a mask; forced tile_sb 2 / 4: the same bits."""
    g, G = PS._load(mods, mname, engine, opts)
    L, N, coo, _ = pr.matrix(mname)
    worst = {}
    for K, which in cr.case_names(mname):
        for masked in (False, True):
            ref = cr.case(mname, K, which, masked)
            tag = f"{mname} engine {engine} {dict(opts).get('t2_tiles', '')} K {K} {which} {'masked' if masked else 'all loci'}"
            got = _got(g.class_posteriors(ref["labels"], K, ref["scale"], ref["log_prior"], ref["mask"]))
            res = cr.compare(ref, got, G)
            print(f"  {tag}: worst observed / bound ll {res['ll'][0]:.3f}, posterior {res['posterior'][0]:.3f}; best and qual "
                  f"compared in {res['best'][0]} of {N} cells, qual on an integer edge in {res['qual_edges']}")
            assert cr.ok(res), f"{tag}: " + cr.describe(ref, got, res)
            for k in ("ll", "posterior"):
                worst[k] = max(worst.get(k, 0.0), res[k][0])
            if engine == 2:
                for sb in (2, 4, 0):
                    g.set_option("tile_sb", sb)
                    _same(got, _got(g.class_posteriors(ref["labels"], K, ref["scale"], ref["log_prior"], ref["mask"])), f"{tag}: tile_sb {sb}")
            if K == 2 and not masked:  # the reference's two-class posterior phase on the same ctx
                g.set_excluded(ref["labels"] == 0)
                two = g.posteriors()
                assert two["ll_minority"].tobytes() == got["ll"][0].tobytes(), tag
                assert two["ll_majority"].tobytes() == got["ll"][1].tobytes(), tag
                sc, lp = mods["cl"].reference_scales(int((ref["labels"] == 0).sum()), N)
                assert list(sc) == ref["scale"] and list(lp) == ref["log_prior"]
                a, b = g.class_alpha_betas(ref["labels"], 2, sc)
                for k in (0, 1):
                    pa, pb = g.posterior_alpha_betas(k)
                    assert np.array_equal(a[k], pa) and np.array_equal(b[k], pb), (tag, k)
    print(f"  {mname} engine {engine} {dict(opts)}: G = {G}; worst over the cases " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    g.close()


@ENGINES
def test_dead_class(mods, engine):
    L, N, coo, _ = pr.matrix("tier2")
    g = _make(mods, engine, L, N, coo)
    lab = np.where(np.arange(N) % 5 == 0, 0, 2).astype(np.uint8)
    lab[3::11] = cr.UNLABELLED
    ref = cr.reference(L, N, coo, lab, 3)
    got = _got(g.class_posteriors(lab, 3))
    assert np.isneginf(got["ll"][1]).all() and (got["posterior"][1] == 0).all() and not (got["best"] == 1).any()
    res = cr.compare(ref, got, cr.g_any(L))
    assert cr.ok(res), cr.describe(ref, got, res)
    r = g.refine_classes(lab, 3, max_iter=3)
    assert r["summary"].class_cells[1] == 0 and not (r["labels"] == 1).any()
    with pytest.raises(mods["ffi"].CellectorError, match="every cell is unlabelled"):
        g.class_posteriors(np.full(N, cr.UNLABELLED, np.uint8), 3)
    g.close()


# ---- refine --------------------------------------------------------------------------------------------------------------------
_twins = {}


def _twin(mods, which, max_iter, min_loci=1, class_delta=True):
    key = (which, max_iter, min_loci, class_delta)
    if key not in _twins:
        L, N, coo, _ = cr.mixture()
        start, K = cr.refine_start(which)
        _twins[key] = mods["cl"].refine(L, coo, start, K, cr.ll_fn_80bit(N, coo), max_iter=max_iter, min_loci=min_loci,
                                        class_delta=class_delta)
    return _twins[key]


def _summary(s):
    return dict(iterations=s.iterations, converged=s.converged, n_moved_last=s.n_moved_last, n_moved_total=s.n_moved_total,
                n_recounts=s.n_recounts, class_cells=list(s.class_cells))


def _twin_summary(tw):
    return dict(tw["summary"], class_cells=[int(x) for x in tw["summary"]["class_cells"]])


@ENGINES
@pytest.mark.parametrize("which", cr.REFINE_STARTS)
def test_refine_follows_the_twin(mods, engine, which):
    """The mixture of three genotypes (900 cells x 600 loci and six one-entry cells) from the truth with 15 % of the labels
    reassigned and 5 % unlabelled; "empties": a fourth class of three cells that dies on the way.  The twin's final labels equal
    the planted truth in every labelled cell (share 1.0000, measured on the CPU)."""
    L, N, coo, _ = cr.mixture()
    start, K = cr.refine_start(which)
    g = _make(mods, engine, L, N, coo)
    assert g.dims().loci_used == L
    full = _twin(mods, which, 20)
    n_steps = full["summary"]["iterations"]
    for max_iter in list(range(0, n_steps + 1)) + [20]:
        tw = _twin(mods, which, max_iter)
        for delta in (1, 0):
            g.set_option("class_delta", delta)
            r = g.refine_classes(start, K, max_iter=max_iter)
            want = _twin_summary(_twin(mods, which, max_iter, class_delta=bool(delta)))
            assert _summary(r["summary"]) == want, (which, engine, max_iter, delta, _summary(r["summary"]), want)
            assert np.array_equal(r["labels"], tw["labels"]), (which, engine, max_iter, delta)
            if delta:
                first = r
            else:  # a recount every step: the same integers, so the same bits everywhere
                assert r["ll"].tobytes() == first["ll"].tobytes() and r["posterior"].tobytes() == first["posterior"].tobytes()
                assert np.array_equal(r["qual"], first["qual"]) and np.array_equal(r["labels"], first["labels"])
                if max_iter >= 2:
                    assert r["summary"].n_recounts == r["summary"].iterations > first["summary"].n_recounts == 1
        # the last step's outputs: those of class_posteriors on the labels that step started from
        last = g.class_posteriors(tw["steps"][-1]["labels_in"], K)
        assert first["ll"].tobytes() == last["ll"].tobytes() and first["posterior"].tobytes() == last["posterior"].tobytes()
        assert np.array_equal(first["qual"], last["qual"])
    if which == "empties":
        assert full["summary"]["class_cells"][3] == 0
    # min_loci 2: the one-entry cells keep their labels; the twin agrees
    g.set_option("class_delta", 1)
    r2, t2 = g.refine_classes(start, K, max_iter=20, min_loci=2), _twin(mods, which, 20, min_loci=2)
    assert np.array_equal(r2["labels"], t2["labels"]) and np.array_equal(r2["labels"][cr.MIX_N:], start[cr.MIX_N:])
    assert _summary(r2["summary"]) == _twin_summary(t2)
    assert np.array_equal(start, cr.refine_start(which)[0])  # the caller's array is not written
    g.close()


# ---- the EM state stays ------------------------------------------------------------------------------------------------------------
@ENGINES
@pytest.mark.parametrize("mname", ["tier2", "row-lengths"])
def test_class_calls_leave_the_loop_alone(mods, mname, engine):
    opts = PS.DEEP[8] if (engine == 2 and mname == "tier2") else ()
    L, N, coo, _ = pr.matrix(mname)
    x, y = _make(mods, engine, L, N, coo, opts), _make(mods, engine, L, N, coo, opts)
    want = x.run(5.0, 40)
    assert not want[-1].any_change
    want.append(x.em_iteration(5.0))  # (one more at the fixed point: at least two iterations in all)
    lab, _, _ = cr.case_labels(mname, 3, "draw")
    got = []
    for it in range(len(want)):
        got.append(y.em_iteration(5.0))
        if it == 1:
            state = (y.excluded(), y.loci_mask())
            y.class_posteriors(lab, 3, mask=cr.case_mask(mname))
            y.refine_classes(lab, 3, max_iter=2)
            y.class_tallies(lab, 3)
            assert np.array_equal(y.excluded(), state[0]) and np.array_equal(y.loci_mask(), state[1])
    assert [bytes(s) for s in got] == [bytes(s) for s in want], (mname, engine)
    assert np.array_equal(x.excluded(), y.excluded()) and np.array_equal(x.loci_mask(), y.loci_mask())
    for k, v in x.cell_outputs().items():
        assert v.tobytes() == y.cell_outputs()[k].tobytes(), k
    x.close(); y.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(mods):
    ffi = mods["ffi"]
    L, N, coo = _row_matrix(65, seed=65)
    lab = (np.arange(N) % 3).astype(np.uint8)

    def refused(fn, match):
        with pytest.raises(ffi.CellectorError, match=match) as e:
            fn()
        assert e.value.status == 1

    def every_call(g, match, n=N):
        l = lab[:n]
        refused(lambda: g.class_tallies(l, 3), match)
        refused(lambda: g.class_alpha_betas(l, 3), match)
        refused(lambda: g.class_posteriors(l, 3), match)
        refused(lambda: g.refine_classes(l, 3), match)

    g = _make(mods, 2, L, N, coo)
    for K in (0, 17):
        refused(lambda: g.class_tallies(np.zeros(N, np.uint8), K), "1..16 are supported")
        refused(lambda: g.refine_classes(np.zeros(N, np.uint8), K), "1..16 are supported")
    bad = lab.copy()
    bad[5], bad[9] = 3, 200
    refused(lambda: g.class_tallies(bad, 3), "cell 5 has label 3")
    refused(lambda: g.class_posteriors(bad, 3), "cell 5 has label 3")
    refused(lambda: g.refine_classes(bad, 3), "cell 5 has label 3")
    for s in ([1.0, -0.5, 1.0], [1.0, np.inf, 1.0], [np.nan, 1.0, 1.0]):
        refused(lambda: g.class_alpha_betas(lab, 3, s), "scale")
        refused(lambda: g.class_posteriors(lab, 3, s), "scale")
        refused(lambda: g.refine_classes(lab, 3, s), "scale")
    refused(lambda: g.class_posteriors(lab, 3, log_prior=[0.0, np.nan, 0.0]), r"log_prior\[1\] is NaN")
    refused(lambda: g.refine_classes(lab, 3, log_prior=[0.0, np.nan, 0.0]), r"log_prior\[1\] is NaN")
    refused(lambda: g.refine_classes(lab, 3, min_loci=0), "min_loci")
    lib = ffi.load_library()
    assert lib.cellector_class_tallies(g.h, None, 3, None, None, None) == 1 and b"null labels" in lib.cellector_last_error(g.h)
    assert lib.cellector_refine_classes(g.h, None, 3, None, None, None, 1, 1, None, None, None, None) == 1
    refused(lambda: g.set_option("class_delta", 2), "class_delta")
    g.em_begin()
    every_call(g, "in flight")
    g.em_threshold(5.0)
    every_call(g, "in flight")
    g.em_finish()
    # usable afterwards: a -inf prior is legal (that class wins no cell), and the refused label array was not written
    out = g.class_posteriors(lab, 3, log_prior=[0.0, -np.inf, 0.0])
    assert (out["posterior"][1] == 0).all() and np.isfinite(out["posterior"]).all() and bad[5] == 3
    assert g.refine_classes(lab, 3, max_iter=2)["summary"].iterations >= 1
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
    os.environ["CELLECTOR_COMM_SELFTEST"] = "1"
    try:
        g = mods["Cellector"](0)
        g.comm_init_rank(ffi.comm_unique_id(), 1, 0)
    finally:
        os.environ.pop("CELLECTOR_COMM_SELFTEST", None)
    g.load_coo(L, N, *S._u32(coo), 0, 0)
    every_call(g, "without a communicator")
    assert g.em_iteration(5.0) is not None
    g.close()
