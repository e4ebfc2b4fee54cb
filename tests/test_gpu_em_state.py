"""GPU: placing and resetting the EM state — cellector_set_excluded, cellector_set_loci_mask, cellector_em_reset — against
the CPU oracle (Oracle.set_excluded), against numpy's exact integers and against ctxs that reached the same state by
iterating.

Tolerances are the project's own: 1e-7 abs on log-likelihood sums, 1e-6 on posteriors, 1e-9 on median / iqr /
threshold and on normalised LLs, integers and sets exact.  Every iteration that is compared with the oracle asserts
n_near_threshold == 0, so a flipped cell can never hide behind a tolerance.

Inputs A and B (synthetic, minority fraction 0.08) converge from the empty set in two iterations to 70 / 190 excluded
cells with no locus filtered.  The starts used here give non-trivial first iterations on the oracle: from
rng(1).random(N) < 0.1 it reports 64 new / 68 rescued (A) and 168 / 167 (B); from every second cell of the converged set
35 / 95 new and none rescued; the tests assert those oracle figures so that the starts stay what they were chosen for.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LL_ATOL = 1e-7
POST_ATOL = 1e-6
CASES = {"A": (1500, 800, 0.1, 11), "B": (4000, 2000, 0.03, 4)}
FIRST_ITERATION = {("A", "random"): (64, 68), ("B", "random"): (168, 167), ("A", "half"): (35, 0), ("B", "half"): (95, 0)}


@pytest.fixture(scope="module")
def env(oracle_lib, hip_lib_path):
    from cellector_amd import Cellector, ffi, synth
    return dict(Cellector=Cellector, ffi=ffi, synth=synth, ob=oracle_lib)


@pytest.fixture(scope="module", params=[2, 1], ids=["tiled", "csr"])
def engine(request):
    return request.param


def _make(env, engine, devices=None, **options):
    g = env["Cellector"](devices=devices) if devices else env["Cellector"](0)
    g.set_option("engine", engine)
    for k, v in options.items():
        g.set_option(k, v)
    return g


_coo_cache, _conv_cache = {}, {}


def _coo(env, case):
    if case not in _coo_cache:
        L, N, d, seed = CASES[case]
        _coo_cache[case] = env["synth"].generate_coo(L, N, d, seed=seed, minority_fraction=0.08)
    return _coo_cache[case]


def _converged(env, case):
    """the plain oracle run's final set"""
    if case not in _conv_cache:
        L, N = CASES[case][:2]
        o = env["ob"].Oracle.from_coo(L, N, *_coo(env, case))
        sums = o.run(5.0, 30)
        assert len(sums) == 2 and not sums[-1].any_change and (o.loci_mask() != 0).all()
        _conv_cache[case] = o.excluded().copy()
        assert int(_conv_cache[case].sum()) == {"A": 70, "B": 190}[case]
        o.close()
    return _conv_cache[case]


def _start(env, case, start):
    N = CASES[case][1]
    if start == "random":
        return (np.random.default_rng(1).random(N) < 0.1).astype(np.uint8)
    f = np.zeros(N, np.uint8)
    f[np.nonzero(_converged(env, case))[0][::2]] = 1
    return f


def _summary_matches(sg, so, o, exact=False):
    assert sg.n_near_threshold == 0
    assert (sg.any_change, sg.n_new_excluded, sg.n_rescued) == (so.any_change, so.n_new_excluded, so.n_rescued)
    assert sg.n_excluded == int(o.excluded().sum())
    assert sg.n_loci_filtered == so.n_loci_filtered
    if exact:
        assert (sg.median, sg.iqr, sg.threshold) == (so.median, so.iqr, so.threshold)
    else:
        np.testing.assert_allclose([sg.median, sg.iqr, sg.threshold], [so.median, so.iqr, so.threshold], rtol=0, atol=1e-9)


def _iterate_both(g, o, first=None, exact=False, iqr=5.0, max_iter=30):
    """both to convergence; every iteration's counts, set, order statistics and integer locus columns compared"""
    for it in range(max_iter):
        sg, so = g.em_iteration(iqr), o.em_iteration(iqr)
        if it == 0 and first is not None:
            assert (so.n_new_excluded, so.n_rescued) == first
        _summary_matches(sg, so, o, exact)
        assert np.array_equal(g.excluded(), o.excluded())
        assert np.array_equal(g.loci_mask(), o.loci_mask())
        lg, lo_ = g.locus_outputs(), o.locus_outputs()
        for k in ("cells_min", "cells_maj", "alt_min", "ref_min", "alt_maj", "ref_maj"):
            assert np.array_equal(lg[k], lo_[k]), (it, k)
        cg, co = g.cell_outputs(), o.cell_outputs()
        assert np.array_equal(cg["loci_used"], co["loci_used"])
        np.testing.assert_allclose(cg["ll"], co["ll"], rtol=0, atol=LL_ATOL)
        np.testing.assert_allclose(cg["normalized"], co["normalized"], rtol=0, atol=1e-9)
        if not so.any_change:
            return it + 1
    raise AssertionError("no convergence")


# ---- 1. placement equals the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", ["random", "half"])
@pytest.mark.parametrize("case", ["A", "B"])
def test_placement_equals_the_oracle(env, engine, case, start):
    L, N = CASES[case][:2]
    coo = _coo(env, case)
    flags = _start(env, case, start)
    g = _make(env, engine)
    g.load_coo(L, N, *coo)
    o = env["ob"].Oracle.from_coo(L, N, *coo)
    g.set_excluded(flags)
    o.set_excluded(flags)
    assert np.array_equal(g.excluded(), flags)
    ag, bg = g.alpha_betas()
    ao, bo = o.alpha_betas()
    assert np.array_equal(ag, ao) and np.array_equal(bg, bo)  # integers in f64
    tg, to = g.final_allele_tallies(), env["ob"].final_tallies_coo(L, *coo, flags)
    for k in to:
        assert np.array_equal(tg[k], to[k]), k
    # posteriors and labels of the placed partition with no iteration run at all
    po = o.posteriors()
    pa_o, aa_o, _ = o.assignments(po["posterior"], po["doublet_posterior"], 0.999, 30)
    for res in (g.posteriors(), g.assign(0.999, 30)):
        for k in ("ll_majority", "ll_minority"):
            np.testing.assert_allclose(res[k], po[k], rtol=0, atol=LL_ATOL)
        np.testing.assert_allclose(res["posterior"], po["posterior"], rtol=0, atol=POST_ATOL)
        np.testing.assert_allclose(res["doublet_posterior"], po["doublet_posterior"], rtol=0, atol=POST_ATOL)
    assert np.array_equal(res["posterior_assignment"], pa_o) and np.array_equal(res["anomaly_assignment"], aa_o)
    n_it = _iterate_both(g, o, first=FIRST_ITERATION[(case, start)])
    assert n_it >= 2 and np.array_equal(g.excluded(), _converged(env, case))
    g.close(); o.close()


# ---- 2. exact tallies at the edges, against numpy -------------------------------------------------------------------------
def _check_tallies(g, L, coo, flags, tag):
    """alt_min / ref_min of the placed set read through alpha_betas() (alpha = S_alt + 1 - alt_min) and final_allele_tallies()"""
    lo, ce, al, re = (np.asarray(x, np.int64) for x in coo)
    m = flags[ce] != 0
    want = {}
    for side, sel in (("min", m), ("maj", ~m)):
        for name, w in (("alt", al), ("ref", re)):
            acc = np.zeros(L, np.int64)
            np.add.at(acc, lo[sel], w[sel])  # (integer accumulation: bincount's float weights stop being exact at 2^53)
            want[f"{name}_{side}"] = acc.astype(np.uint64)
    assert g.dims().loci_used == L
    counts = g.locus_counts()  # [:, 0] sum ref, [:, 1] sum alt
    alpha, beta = g.alpha_betas()
    assert np.array_equal(counts[:, 1] + 1.0 - alpha, want["alt_min"].astype(np.float64)), tag
    assert np.array_equal(counts[:, 0] + 1.0 - beta, want["ref_min"].astype(np.float64)), tag
    t = g.final_allele_tallies()
    for k in want:
        assert np.array_equal(t[k], want[k]), (tag, k)
    assert np.array_equal(g.excluded(), flags)


def test_exact_tallies_for_any_set_size(env, engine):
    L, N = CASES["A"][:2]
    coo = _coo(env, "A")
    g = _make(env, engine)
    g.load_coo(L, N, *coo, 0, 0)
    rng = np.random.default_rng(3)
    for n in (0, 1, N // 10, int(0.6 * N), N, 7):  # (down again at the end: nothing is left of the larger set)
        flags = np.zeros(N, np.uint8)
        flags[rng.choice(N, n, replace=False)] = 1
        g.set_excluded(flags)
        _check_tallies(g, L, coo, flags, f"{n} cells")
    g.close()


def test_exact_tallies_beyond_32_bits(env, engine):
    """70 000 cells with one entry of 65535 alt reads each at locus 3: 4 587 450 000 reads, more than 2^32, all placed."""
    N, L = 70_000, 16
    rng = np.random.default_rng(2)
    ce = np.concatenate([np.arange(N), np.arange(N)])
    lo = np.concatenate([np.full(N, 3), rng.integers(0, L, N)])
    al = np.concatenate([np.full(N, 65535), rng.integers(0, 2, N)])
    re = np.concatenate([np.zeros(N, np.int64), np.ones(N, np.int64)])
    re[N:] -= al[N:]
    coo = tuple(x.astype(np.uint32) for x in (lo, ce, al, re))
    g = _make(env, engine)
    g.load_coo(L, N, *coo, 0, 0)
    for flags in (np.ones(N, np.uint8), (rng.random(N) < 0.97).astype(np.uint8)):
        assert int(flags.sum()) * 65535 > 2**32
        g.set_excluded(flags)
        _check_tallies(g, L, coo, flags, "wide sums")
    g.close()


def test_exact_tallies_with_a_pair_listed_70_times(env, engine):
    N, L, repeats = 3000, 500, 70
    rng = np.random.default_rng(70)
    ce = np.repeat(np.arange(N), repeats + 4)
    lo = np.concatenate([np.zeros((N, repeats), np.int64), rng.integers(1, L, (N, 4))], axis=1).ravel()
    al = np.concatenate([np.ones((N, repeats), np.int64), rng.integers(0, 2, (N, 4))], axis=1).ravel()
    re = np.where(lo == 0, 0, 1 - al)
    coo = tuple(x.astype(np.uint32) for x in (lo, ce, al, re))
    g = _make(env, engine)
    g.load_coo(L, N, *coo, 0, 0)
    flags = (rng.random(N) < 0.4).astype(np.uint8)
    g.set_excluded(flags)
    _check_tallies(g, L, coo, flags, "70 lines per pair")
    assert g.locus_counts()[0, 1] + 1.0 - g.alpha_betas()[0][0] == 70.0 * flags.sum()
    g.close()


# ---- 3. restore equals continue, bit for bit ------------------------------------------------------------------------------
def _filter_coo(env):
    """the construction of test_gpu_parity.test_locus_filter_triggers: one deep locus the minority is fixed at the other allele for"""
    L, N = 400, 600
    lo, ce, al, re = env["synth"].generate_coo(L, N, 0.25, seed=9, minority_fraction=0.1)
    cls = env["synth"].cell_classes(N, seed=9, minority_fraction=0.1)
    lo = np.concatenate([lo, np.full(N, L, np.uint32)]); ce = np.concatenate([ce, np.arange(N, dtype=np.uint32)])
    al = np.concatenate([al, np.where(cls == 1, 60, 0).astype(np.uint32)])
    re = np.concatenate([re, np.where(cls == 1, 0, 60).astype(np.uint32)])
    return L + 1, N, (lo, ce, al, re)


def _bit_equal_iteration(x, y, sx, sy, tag):
    assert bytes(sx) == bytes(sy), tag
    cx, cy = x.cell_outputs(), y.cell_outputs()
    for k in cx:
        assert cx[k].tobytes() == cy[k].tobytes(), (tag, k)
    lx, ly = x.locus_outputs(), y.locus_outputs()
    for k in lx:
        assert lx[k].tobytes() == ly[k].tobytes(), (tag, k)
    assert np.array_equal(x.excluded(), y.excluded()) and np.array_equal(x.loci_mask(), y.loci_mask())


def _restore_equals_continue(env, engine, devices, **options):
    L, N, coo = _filter_coo(env)
    start = (np.random.default_rng(1).random(N) < 0.1).astype(np.uint8)
    x = _make(env, engine, devices, **options)
    x.load_coo(L, N, *coo)
    x.set_excluded(start)
    masked = 0
    for _ in range(4):  # (until the filter has masked the deep locus: the restored state must carry a mask)
        x.em_iteration(5.0)
        masked = int((x.loci_mask() == 0).sum())
        if masked:
            break
    assert masked >= 1
    y = _make(env, engine, devices, **options)
    y.load_coo(L, N, *coo)
    y.set_loci_mask(x.loci_mask())
    y.set_excluded(x.excluded())
    assert np.array_equal(y.excluded(), x.excluded()) and np.array_equal(y.loci_mask(), x.loci_mask())
    ax, ay = x.alpha_betas(), y.alpha_betas()
    assert ax[0].tobytes() == ay[0].tobytes() and ax[1].tobytes() == ay[1].tobytes()
    for it in range(3):
        sx, sy = x.em_iteration(5.0), y.em_iteration(5.0)
        _bit_equal_iteration(x, y, sx, sy, f"iteration {it}")
    px, py = x.posteriors(), y.posteriors()
    for k in px:
        assert px[k].tobytes() == py[k].tobytes(), k
    x.close(); y.close()


@pytest.mark.parametrize("locus_mode", [0, 1, 2])
@pytest.mark.parametrize("tally_delta", [0, 1])
def test_restore_equals_continue(env, engine, tally_delta, locus_mode):
    _restore_equals_continue(env, engine, None, tally_delta=tally_delta, locus_mode=locus_mode)


def test_restore_equals_continue_sharded(env, engine):
    _restore_equals_continue(env, engine, [0, 0])


# ---- 4. reset ---------------------------------------------------------------------------------------------------------------
def _run_record(g, iqr=5.0):
    out = []
    for _ in range(30):
        s = g.em_iteration(iqr)
        out.append((bytes(s), {k: v.tobytes() for k, v in g.cell_outputs().items()},
                    {k: v.tobytes() for k, v in g.locus_outputs().items()}, g.excluded().tobytes(), g.loci_mask().tobytes()))
        if not s.any_change:
            return out
    raise AssertionError("no convergence")


@pytest.mark.parametrize("devices", [None, [0, 0, 0]], ids=["single", "three-shards"])
def test_reset_equals_a_fresh_ctx(env, engine, devices):
    L, N, coo = _filter_coo(env)  # (a run that also masks a locus: the reset has a mask and masked counts to clear)
    g = _make(env, engine, devices)
    g.load_coo(L, N, *coo)
    first = _run_record(g)
    assert any(np.frombuffer(r[4], np.uint8).min() == 0 for r in first)
    g.em_reset()
    assert not g.excluded().any() and g.loci_mask().all()
    a, b = g.alpha_betas()
    counts = g.locus_counts()
    assert np.array_equal(a, counts[:, 1] + 1.0) and np.array_equal(b, counts[:, 0] + 1.0)
    with pytest.raises(env["ffi"].CellectorError):
        g.locus_outputs()  # no finished iteration any more
    again = _run_record(g)
    fresh = _make(env, engine, devices)
    fresh.load_coo(L, N, *coo)
    assert again == first and _run_record(fresh) == first
    # another interquartile_range_multiple on the resident matrix
    g.em_reset()
    fresh3 = _make(env, engine, devices)
    fresh3.load_coo(L, N, *coo)
    assert _run_record(g, 3.0) == _run_record(fresh3, 3.0)
    o = env["ob"].Oracle.from_coo(L, N, *coo)
    o.run(3.0, 30)
    assert np.array_equal(g.excluded(), o.excluded()) and np.array_equal(g.loci_mask(), o.loci_mask())
    g.close(); fresh.close(); fresh3.close(); o.close()


# ---- 5. the caller's mask -----------------------------------------------------------------------------------------------------
def test_callers_mask_one_iteration_and_trajectory(env, engine):
    L, N = CASES["A"][:2]
    coo = _coo(env, "A")
    g = _make(env, engine)
    g.load_coo(L, N, *coo)
    o = env["ob"].Oracle.from_coo(L, N, *coo)
    Lu = g.dims().loci_used
    mask = (np.random.default_rng(5).random(Lu) < 0.8).astype(np.uint8)
    assert 0 < mask.sum() < Lu
    g.set_loci_mask(mask)
    assert np.array_equal(g.loci_mask(), mask)
    alpha, beta = o.alpha_betas()  # the empty set's
    ag, bg = g.alpha_betas()
    assert np.array_equal(ag, alpha) and np.array_equal(bg, beta)  # a masked locus still counts in alpha / beta
    ll, ell, nl = o.cell_log_likelihoods(alpha, beta, mask)
    s = g.em_iteration(5.0)
    cg = g.cell_outputs()
    assert np.array_equal(cg["loci_used"], nl)
    np.testing.assert_allclose(cg["ll"], ll, rtol=0, atol=LL_ATOL)
    np.testing.assert_allclose(cg["expected_ll"], ell, rtol=0, atol=LL_ATOL)
    # whole trajectory: an oracle whose matrix lacks the masked loci's entries sees the same per-cell values (a masked locus
    # only leaves the cell sums; the filter and the order statistics work on those)
    ids = g.locus_ids().astype(np.int64)
    masked_ids = ids[mask == 0]
    lo, ce, al, re = coo
    keep = ~np.isin(np.asarray(lo, np.int64), masked_ids)
    o2 = env["ob"].Oracle.from_coo(L, N, lo[keep], ce[keep], al[keep], re[keep])
    assert o2.loci_used == int(mask.sum())
    g.em_reset()
    g.set_loci_mask(mask)
    for it in range(30):
        sg, so = g.em_iteration(5.0), o2.em_iteration(5.0)
        assert sg.n_near_threshold == 0
        assert (sg.n_new_excluded, sg.n_rescued, sg.any_change) == (so.n_new_excluded, so.n_rescued, so.any_change)
        np.testing.assert_allclose([sg.median, sg.iqr, sg.threshold], [so.median, so.iqr, so.threshold], rtol=0, atol=1e-9)
        assert np.array_equal(g.excluded(), o2.excluded())
        np.testing.assert_allclose(g.cell_outputs()["normalized"], o2.cell_outputs()["normalized"], rtol=0, atol=1e-9)
        if not so.any_change:
            break
    assert it >= 1 and g.excluded().any()
    g.close(); o.close(); o2.close()


def test_all_zero_and_all_one_masks(env, engine):
    L, N = CASES["A"][:2]
    coo = _coo(env, "A")
    g = _make(env, engine)
    g.load_coo(L, N, *coo)
    Lu = g.dims().loci_used
    g.set_loci_mask(np.zeros(Lu, np.uint8))
    s = g.em_iteration(5.0)  # every locus masked: the pass completes
    c = g.cell_outputs()
    assert not c["normalized"].any() and not c["loci_used"].any() and not c["ll"].any()
    assert (s.n_excluded, s.n_new_excluded, s.any_change) == (0, 0, 0) and (s.median, s.threshold) == (0.0, 0.0)
    assert not g.excluded().any()
    g.set_loci_mask(np.ones(Lu, np.uint8))
    fresh = _make(env, engine)
    fresh.load_coo(L, N, *coo)
    g.em_reset()
    assert _run_record(g) == _run_record(fresh)
    g.close(); fresh.close()


def test_engines_agree_under_a_mask(env):
    L, N = CASES["B"][:2]
    coo = _coo(env, "B")
    runs = []
    for eng in (2, 1):
        g = _make(env, eng)
        g.load_coo(L, N, *coo)
        mask = (np.random.default_rng(6).random(g.dims().loci_used) < 0.8).astype(np.uint8)
        g.set_loci_mask(mask)
        g.set_excluded(_start(env, "B", "random"))
        rec = []
        for _ in range(30):
            s = g.em_iteration(5.0)
            rec.append((s, g.cell_outputs(), g.excluded()))
            if not s.any_change:
                break
        runs.append(rec)
        g.close()
    assert len(runs[0]) == len(runs[1]) >= 2
    for (s2, c2, e2), (s1, c1, e1) in zip(*runs):
        assert s2.n_near_threshold == 0 and s1.n_near_threshold == 0
        assert (s2.n_new_excluded, s2.n_rescued, s2.n_excluded) == (s1.n_new_excluded, s1.n_rescued, s1.n_excluded)
        np.testing.assert_allclose([s2.median, s2.iqr, s2.threshold], [s1.median, s1.iqr, s1.threshold], rtol=0, atol=1e-9)
        np.testing.assert_allclose(c2["normalized"], c1["normalized"], rtol=0, atol=1e-9)
        assert np.array_equal(c2["loci_used"], c1["loci_used"]) and np.array_equal(e2, e1)


# ---- 6. sharding ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", [[0, 0], [0] * 5], ids=["two", "five"])
def test_sharded_placement_equals_single(env, engine, devices):
    L, N = CASES["A"][:2]
    coo = _coo(env, "A")
    flags = _start(env, "A", "random")
    single = _make(env, engine)
    single.load_coo(L, N, *coo)
    single.set_excluded(flags)
    m = _make(env, engine, devices)
    m.load_coo(L, N, *coo)
    m.set_excluded(flags)  # one global array, global cell order
    assert np.array_equal(m.excluded(), flags)
    a1, am = single.alpha_betas(), m.alpha_betas()
    assert np.array_equal(a1[0], am[0]) and np.array_equal(a1[1], am[1])
    t1, tm = single.final_allele_tallies(), m.final_allele_tallies()
    for k in t1:
        assert np.array_equal(t1[k], tm[k]), k
    p1, pm = single.posteriors(), m.posteriors()
    np.testing.assert_allclose(pm["posterior"], p1["posterior"], rtol=0, atol=1e-9)
    for _ in range(30):
        s1, sm = single.em_iteration(5.0), m.em_iteration(5.0)
        assert (sm.any_change, sm.n_new_excluded, sm.n_rescued, sm.n_excluded, sm.n_loci_filtered, sm.n_near_threshold) == \
               (s1.any_change, s1.n_new_excluded, s1.n_rescued, s1.n_excluded, s1.n_loci_filtered, 0)
        assert np.allclose([sm.median, sm.iqr, sm.threshold], [s1.median, s1.iqr, s1.threshold], rtol=1e-12, atol=1e-12)
        assert np.array_equal(m.excluded(), single.excluded())
        if not s1.any_change:
            break
    assert np.array_equal(single.excluded(), _converged(env, "A"))
    single.close(); m.close()


def test_one_rank_communicator(env, engine):
    """cellector_comm_init_rank with one rank: the tally reduction runs as a real all-reduce on the ctx's stream"""
    L, N = CASES["A"][:2]
    coo = _coo(env, "A")
    flags = _start(env, "A", "random")
    os.environ["CELLECTOR_COMM_SELFTEST"] = "1"
    try:
        g = _make(env, engine)
        g.comm_init_rank(env["ffi"].comm_unique_id(), 1, 0)
    finally:
        os.environ.pop("CELLECTOR_COMM_SELFTEST", None)
    g.load_coo(L, N, *coo)
    o = env["ob"].Oracle.from_coo(L, N, *coo)
    g.set_excluded(flags)
    o.set_excluded(flags)
    ag, ao = g.alpha_betas(), o.alpha_betas()
    assert np.array_equal(ag[0], ao[0]) and np.array_equal(ag[1], ao[1])
    _iterate_both(g, o, first=FIRST_ITERATION[("A", "random")])
    g.em_reset()
    assert len(g.run(5.0, 30)) == 2 and np.array_equal(g.excluded(), _converged(env, "A"))
    g.close(); o.close()


def test_host_driven_shard_is_refused(env, engine):
    L, N = CASES["A"][:2]
    g = _make(env, engine)
    g.set_shard(0, N // 2)
    g.load_coo(L, N, *_coo(env, "A"))
    E = env["ffi"].CellectorError
    with pytest.raises(E, match="communicator"):
        g.set_excluded(np.zeros(N // 2, np.uint8))
    with pytest.raises(E, match="communicator"):
        g.set_loci_mask(np.ones(g.dims().loci_used, np.uint8))
    with pytest.raises(E, match="communicator"):
        g.em_reset()
    g.close()


# ---- 7. state errors ----------------------------------------------------------------------------------------------------------
def test_calls_out_of_order_are_refused(env, engine):
    L, N = CASES["A"][:2]
    coo = _coo(env, "A")
    E = env["ffi"].CellectorError
    g = _make(env, engine)
    lib, h = g._lib, g.h
    z = np.zeros(max(L, N), np.uint8)
    for st in (lib.cellector_set_excluded(h, z.ctypes.data), lib.cellector_set_loci_mask(h, z.ctypes.data), lib.cellector_em_reset(h)):
        assert st == 1  # CELLECTOR_EINVAL: nothing loaded
    assert b"no matrix" in lib.cellector_last_error(h)
    m = env["Cellector"](devices=[0, 0])
    for st in (m._lib.cellector_set_excluded(m.h, z.ctypes.data), m._lib.cellector_set_loci_mask(m.h, z.ctypes.data),
               m._lib.cellector_em_reset(m.h)):
        assert st == 1
    m.close()
    g.load_coo(L, N, *coo)
    ref = _make(env, engine)
    ref.load_coo(L, N, *coo)
    Lu = g.dims().loci_used
    g.em_begin()
    for call in (lambda: g.set_excluded(np.ones(N, np.uint8)), lambda: g.set_loci_mask(np.zeros(Lu, np.uint8)), g.em_reset):
        with pytest.raises(E, match="in flight"):
            call()
    g.em_threshold(5.0)
    with pytest.raises(E, match="in flight"):
        g.em_reset()
    s, sr = g.em_finish(), ref.em_iteration(5.0)  # the refused calls changed nothing
    _bit_equal_iteration(g, ref, s, sr, "after the refusals")
    s, sr = g.em_iteration(5.0), ref.em_iteration(5.0)
    _bit_equal_iteration(g, ref, s, sr, "second iteration")
    with pytest.raises(ValueError):
        g.set_excluded(np.zeros(N + 1, np.uint8))
    with pytest.raises(ValueError):
        g.set_loci_mask(np.zeros(Lu + 1, np.uint8))
    g.close(); ref.close()


# ---- 8. with resolve_ties ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["A", "B"])
def test_warm_start_with_resolve_ties_is_the_oracles_bits(env, engine, case):
    L, N = CASES[case][:2]
    coo = _coo(env, case)
    g = _make(env, engine, resolve_ties=1)  # before the ingest: it keeps the file-order copy
    g.load_coo(L, N, *coo)
    o = env["ob"].Oracle.from_coo(L, N, *coo)
    flags = _start(env, case, "random")
    g.set_excluded(flags)
    o.set_excluded(flags)
    _iterate_both(g, o, first=FIRST_ITERATION[(case, "random")], exact=True)
    assert g.resolution().mode == 1
    g.close(); o.close()
