"""GPU: engine 2 keeps the exclusion set's per-(locus, code) counts across iterations and updates them from the set's change
(option tally_delta, default 1).  Counts are integers, so every output must equal, to the bit, what a recount every
iteration (tally_delta 0) gives, at every iteration, and agree with the oracle."""
import numpy as np
import pytest

import test_gpu_parity as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods(oracle_lib, hip_lib_path):
    from cellector_amd import Cellector, synth
    return dict(Cellector=Cellector, synth=synth, ob=oracle_lib)


def _summary(s):
    return (s.any_change, s.n_new_excluded, s.n_rescued, s.n_excluded, s.n_loci_filtered, s.n_near_threshold,
            s.median, s.iqr, s.threshold)


def _assert_same(a, b):
    """Both contexts finished the same iteration: every output equal to the bit."""
    for x, y in ((a.cell_outputs(), b.cell_outputs()), (a.locus_outputs(), b.locus_outputs())):
        assert x.keys() == y.keys()
        for k in x:
            assert np.array_equal(x[k], y[k]), k
    assert np.array_equal(a.excluded(), b.excluded())
    assert np.array_equal(a.loci_mask(), b.loci_mask())


def _ctx(mods, delta, opts=(), engine=None):
    g = mods["Cellector"](0)
    if engine is not None:
        g.set_option("engine", engine)
    g.set_option("tally_delta", delta)
    for k, v in opts:
        g.set_option(k, v)
    return g


def _run_ab(mods, L, N, coo, iqr, opts=(), max_iter=30):
    """tally_delta 1 against 0 and the oracle, iteration by iteration until convergence; returns the summaries."""
    g1, g0 = _ctx(mods, 1, opts), _ctx(mods, 0, opts)
    g1.load_coo(L, N, *coo)
    g0.load_coo(L, N, *coo)
    o = mods["ob"].Oracle.from_coo(L, N, *coo)
    out = []
    for _ in range(max_iter):
        s1, s0, so = g1.em_iteration(iqr), g0.em_iteration(iqr), o.em_iteration(iqr)
        assert _summary(s1) == _summary(s0)
        _assert_same(g1, g0)
        T._check_iteration(g1, o, s1, so)
        out.append(s1)
        if not so.any_change:
            break
    g1.close(); g0.close(); o.close()
    return out


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_shallow_with_tier2_and_rescues(mods, mode):
    """Vartrix-like totals (some 5..8: tier 2).  A threshold half an IQR below the median keeps cells moving both ways for a
    few iterations: newly excluded and rescued cells in one change."""
    L, N = 1500, 2000
    coo = mods["synth"].generate_coo(L, N, 0.03, seed=33, minority_fraction=0.2)
    tot = coo[2] + coo[3]
    assert ((tot >= 5) & (tot <= 8)).any()
    s = _run_ab(mods, L, N, coo, 0.5, (("locus_mode", mode),))
    assert sum(x.n_rescued for x in s) > 0 and len(s) >= 3


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_deep_coverage(mods, mode):
    """Totals 1 + Geometric(0.4) (synth_continue_pct 60): many tier-2 and overflow entries; cells rescued in iteration 2."""
    L, N = 1200, 2000
    coo = mods["synth"].generate_coo(L, N, 0.05, seed=8, minority_fraction=0.1, continue_pct=60)
    s = _run_ab(mods, L, N, coo, 0.5, (("locus_mode", mode),))
    assert sum(x.n_rescued for x in s) > 0


def test_locus_filter_hits(mods):
    """A locus fixed for opposite alleles in the two populations at depth 60 is masked by the -80 filter (main.rs:444-447):
    the kept counts go on over all loci, masked or not."""
    L, N = 400, 900
    coo = mods["synth"].generate_coo(L, N, 0.25, seed=9, minority_fraction=0.1)
    cls = mods["synth"].cell_classes(N, seed=9, minority_fraction=0.1)
    lo, ce, al, re = coo
    lo = np.concatenate([lo, np.full(N, L, np.uint32)])
    ce = np.concatenate([ce, np.arange(N, dtype=np.uint32)])
    al = np.concatenate([al, np.where(cls == 1, 60, 0).astype(np.uint32)])
    re = np.concatenate([re, np.where(cls == 1, 0, 60).astype(np.uint32)])
    s = _run_ab(mods, L + 1, N, (lo, ce, al, re), 1.0)
    assert sum(x.n_loci_filtered for x in s) > 0


def test_invalidation_reload_shard_and_engine_switch(mods):
    """The kept counts belong to one matrix, one shard and engine 2's own iterations: a reload, a shard ctx and an engine
    switch 2 -> 1 -> 2 between iterations must give what a ctx that recounts every iteration gives."""
    synth = mods["synth"]
    La, Na, Lb, Nb = 1300, 1700, 900, 2000
    coo_a = synth.generate_coo(La, Na, 0.03, seed=6, minority_fraction=0.2)
    coo_b = synth.generate_coo(Lb, Nb, 0.04, seed=5, minority_fraction=0.1)
    # reload: a ctx that ran iterations on A, then B (more cells than A), against a fresh ctx on B
    g = _ctx(mods, 1)
    g.load_coo(La, Na, *coo_a)
    for _ in range(2):
        g.em_iteration(0.5)
    g.load_coo(Lb, Nb, *coo_b)
    f = _ctx(mods, 0)
    f.load_coo(Lb, Nb, *coo_b)
    o = mods["ob"].Oracle.from_coo(Lb, Nb, *coo_b)
    for _ in range(30):
        sg, sf, so = g.em_iteration(0.5), f.em_iteration(0.5), o.em_iteration(0.5)
        assert _summary(sg) == _summary(sf)
        _assert_same(g, f)
        T._check_iteration(g, o, sg, so)
        if not so.any_change:
            break
    g.close(); f.close(); o.close()
    # a shard of the cells (cellector_set_shard): no exchanges, the shard's own exclusion set
    pair = []
    for delta in (1, 0):
        h = _ctx(mods, delta)
        h.set_shard(300, 1400)
        h.load_coo(La, Na, *coo_a)
        pair.append(h)
    for _ in range(6):
        s1, s0 = pair[0].em_iteration(0.5), pair[1].em_iteration(0.5)
        assert _summary(s1) == _summary(s0)
        _assert_same(*pair)
    for h in pair:
        h.close()
    # engine 2 -> 1 -> 2 between iterations (ingest under engine 1: it keeps the by-locus CSC engine 1 streams)
    pair = []
    for delta in (1, 0):
        h = _ctx(mods, delta, engine=1)
        h.load_coo(La, Na, *coo_a)
        h.set_option("engine", 2)
        pair.append(h)
    o = mods["ob"].Oracle.from_coo(La, Na, *coo_a)
    for it, engine in enumerate((2, 1, 2, 2, 1, 1, 2, 2)):
        for h in pair:
            h.set_option("engine", engine)
        s1, s0, so = pair[0].em_iteration(0.5), pair[1].em_iteration(0.5), o.em_iteration(0.5)
        assert _summary(s1) == _summary(s0), it
        _assert_same(*pair)
        T._check_iteration(pair[0], o, s1, so)
    for h in pair:
        h.close()
    o.close()


@pytest.mark.parametrize("devices", [[0, 0, 0]], ids=["3shards"])
def test_logical_shards_match_recount(mods, devices):
    """A multi-shard ctx (logical shards on one GPU): every shard keeps its own counts; bit for bit against tally_delta 0."""
    L, N = 1500, 2001
    coo = mods["synth"].generate_coo(L, N, 0.03, seed=33, minority_fraction=0.2)
    pair = []
    for delta in (1, 0):
        m = mods["Cellector"](devices=devices)
        m.set_option("bank_order", 0)
        m.set_option("tally_delta", delta)
        m.load_coo(L, N, *coo)
        pair.append(m)
    o = mods["ob"].Oracle.from_coo(L, N, *coo)
    for _ in range(30):
        s1, s0, so = pair[0].em_iteration(0.5), pair[1].em_iteration(0.5), o.em_iteration(0.5)
        assert _summary(s1) == _summary(s0)
        _assert_same(*pair)
        T._check_iteration(pair[0], o, s1, so)
        if not so.any_change:
            break
    for m in pair:
        m.close()
    o.close()


def test_option_values(mods):
    from cellector_amd import ffi
    g = mods["Cellector"](0)
    g.set_option("tally_delta", 0)
    g.set_option("tally_delta", 1)
    with pytest.raises(ffi.CellectorError):
        g.set_option("tally_delta", 2)
    g.close()
