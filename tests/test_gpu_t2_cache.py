"""GPU: keeping the EM pass' tier-2 lookup values across iterations must not change a bit (option t2_cache;
csrc/kernels_tiled.hip, k_t2_cell<.., CACHE> and the dirty mask k_t2_tables forms).

An entry's two looked-up values are a pure function of its locus' (alpha, beta) bits, so the caching instance keeps them per
entry and gathers again only at loci whose bits differ from those the kept values were written under.  Whatever state the store
is in — empty, partly stale, up to date — a row's lane adds the same values in the same order as the plain instance, so two
contexts that differ in t2_cache alone are compared with ==, never approx, on everything a caller can read after every step:
cell_outputs(), locus_outputs(), excluded(), loci_mask() and the iteration summary.

Shapes: 3 001 cells (46 full 64-row groups and a ragged one of 57 rows) x 400 loci at density 0.08, every locus used (min_alt =
min_ref = 0).  Entry totals: 91 % in 1..4 (the tiles), 6 % in 5..8 (tier 2), 1.5 % in 9..40 (the tier lists) and 1.5 % total 0
(alt = ref = 0).  Cell 7 has no tier-2 entry (all its totals 2) and cell 11 only tier-2 entries (all its totals 6).  9 % of the
entries lie outside the tables, more than the 3 % beyond which the ingest chooses the deep layouts (which have no lookup
kernel), so the shallow layouts are asked for with ovf_deep 0 before the ingest.  The lookups run beside the tile kernel
(overlap 1) with the helper grid forced (t2_helper 1: both grids deal their groups from the device counter) and without it
(t2_helper 0: the strided instance).  t2_fill forces what a pass does at dirty loci: 1 gathers and stores, 0 gathers without
storing; -1 leaves it to the device's rule.
"""
import numpy as np
import pytest

N_CELLS, N_LOCI, DENSITY = 3001, 400, 0.08
ROW_NONE, ROW_ONLY = 7, 11  # the cell without a tier-2 entry, the cell with nothing else


@pytest.fixture(scope="module")
def mods(hip_lib_path):
    from cellector_amd import Cellector
    return dict(Cellector=Cellector)


def _coo(n_cells=N_CELLS, seed=3):
    rng = np.random.default_rng(seed)
    pick = rng.random((N_LOCI, n_cells)) < DENSITY
    locus, cell = np.nonzero(pick)
    n = locus.size
    kind = rng.random(n)
    total = rng.integers(1, 5, n)
    total = np.where(kind < 0.06, rng.integers(5, 9, n), total)
    total = np.where((kind >= 0.06) & (kind < 0.075), rng.integers(9, 41, n), total)
    total = np.where((kind >= 0.075) & (kind < 0.09), 0, total)
    total = np.where(cell == ROW_NONE, 2, total)
    total = np.where(cell == ROW_ONLY, 6, total)
    # a minority of cells reads mostly alt where the others read mostly ref: the EM loop has something to exclude
    p_alt = np.where(cell % 17 == 0, 0.8, 0.25) * (0.5 + rng.random(N_LOCI))[locus]
    alt = rng.binomial(total, np.clip(p_alt, 0.02, 0.98))
    u32 = lambda a: np.ascontiguousarray(a, dtype=np.uint32)
    return u32(locus), u32(cell), u32(alt), u32(total - alt)


COO = _coo()


def _make(mods, cache, helper, engine=2):
    g = mods["Cellector"](0)
    g.set_option("engine", engine)
    g.set_option("ovf_deep", 0)
    g.set_option("overlap", 1)
    g.set_option("t2_helper", helper)
    g.set_option("t2_cache", cache)
    g.load_coo(N_LOCI, N_CELLS, *COO, min_alt=0, min_ref=0)
    if engine == 2:
        info = g.engine_info()
        assert info.engine == 2 and info.nnz_overflow > 0
    return g


class Pair:
    """two contexts on the same matrix, t2_cache 1 and 0: every action goes to both, every state is compared"""

    def __init__(self, mods, helper, fill=-1, engine=2):
        self.on, self.off = _make(mods, 1, helper, engine), _make(mods, 0, helper, engine)
        self.on.set_option("t2_fill", fill)
        self.steps = 0

    def both(self, fn):
        return fn(self.on), fn(self.off)

    def check(self, what, summaries=None):
        self.steps += 1
        if summaries:
            a, b = ([float(getattr(s, f)) for f, _ in s._fields_] for s in summaries)
            assert a == b, f"step {self.steps} ({what}): summaries differ: {a} / {b}"
        for name in ("cell_outputs", "locus_outputs"):
            got, want = self.both(lambda g: getattr(g, name)())
            assert list(got) == list(want)
            for k in got:
                same = (got[k] == want[k]) | ((got[k] != got[k]) & (want[k] != want[k]))  # NaN only against NaN
                assert same.all(), f"step {self.steps} ({what}): {name}()[{k}] differs in {int((~same).sum())} places"
        for name in ("excluded", "loci_mask"):
            got, want = self.both(lambda g: getattr(g, name)())
            assert (got == want).all(), f"step {self.steps} ({what}): {name}() differs"

    def iterate(self, what, n=1):
        last = None
        for _ in range(n):
            s = self.both(lambda g: g.em_iteration(5.0))
            self.check(what, s)
            last = s[0]
        return last

    def converge(self, what, limit=100):
        for _ in range(limit):
            if not self.iterate(what).any_change:
                return
        raise AssertionError(f"{what}: no fixed point within {limit} iterations")

    def close(self):
        self.both(lambda g: g.close())


@pytest.fixture(params=[1, 0], ids=["dealt", "strided"])
def pair(mods, request):
    p = Pair(mods, request.param)
    yield p
    p.close()


def _flip(p, k, seed):
    """set_excluded with k cells flipped against the current set"""
    f = p.on.excluded().copy()
    idx = np.random.default_rng(seed).choice(f.size, k, replace=False)
    f[idx] ^= 1
    p.both(lambda g: g.set_excluded(f))


@pytest.mark.gpu
def test_the_shape_has_what_the_kernel_branches_on(mods):
    locus, cell, alt, ref = COO
    tot = alt + ref
    t2 = (tot >= 5) & (tot <= 8)
    assert 0.03 < t2.mean() < 0.10 and (tot == 0).sum() > 100 and (tot > 8).sum() > 100
    assert not t2[cell == ROW_NONE].any() and (cell == ROW_NONE).sum() > 5
    assert t2[cell == ROW_ONLY].all() and (cell == ROW_ONLY).sum() > 5
    assert N_CELLS % 64 != 0


@pytest.mark.gpu
def test_option_values(mods):
    from cellector_amd.ffi import CellectorError
    g = mods["Cellector"](0)
    for key in ("t2_cache", "t2_fill"):
        for v in (-1, 0, 1):
            g.set_option(key, v)
        for v in (-2, 2):
            with pytest.raises(CellectorError, match=key):
                g.set_option(key, v)
    g.close()


@pytest.mark.gpu
def test_run_to_the_fixed_point_and_stay(pair):
    pair.converge("from the ingest")
    s = pair.iterate("at the fixed point", 2)
    assert not s.any_change
    assert pair.steps >= 4  # all-dirty passes, partly dirty ones and clean ones were all compared


@pytest.mark.gpu
def test_set_excluded_few_many_nearly_all(pair):
    pair.iterate("start", 2)
    for k, seed in ((1, 1), (5, 2), (N_CELLS - 1, 3)):  # few dirty loci, many, nearly all
        _flip(pair, k, seed)
        pair.iterate(f"after {k} cells flipped", 2)


@pytest.mark.gpu
def test_loci_mask_on_and_off(pair):
    pair.iterate("start", 2)
    locus, _, alt, ref = COO
    t2_loci = np.unique(locus[(alt + ref >= 5) & (alt + ref <= 8)])
    assert t2_loci.size > 50
    used = np.ones(N_LOCI, np.uint8)
    used[t2_loci[::3]] = 0
    pair.both(lambda g: g.set_loci_mask(used))
    pair.iterate("loci masked", 2)
    used[t2_loci[::6]] = 1  # half of them back
    pair.both(lambda g: g.set_loci_mask(used))
    pair.iterate("some unmasked", 2)
    pair.both(lambda g: g.set_loci_mask(np.ones(N_LOCI, np.uint8)))
    pair.iterate("all unmasked", 2)


@pytest.mark.gpu
def test_em_reset_and_a_posterior_phase_between_iterations(pair):
    pair.iterate("start", 3)
    pair.both(lambda g: g.em_reset())
    pair.iterate("after em_reset", 2)
    post = pair.both(lambda g: g.posteriors())
    for k in post[0]:
        assert np.array_equal(post[0][k], post[1][k], equal_nan=True), k
    pair.iterate("after a posterior phase", 2)


@pytest.mark.gpu
def test_restage_and_combine_rebuild_the_store(mods, pair):
    pair.iterate("start", 3)
    keep = np.ones(N_CELLS, np.uint8)
    keep[::5] = 0
    pair.both(lambda g: g.restage(keep=keep))
    pair.both(lambda g: g.ingest_finish(0, 0))
    pair.iterate("after restage", 3)
    src = mods["Cellector"](0)
    src.load_coo(N_LOCI, 301, *_coo(301, seed=8), min_alt=0, min_ref=0)
    pair.both(lambda g: g.combine(src))
    pair.both(lambda g: g.ingest_finish(0, 0))
    src.close()
    pair.iterate("after combine", 3)


@pytest.mark.gpu
def test_engine_switch_and_back(mods):
    """(an engine-2 ingest releases the by-locus CSC engine 1 walks, so the pair is ingested under engine 1)"""
    p = Pair(mods, 1, engine=1)
    try:
        p.iterate("engine 1 from the ingest", 1)
        p.both(lambda g: g.set_option("engine", 2))
        p.iterate("engine 2", 3)
        p.both(lambda g: g.set_option("engine", 1))
        p.iterate("engine 1", 2)  # alpha / beta move while engine 2's store is not kept up
        p.both(lambda g: g.set_option("engine", 2))
        p.iterate("engine 2 again", 3)
    finally:
        p.close()


@pytest.mark.gpu
def test_compute_expected_toggled(pair):
    pair.iterate("with the expected column", 2)
    pair.both(lambda g: g.set_option("compute_expected", 0))
    pair.iterate("without it", 2)
    _flip(pair, 3, 4)
    pair.iterate("without it, some loci dirty", 1)
    pair.both(lambda g: g.set_option("compute_expected", 1))
    pair.iterate("with it again", 3)  # (the values kept without the column must not serve)


@pytest.mark.gpu
def test_option_toggled_on_off_on(pair):
    pair.iterate("on", 3)
    pair.on.set_option("t2_cache", 0)
    pair.iterate("off", 2)  # alpha / beta move while the store is not kept up
    _flip(pair, 4, 5)
    pair.iterate("off, cells flipped", 1)
    pair.on.set_option("t2_cache", 1)
    pair.iterate("on again", 3)
    pair.on.set_option("t2_cache", -1)  # automatic: off at this size
    pair.iterate("automatic", 2)


@pytest.mark.gpu
@pytest.mark.parametrize("helper", [1, 0], ids=["dealt", "strided"])
@pytest.mark.parametrize("fill", [1, 0], ids=["fill", "bypass"])
def test_fill_rule_forced_both_ways_on_the_all_dirty_pass(mods, helper, fill):
    """the first pass after the ingest finds every locus dirty: forced to store, forced not to, then whatever the rule says"""
    p = Pair(mods, helper, fill)
    try:
        p.iterate(f"all dirty, t2_fill {fill}", 2)
        p.on.set_option("t2_fill", 1 - fill)
        p.iterate(f"t2_fill {1 - fill}", 2)
        p.on.set_option("t2_fill", -1)
        p.converge("the rule")
        p.iterate("at the fixed point", 2)
    finally:
        p.close()
