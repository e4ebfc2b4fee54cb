"""GPU: the posterior phase (calculate_posteriors; csrc/kernels_tiled.hip tiled_posteriors / k_posterior_finalize, csrc/kernels_em.hip
k_ab_posterior / k_posterior, api_posteriors.cpp posterior_priors) held to an exact reference, the doublet set included.

Every other test of posterior and doublet_posterior compares with the oracle at 1e-6 absolute, which a value wrong by a factor of
e^5 passes in most cells (p ~ 1 or ~ 1e-30), and none looks at the doublet set's per-cell sum, which the ABI does not return.
Here a hand-built matrix is loaded, the exclusion set is placed with set_excluded (no EM run, so no near-threshold condition),
posteriors() is called and EVERY cell is compared with tests/posterior_reference.py: ll_minority and ll_majority within the bound of
their sums, posterior and doublet_posterior within a RELATIVE bound derived from the device's operations (1e-13 at the median,
4e-10 at most: posterior_reference's docstring has the count), or, where the reference is below 1e-290, below 1e-280 and not
negative.  tests/test_posterior_reference.py shows on the CPU that under this rule a doublet sum that is off by one term — the
smallest of the cell — is rejected in every cell that has one, on every case used here, so a misrouted lookup, a wrong stride or a
dropped partial sum of table set 2 cannot pass.

Matrices (the builders of tests/test_gpu_tile_sweep.py, the smallest shapes that reach these paths): the row-length matrix (5420
cells, rows of 0 to 639 entries, slices on the loop beyond 15 entries); the tier-2 matrix under ovf_deep 1 with t2_tiles 8, 6 and 0
(the second tile set, the ELL side path, a block without a tier-2 entry); a shallow ragged one (3 x 639 - 17 loci x 5 x 1024 + 1
cells); the second-trip matrix under tile_groups 64 with the planted set (a wrong 2 * set_stride or g * npad lands in another
set's partial sums).  Exclusion sets, each with a clamp of main.rs:240-259 on an edge: empty (mf0 = 1 / (N + 1) below both clamps,
minority alpha = beta = 1), three cells, the largest set with mf0 < 0.01 and the next one, the planted 7 % (between the 0.01 and the
0.1 clamp), 12 %, every second cell, all but one, all (mf = 1, lp_maj = -inf, majority alpha = beta = 1: every output finite).
Dispatch: engine 2 and engine 1; tile_sb 2 / 4 / 0 and overlap 0 / 1 / 2 (the same bits); a ctx of three logical shards (priors from
the global set size and N, output in global cell order); a ctx that ran the phase on another matrix before.  The reference of a
(matrix, set) is computed once and shared by all of them.

Exact claims (np.array_equal on the doubles): posterior_alpha_betas(0 / 1 / 2) is the numpy restatement bit for bit; posteriors()
twice, every tile_sb and every overlap return the same bits; assign() with resolve_posteriors 0 returns the four vectors of
posteriors() and the labels and quals ffi.assignments gives for them; cells without entries all get one and the same pair of
values.  (That pair is held to the chain's own bound, B = 0: a dozen roundings.  It is not asserted to equal a numpy evaluation bit
for bit: exp and log of the device and of numpy each carry up to an ulp and need not round alike.)

Worst observed / bound ratios are printed per case (pytest -s).
"""
import numpy as np
import pytest

import posterior_reference as pr
import test_gpu_tile_sweep as S

pytestmark = pytest.mark.gpu

DEEP = {8: (("ovf_deep", 1), ("t2_tiles", 8)), 6: (("ovf_deep", 1), ("t2_tiles", 6)), 0: (("ovf_deep", 1), ("t2_tiles", 0))}


@pytest.fixture(scope="module")
def mods(oracle_lib, hip_lib_path):
    import torch
    from cellector_amd import Cellector, ffi
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    return dict(Cellector=Cellector, ffi=ffi, ob=oracle_lib, ncu=ncu)


def _load(mods, mname, engine, opts=(), devices=None):
    """(ctx, G): the matrix loaded with every locus used; G = the partial sums a cell's sum is added from"""
    L, N, coo, _ = pr.matrix(mname)
    g = mods["Cellector"](devices=devices) if devices else mods["Cellector"](0)
    g.set_option("engine", engine)
    for k, v in opts:
        g.set_option(k, v)
    g.load_coo(L, N, *S._u32(coo), 0, 0)
    d = g.dims()
    assert (d.loci_used, d.total_cells, d.nnz_used) == (L, N, len(coo[0]))
    assert np.array_equal(g.locus_counts(), pr.case(mname, "planted")["locus_counts"])
    if engine == 1:
        return g, pr.WAVE_STEPS
    if devices:
        return g, pr.g_max(L, dict(opts).get("t2_tiles", 0))
    _, _, groups, _ = S._assert_geometry(mods, g, L, N, coo, opts)
    return g, S._n_partials(groups, L, opts)


def _same(a, b, tag):
    for k in pr.OUTPUTS:
        assert np.array_equal(a[k], b[k]), f"{tag}: {k} differs at {np.nonzero(a[k] != b[k])[0][:8]}"


def _check_alpha_betas(g, ref, tag):
    for which in (0, 1, 2):
        a, b = g.posterior_alpha_betas(which)
        assert np.array_equal(a, ref["ab"][which][0]) and np.array_equal(b, ref["ab"][which][1]), (tag, which)


def _place_and_check(tag, g, ref, G, worst):
    """place the set, run the phase, hold every cell to the reference; returns the four vectors"""
    g.set_excluded(ref["excluded"])
    assert np.array_equal(g.excluded() != 0, ref["excluded"])
    got = g.posteriors()
    res = pr.compare(ref, got, G)
    print(f"  {tag}: worst observed / bound " + ", ".join(f"{k} {res[k][0]:.3f}" for k in pr.OUTPUTS))
    assert all(bad.size == 0 for _, bad in res.values()), f"{tag}: " + pr.describe(ref, got, res, G)
    for k in pr.OUTPUTS:
        worst[k] = max(worst.get(k, 0.0), res[k][0])
    empty = ref["count"] == 0
    if empty.any():  # s = 0 in all three sets: the priors' quotient, one value for all of them
        for k in ("posterior", "doublet_posterior"):
            assert (got[k][empty] == got[k][empty][0]).all(), (tag, k)
        assert not got["ll_minority"][empty].any() and not got["ll_majority"][empty].any()
    return got


SWEEP = [("row-lengths", 2, ()), ("row-lengths", 1, ()), ("tier2", 2, DEEP[8]), ("tier2", 2, DEEP[6]), ("tier2", 2, DEEP[0]),
         ("tier2", 1, ()), ("shallow-ragged", 2, ()), ("shallow-ragged", 1, ()), ("second-trip", 2, (("tile_groups", 64),))]


@pytest.mark.parametrize("mname,engine,opts", SWEEP,
                         ids=[f"{m}-engine{e}" + "".join(f"-{k}{v}" for k, v in o if k != "ovf_deep") for m, e, o in SWEEP])
def test_every_cell_against_the_reference(mods, mname, engine, opts):
    """One ctx per (matrix, engine, options); every exclusion set placed on it in turn.  Per set: the three alpha / beta sets to the
    bit; the four outputs of every cell against the reference; the call again, every column width and every overlap mode: the same
    bits; assign(): the same four vectors, labels and quals by the rule on them."""
    ffi = mods["ffi"]
    g, G = _load(mods, mname, engine, opts)
    epc = g.entries_per_cell()
    assert np.array_equal(epc, pr.case(mname, "planted")["count"])
    worst = {}
    for sname in pr.set_names(mname):
        ref = pr.case(mname, sname)
        tag = f"{mname} engine {engine} {dict(opts).get('t2_tiles', '')} {sname}"
        got = _place_and_check(tag, g, ref, G, worst)
        _check_alpha_betas(g, ref, tag)
        assert all(np.isfinite(got[k]).all() for k in pr.OUTPUTS), tag
        _same(got, g.posteriors(), f"{tag}: second call")
        if engine == 2:
            for sb in (2, 4, 0):
                g.set_option("tile_sb", sb)
                _same(got, g.posteriors(), f"{tag}: tile_sb {sb}")
        for overlap in (0, 2, 1):
            g.set_option("overlap", overlap)
            _same(got, g.posteriors(), f"{tag}: overlap {overlap}")
        res = g.assign(0.999, 30)
        _same(got, res, f"{tag}: assign")
        pa, aa, q = ffi.assignments(got["posterior"], got["doublet_posterior"], epc, ref["excluded"])
        assert np.array_equal(res["posterior_assignment"], pa) and np.array_equal(res["anomaly_assignment"], aa), tag
        assert np.array_equal(res["qual"], q), (tag, np.nonzero(res["qual"] != q)[0][:8])
    print(f"  {mname} engine {engine} {dict(opts)}: G = {G}; worst over the sets " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    g.close()


@pytest.mark.parametrize("engine", [2, 1], ids=["tiled", "csr"])
@pytest.mark.parametrize("mname", ["row-lengths", "tier2", "shallow-ragged"])
def test_three_logical_shards(mods, mname, engine):
    """Cellector(devices=[0, 0, 0]): every shard runs the phase on its cells with the priors of the GLOBAL set size and N and the
    alpha / beta of the all-reduced tallies; the output is in global cell order.  G: the largest a shard's geometry can have."""
    g, G = _load(mods, mname, engine, devices=[0, 0, 0])
    worst = {}
    for sname in pr.set_names(mname):
        ref = pr.case(mname, sname)
        tag = f"{mname} engine {engine} three shards {sname}"
        got = _place_and_check(tag, g, ref, G, worst)
        _check_alpha_betas(g, ref, tag)
        _same(got, g.posteriors(), f"{tag}: second call")
    print(f"  {mname} engine {engine} three shards: G = {G}; worst over the sets " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    g.close()


@pytest.mark.parametrize("engine", [2, 1], ids=["tiled", "csr"])
def test_a_ctx_that_ran_the_phase_on_another_matrix(mods, engine):
    """the tier-2 matrix after the shallow ragged one on one ctx (twice the cells, fewer loci: another set of tile buffers and
    partial sums): the bits of a fresh ctx, and every cell inside the bound"""
    opts = DEEP[8] if engine == 2 else ()
    fresh, G = _load(mods, "tier2", engine, opts)
    L, N, coo, _ = pr.matrix("shallow-ragged")
    h = mods["Cellector"](0)
    h.set_option("engine", engine)
    for k, v in opts:
        h.set_option(k, v)
    h.load_coo(L, N, *S._u32(coo), 0, 0)
    h.set_excluded(pr.exclusion_set("shallow-ragged", "every-second"))
    h.posteriors()
    L, N, coo, _ = pr.matrix("tier2")
    h.load_coo(L, N, *S._u32(coo), 0, 0)
    worst = {}
    for sname in ("planted", "all", "empty"):
        ref = pr.case("tier2", sname)
        want = _place_and_check(f"fresh ctx, engine {engine} {sname}", fresh, ref, G, worst)
        got = _place_and_check(f"used ctx, engine {engine} {sname}", h, ref, G, worst)
        _same(want, got, f"engine {engine} {sname}: a ctx that ran the phase on another matrix")
    fresh.close(); h.close()


@pytest.mark.parametrize("engine", [2, 1], ids=["tiled", "csr"])
@pytest.mark.parametrize("mname", ["tier2", "row-lengths"])
def test_the_phase_leaves_the_loop_alone(mods, mname, engine):
    """tiled_posteriors rebuilds table set 0 and reuses the column counters of the EM pass (tables_prebuilt = false, work_zeroed =
    false).  A ctx that calls posteriors() between two iterations must produce the second iteration's summary, cell_outputs() and
    locus_outputs() bit-identical to a twin that did not; then the other way round: its posteriors after that iteration are the
    twin's."""
    opts = DEEP[8] if (engine == 2 and mname == "tier2") else ()
    x, _ = _load(mods, mname, engine, opts)
    y, _ = _load(mods, mname, engine, opts)
    for it in range(2):
        sx, sy = x.em_iteration(5.0), y.em_iteration(5.0)
        assert bytes(sx) == bytes(sy), (mname, engine, it)
        for fetch in ("cell_outputs", "locus_outputs"):
            ox, oy = getattr(x, fetch)(), getattr(y, fetch)()
            for k in ox:
                assert ox[k].tobytes() == oy[k].tobytes(), (mname, engine, it, fetch, k)
        assert np.array_equal(x.excluded(), y.excluded()) and np.array_equal(x.loci_mask(), y.loci_mask())
        if it == 0:
            assert sx.n_excluded > 0
            x.posteriors()
            x.assign(0.999, 30)
    _same(x.posteriors(), y.posteriors(), f"{mname} engine {engine}: posteriors after the second iteration")
    x.close(); y.close()
