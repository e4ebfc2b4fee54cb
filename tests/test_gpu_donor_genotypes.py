"""GPU: cellector_donor_genotypes (csrc/kernels_donor_genotypes.hip) on both engines' ctxs against plain integers, the numpy twin
cellector_amd/donor_genotypes.py, the 80-bit reference tests/donor_genotypes_reference.py, cellector_class_genotypes, the final
tallies and cellector_donor_tables.  The tallies, cells and the decided gt_out / kind are exact; la / lb at the used loci are
tab1's bits; q is held to the reference's derived bound.  Every matrix has at most 900 cells x 600 loci.

The tally kernel's edges (a block takes 4096 entries, its LDS window holds 4096 / (D + 1) loci, made odd): donor_genotypes_reference
.edge_matrix has a locus of 4500 entries across the first block edge (every pair five times over, 300 counts of 65535), 99 used loci
and a run of 500 single-entry loci that fail the filter but hold reads, longer than the window for D >= 16: there the entries past
the window take the direct path.  For small D the window holds up to 2047 loci: test_a_sparse_run_longer_than_any_window stages 2550
single-entry loci in one block's run, so the direct path runs at D = 1 and D = 2 as well.  The staged COO of a loaded matrix is always
locus-major (the build sorts by locus whatever order ingest_coo was given), so "shuffled" below changes the order of the cells inside
a locus and the order the build's sort sees, not what the tally kernel's window test meets; a locus below a block's first one cannot
be staged through the library.
"""
import numpy as np
import pytest

import donor_genotypes_reference as gr

pytestmark = pytest.mark.gpu

DS = (1, 2, 16, 31, 32, 33, 64)  # (16: the last D cellector_class_genotypes' planes can be compared at)
ERR, AMB = 0.02, 0.05


@pytest.fixture(scope="module")
def mods(hip_lib_path):
    from cellector_amd import Cellector, donor_genotypes, ffi, synth
    return dict(Cellector=Cellector, ffi=ffi, dg=donor_genotypes, synth=synth)


def _u32(coo):
    return [np.ascontiguousarray(x, np.uint32) for x in coo]


def _load(mods, TL, N, coo, engine=2, min_alt=4, min_ref=4):
    g = mods["Cellector"](0)
    g.set_option("engine", engine)
    g.load_coo(TL, N, *_u32(coo), min_alt, min_ref)
    return g


def _check(mods, g, TL, coo, assign, D, prior, classes=True, **kw):
    """one call against everything the module docstring names; coo: the entries the caller staged, in any order.  Returns the
    library's dict."""
    dg = mods["dg"]
    kw = dict(dict(err=ERR, ambient=AMB), **kw)
    got = g.donor_genotypes(assign, prior, n_donors=D, **kw)
    # plain integers, and the twin on the ctx's own staged entries
    cells, alt, ref = gr.tally_reference(TL, coo, assign, D)
    for k, want in (("cells", cells), ("alt", alt), ("ref", ref)):
        assert got[k].dtype == np.uint64 and np.array_equal(got[k], want), (D, k)
    tc, ta, tr_ = dg.tallies(TL, g.staged_coo(), assign, D)
    assert np.array_equal(tc, cells) and np.array_equal(ta, alt) and np.array_equal(tr_, ref)
    # the tallies alone: the same planes
    only = g.donor_genotypes(assign, None, n_donors=D, posterior=False)
    assert set(only) == {"cells", "alt", "ref"} and np.array_equal(only["alt"], alt) and np.array_equal(only["ref"], ref)
    # the D + 1 slots add up to the final tallies' totals
    fin = g.final_allele_tallies()
    assert np.array_equal(got["alt"].sum(axis=0), fin["alt_min"] + fin["alt_maj"])
    assert np.array_equal(got["ref"].sum(axis=0), fin["ref_min"] + fin["ref_maj"])
    # the class genotypes' planes on the same labels
    if classes and D <= 16 and (assign != 255).any():
        cg = g.class_genotypes(assign, D, genotypes=False)
        assert np.array_equal(cg["alt"], alt) and np.array_equal(cg["ref"], ref) and np.array_equal(cg["cells"], cells)
    # la / lb at the used loci are tab1's bits
    ids = g.locus_ids().astype(np.int64)
    tab1 = g.donor_tables(np.zeros((D, TL), np.uint8), err=kw["err"], ambient=kw["ambient"])["tab1"]
    assert len(ids) > 0 and got["tab"][ids].tobytes() == np.ascontiguousarray(tab1[:, :3]).tobytes(), D
    assert gr.compare_tab(alt, ref, kw["err"], kw["ambient"], got["tab"]) <= 1.0
    # q within the derived bound; gt_out and kind wherever the reference decides them, and there the twin's too
    r = gr.reference(alt, ref, got["tab"], prior, **kw)
    res, undecided = gr.compare(r, got)
    print(D, {k: round(v, 3) for k, v in res.items()}, "undecided", int(undecided.sum()))
    assert max(res.values()) <= 1.0, (D, res)
    assert undecided.sum() <= 0.01 * max(int((r["depth"] > 0).sum()), 1)
    twin = dg.posterior(alt, ref, got["tab"], prior, **kw)
    assert np.array_equal(twin["gt_out"][~undecided], got["gt_out"][~undecided])
    assert np.array_equal(twin["kind"][~undecided], got["kind"][~undecided])
    want = dg.summary(cells, got["kind"])
    assert sorted(want) == sorted(got["summary"])
    for k in want:
        assert np.array_equal(want[k], got["summary"][k]), k
    return got


@pytest.fixture(scope="module", params=[1, 2])
def edge(request, mods):
    """the edge matrix on one engine's ctx, staged locus-major and staged in a random order through ingest_coo (the build sorts it)"""
    TL, N, coo = gr.edge_matrix()
    perm = np.random.default_rng(12).permutation(len(coo[0]))
    shuffled = [x[perm] for x in coo]
    a, b = _load(mods, TL, N, coo, request.param), _load(mods, TL, N, shuffled, request.param)
    yield dict(TL=TL, N=N, coo=coo, sorted=a, shuffled=b, engine=request.param)
    a.close(); b.close()


@pytest.mark.parametrize("D", DS)
def test_edge_matrix_sorted_and_shuffled(mods, edge, D):
    TL, N, coo = edge["TL"], edge["N"], edge["coo"]
    d = edge["sorted"].dims()
    assert d.total_loci == TL and 0 < d.loci_used <= 100  # (the 500 single-entry loci fail min_alt / min_ref = 4)
    assign, prior = gr.edge_assign(D), gr.case_prior(D, TL, "soft")
    a = _check(mods, edge["sorted"], TL, coo, assign, D, prior)
    b = _check(mods, edge["shuffled"], TL, coo, assign, D, prior, classes=False)
    for k in ("cells", "alt", "ref", "tab", "q", "gt_out", "kind"):
        assert a[k].tobytes() == b[k].tobytes(), k
    failed = np.setdiff1d(np.arange(TL), edge["sorted"].locus_ids().astype(np.int64))
    assert a["alt"][:, failed].any() and (a["kind"][:, failed] != 0).any()
    assert a["alt"][:, 0].sum() > 300 * 65535 - 1 and a["alt"][:, 300:310].sum() == 0 and (a["kind"][:, 300:310] == 0).all()
    if D >= 2:  # (edge_assign leaves the last donor without a cell: its floored prior, kind 0 everywhere)
        assert a["cells"][D - 1] == 0 and (a["kind"][D - 1] == 0).all() and (a["gt_out"][D - 1] == 3).sum() > 0


@pytest.mark.parametrize("D", (1, 33))
def test_no_cell_assigned_and_no_prior(mods, edge, D):
    TL, N, coo = edge["TL"], edge["N"], edge["coo"]
    for g in (edge["sorted"], edge["shuffled"]):
        got = _check(mods, g, TL, coo, gr.edge_assign(D, mode="none"), D, None)
        assert not got["alt"][:D].any() and not got["ref"][:D].any() and got["alt"][D].any() and got["cells"].tolist() == [0] * D + [N]
        assert (got["kind"] == 0).all() and (got["gt_out"] == 3).all() and (got["q"] == 1.0 / 3.0).all()
    got = _check(mods, edge["sorted"], TL, coo, gr.edge_assign(D), D, None, prior_floor=0.0, gt_threshold=0.9)
    assert set(np.unique(got["kind"]).tolist()) <= {0, 2, 4} and (got["kind"] == 2).any()


@pytest.mark.parametrize("engine", [1, 2])
def test_a_sum_beyond_32_bits_in_one_block(mods, engine):
    """4096 entries of one locus and one donor at alt = ref = 65535 fill one block's LDS counter to its bound (268 431 360 a half),
    seventeen such blocks pass 2^32 in the plane; an eighteenth block mixes donors"""
    n, N = 18 * 4096, 900
    rng = np.random.default_rng(2)
    lo, ce = np.zeros(n, np.int64), np.concatenate([np.zeros(17 * 4096, np.int64), rng.integers(0, N, 4096)])
    al, re = np.full(n, 65535), np.full(n, 65535)
    lo = np.concatenate([lo, [1, 1, 2]]); ce = np.concatenate([ce, [5, 5, 6]]); al = np.concatenate([al, [3, 3, 1]]); re = np.concatenate([re, [1, 1, 0]])
    g = _load(mods, 3, N, (lo, ce, al, re), engine)
    assign = (np.arange(N) % 2).astype(np.uint8)
    got = _check(mods, g, 3, (lo, ce, al, re), assign, 2, None)
    assert got["alt"][0, 0] > 2 ** 32 and got["alt"][:, 1].tolist() == [0, 6, 0] and got["ref"][:, 2].tolist() == [0, 0, 0]
    assert np.isfinite(got["q"]).all() and got["gt_out"][0, 0] == 1  # (1.1e9 reads a side: a het, and no NaN)
    g.close()


@pytest.mark.parametrize("engine", [1, 2])
def test_a_sparse_run_longer_than_any_window(mods, engine):
    """2550 loci of one entry each, then 50 loci of 40 entries: the first block's run of 4096 entries spans 2588 loci, more than the
    window at every D (2047 at D = 1, 1365 at D = 2, 239 at D = 16, 63 at D = 64), so entries of the same block go through the LDS
    and through the direct path, the used loci among the latter"""
    TL, N = 2600, 300
    rng = np.random.default_rng(14)
    lo = np.concatenate([np.arange(2550), np.repeat(np.arange(2550, 2600), 40)])
    ce = np.concatenate([rng.integers(0, N, 2550), np.concatenate([np.sort(rng.choice(N, 40, replace=False)) for _ in range(50)])])
    tot = rng.integers(1, 9, len(lo))
    al = rng.binomial(tot, rng.choice([0.02, 0.5, 0.98], len(lo)))
    coo = (lo, ce, al, tot - al)
    g = _load(mods, TL, N, coo, engine)
    assert g.dims().loci_used == 50 and np.array_equal(g.staged_coo()[0], lo)
    for D in (1, 2, 16, 64):
        got = _check(mods, g, TL, coo, gr.case_assign(D, N, seed=5), D, gr.case_prior(D, TL, "onehot"))
        assert got["alt"][:, 2047:2550].any() and got["alt"][:, 2550:].any() and (got["kind"][:, :2550] != 0).any()
    g.close()


@pytest.mark.parametrize("engine", [1, 2])
def test_called_matrix_through_ingest_combine_and_join(mods, engine):
    """the pool with planted genotypes: staged as it is, as two halves combined, and as an alt and a ref stream joined by (locus,
    cell), each stream in an order of its own: the same planes, the same bytes behind them; the calls recover the planted genotypes"""
    dg = mods["dg"]
    D = 33
    TL, N, coo, assign, truth = gr.called_matrix(D)
    prior = gr.prior_of(truth, "onehot")
    g = _load(mods, TL, N, coo, engine)
    a = _check(mods, g, TL, coo, assign, D, prior)
    g.close()
    called = (a["kind"] >= 1) & (a["kind"] <= 3)  # (a call at a site with reads; the twin on the CPU: 7758 sites, 99.3 % the truth)
    assert called.sum() > 0.5 * called.size and (a["gt_out"][called] == truth[called]).mean() > 0.99
    assert (a["gt_out"][a["kind"] == 3] == truth[a["kind"] == 3]).all() and (a["kind"] == 3).sum() > 20
    assert set(np.unique(a["kind"]).tolist()) == {0, 1, 2, 3, 4}
    # two halves of the cells, combined
    lo, ce, al, re = coo
    first = ce < N // 2
    x = _load(mods, TL, N // 2, [v[first] for v in coo], engine)
    y = _load(mods, TL, N - N // 2, [lo[~first], ce[~first] - N // 2, al[~first], re[~first]], engine)
    x.combine(y)
    x.ingest_finish(4, 4)
    b = _check(mods, x, TL, coo, assign, D, prior)
    x.close(); y.close()
    # two streams joined
    rng = np.random.default_rng(4)
    p1, p2 = rng.permutation(len(lo)), rng.permutation(len(lo))
    j = mods["Cellector"](0)
    j.set_option("engine", engine)
    j.ingest_coo_joined(TL, N, _u32([lo[p1], ce[p1], al[p1]]), _u32([lo[p2], ce[p2], re[p2]]), "ref")
    j.ingest_finish(4, 4)
    c = _check(mods, j, TL, coo, assign, D, prior)
    j.close()
    for other in (b, c):
        for k in ("cells", "alt", "ref", "tab", "q", "gt_out", "kind"):
            assert a[k].tobytes() == other[k].tobytes(), k
    # to_gp and prior_from_gt feed the donor call
    assert dg.to_gp(a["q"]).dtype == np.float32 and np.array_equal(np.isnan(dg.prior_from_gt(a["gt_out"])).all(axis=2), a["gt_out"] == 3)


def test_refine_donors_on_a_planted_pool(mods):
    """calls and genotypes in turn on planted pool 6 under its damaged genotypes: the loop ends, no singlet is lost, the flipped
    calls come back (tests/test_donor_genotypes_reference.py measures the same with the reference: 898 -> 900 singlets)"""
    dg = mods["dg"]
    P = gr.planted(6)
    g = _load(mods, P["L"], P["N"], P["coo"], 2, 0, 0)
    prior = dg.prior_from_gt(P["damaged"])
    before = g.donor_posteriors_gp(prior)
    don, gen, rounds = g.refine_donors(prior, max_iter=10)
    g.close()
    single = P["truth_cell"] != 255
    ok = lambda r: int(((r["status"] == 0) & (r["best"] == P["truth_cell"]))[single].sum())
    print("refine_donors: rounds", rounds, "singlets before", ok(before), "after", ok(don))
    assert 2 <= rounds < 10 and ok(don) >= ok(before) and ok(don) >= 898
    fl = P["flipped"] & (P["full"] != 3)
    assert (gen["gt_out"][fl] == P["full"][fl]).mean() >= 0.95 and (gen["kind"][3] == 0).all()


def test_the_loop_continues_with_the_same_bits(mods):
    TL, N = 1500, 700
    coo = mods["synth"].generate_coo(TL, N, 0.10, seed=4, minority_fraction=0.08)
    x, y = _load(mods, TL, N, coo), _load(mods, TL, N, coo)
    want = x.run(5.0, 40)
    assert len(want) >= 2 and not want[-1].any_change
    want.append(x.em_iteration(5.0))  # (one more at the fixed point: an iteration follows the interruption)
    got = []
    for it in range(len(want)):
        got.append(y.em_iteration(5.0))
        if it == 1:
            state = (y.excluded(), y.loci_mask())
            y.donor_genotypes(gr.case_assign(64, N), gr.case_prior(64, TL, "soft"))
            y.donor_genotypes(gr.case_assign(3, N), None, n_donors=3, posterior=False)
            assert np.array_equal(y.excluded(), state[0]) and np.array_equal(y.loci_mask(), state[1])
    assert [bytes(s) for s in got] == [bytes(s) for s in want]
    assert np.array_equal(x.excluded(), y.excluded()) and np.array_equal(x.loci_mask(), y.loci_mask())
    for k, v in x.cell_outputs().items():
        assert v.tobytes() == y.cell_outputs()[k].tobytes(), k
    x.close(); y.close()


def test_refusals(mods):
    ffi = mods["ffi"]
    TL, N = 37, 50
    rng = np.random.default_rng(2)
    coo = (np.sort(rng.integers(0, TL, 300)), rng.integers(0, N, 300), rng.integers(0, 6, 300), rng.integers(0, 6, 300))
    assign = (np.arange(N) % 3).astype(np.uint8)
    prior = gr.case_prior(3, TL, "soft")

    def refused(fn, match):
        with pytest.raises(ffi.CellectorError, match=match) as e:
            fn()
        assert e.value.status == 1

    g = _load(mods, TL, N, coo, 2, 0, 0)
    for D in (0, 65):
        refused(lambda: g.donor_genotypes(np.zeros(N, np.uint8), None, n_donors=D), "1..64 are supported")
    bad = assign.copy()
    bad[5] = 3
    refused(lambda: g.donor_genotypes(bad, prior), "assign of cell 5 is 3")
    for row in ([np.nan, 0.5, 0.5], [0, 0, 0], [-1, 1, 1], [np.inf, 0, 0]):
        p = prior.copy()
        p[1, 7] = row
        refused(lambda: g.donor_genotypes(assign, p), "of donor 1 at locus 7")
    for v in (1.5, -0.1, np.nan):
        refused(lambda: g.donor_genotypes(assign, prior, gt_threshold=v), "gt_threshold")
        refused(lambda: g.donor_genotypes(assign, prior, prior_floor=v), "prior_floor")
    for v in (0.0, 0.5, np.nan):
        refused(lambda: g.donor_genotypes(assign, prior, err=v), r"err = .* is not within \(0, 0.5\)")
    for v in (1.0, -0.1, np.nan):
        refused(lambda: g.donor_genotypes(assign, prior, ambient=v), r"ambient = .* is not within \[0, 1\)")
    lib = ffi.load_library()
    assert lib.cellector_donor_genotypes(g.h, None, None, 3, *([None] * 10)) == 1 and b"null assign" in lib.cellector_last_error(g.h)
    g.em_begin()
    refused(lambda: g.donor_genotypes(assign, prior), "in flight")
    g.em_threshold(5.0)
    g.em_finish()
    # usable afterwards, every output optional, the bounds of the two new parameters included
    assert lib.cellector_donor_genotypes(g.h, assign.ctypes.data, None, 3, *([None] * 10)) == 0
    got = g.donor_genotypes(assign, prior, gt_threshold=1.0, prior_floor=1.0)
    assert got["cells"].tolist() == [17, 17, 16, 0] and (got["gt_out"] == 3).all()
    assert g.donor_genotypes(assign, prior, gt_threshold=0.0, prior_floor=0.0, timing=True)["pass_ms"].min() >= 0.0
    g.close()
    g = mods["Cellector"](0)
    refused(lambda: g.donor_genotypes(assign, prior), "no matrix loaded")
    g.close()
    g = mods["Cellector"](0)
    g.set_option("keep_coo", 0)
    g.load_coo(TL, N, *_u32(coo), 0, 0)
    refused(lambda: g.donor_genotypes(assign, prior), r"needs the staged COO \(option keep_coo=1\)")
    g.close()
    m = mods["Cellector"](devices=[0, 0, 0])
    m.load_coo(TL, N, *_u32(coo), 0, 0)
    refused(lambda: m.donor_genotypes(assign, prior), "single-device")
    m.close()
    g = mods["Cellector"](0)
    g.set_shard(10, 40)
    g.load_coo(TL, N, *_u32(coo), 0, 0)
    refused(lambda: g.donor_genotypes(assign[:30], prior), "set_shard")
    g.close()
