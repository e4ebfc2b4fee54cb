"""GPU: the donor calls from genotype probabilities (cellector_donor_weights / cellector_donor_posteriors_gp /
cellector_match_donors_gp; csrc/kernels_donors.hip) on both engines, against the hard calls, the numpy twin (cellector_amd/donors.py,
soft_*) and tests/donor_gp_reference.py.

The matrix is donor_reference.case_matrix() (677 cells x 487 loci) with D = 1, 2, 3, 5, 9, 16, 31, 32, 33, 64, as the hard calls'
tests.

What involves no exp or log is exact: the weights and kinds equal the twin's bit for bit; with the one-hot of a gt every output of the
soft calls is the hard calls' bytes; under soft rows the columns of the donors that are one-hot or no-call throughout are the twin's
bytes.  What passes through the device's exp and log is held to donor_gp_reference's derived bounds (the worst observed / bound
ratios are printed), the decisions exactly wherever the reference decides them by more than the bounds; undecided cells stay under
1 %.  The deep matrix (counts up to 2000 on one side) drives t_g - m below -745.
"""
import numpy as np
import pytest

import donor_gp_reference as gr
import donor_reference as dr
import test_gpu_tile_sweep as S

pytestmark = pytest.mark.gpu

ENGINES = pytest.mark.parametrize("engine", [2, 1], ids=["tiled", "csr"])
DONORS = pytest.mark.parametrize("D", dr.DONORS)
MASKED = pytest.mark.parametrize("masked", [False, True], ids=["all-loci", "masked"])
_mat = {}


@pytest.fixture(scope="module")
def mods(oracle_lib, hip_lib_path):
    from cellector_amd import Cellector, cluster, donors, ffi
    return dict(Cellector=Cellector, ffi=ffi, cl=cluster, dn=donors)


def _make(mods, engine, case=dr.case_matrix):
    L, N, coo = case()
    g = mods["Cellector"](0)
    g.set_option("engine", engine)
    g.load_coo(L, N, *S._u32(coo), 0, 0)
    assert g.dims().loci_used == L and np.array_equal(g.locus_ids(), np.arange(L, dtype=np.uint64))  # (every locus is used, in order)
    return g


def _matrix(mods, masked):
    if masked not in _mat:
        L, N, coo = dr.case_matrix()
        mask = dr.case_mask() if masked else None
        _mat[masked] = (mask, mods["cl"].Matrix(L, N, coo, mask))
    return _mat[masked]


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = (bytes(v) if k == "summary" else v.tobytes() for v in (a[k], b[k]))
        assert x == y, k


def _labels(N):
    labels = (np.arange(N) % 5).astype(np.uint8)
    labels[::7] = 255
    labels[labels == 3] = 255  # class 3 has no cell
    return labels


# ---- the weights -------------------------------------------------------------------------------------------------------------------
@ENGINES
def test_weights_are_the_twins(mods, engine):
    g = _make(mods, engine)
    for D in dr.DONORS:
        gp = gr.case_gp(D)
        w, kind = g.donor_weights(gp)
        tw, tk = mods["dn"].soft_weights(gp, np.arange(dr.CASE_L))
        rw, rk = gr.weights_reference(gp)
        assert w.tobytes() == tw.tobytes() == rw.tobytes() and kind.tobytes() == tk.tobytes() == rk.tobytes(), D
        assert set(np.unique(kind)) <= {0, 1, 2, 3, 4} and (kind == 4).any() and (w[kind == 3] == 0).all()
        ow, ok = g.donor_weights(mods["dn"].one_hot(dr.case_gt(D)))
        assert np.array_equal(ok, dr.case_gt(D).T) and np.array_equal(ow[ok < 3].sum(axis=1), np.ones((ok < 3).sum()))
    g.close()


# ---- one-hot rows: the hard calls' bytes ---------------------------------------------------------------------------------------------
@ENGINES
@MASKED
@DONORS
def test_one_hot_gp_is_the_hard_call(mods, D, masked, engine):
    g = _make(mods, engine)
    gt = dr.case_gt(D)
    gp = mods["dn"].one_hot(gt)
    mask, _ = _matrix(mods, masked)
    lp = dr.case_prior(D)
    given = (np.arange(dr.CASE_N) % D).astype(np.uint8)
    for prior, anchor, prm in ((None, None, {}), (lp, None, dict(doublet_rate=0.3, posterior_threshold=0.9, min_loci=3)),
                               (lp, given, dict(err=0.2, ambient=0.0)), (None, given, dict(doublet_rate=0.0))):
        _same(g.donor_posteriors_gp(gp, prior, anchor, mask, tables=True, **prm), g.donor_posteriors(gt, prior, anchor, mask, tables=True, **prm))
    labels = _labels(dr.CASE_N)
    for prm in ({}, dict(err=0.2, ambient=0.0)):
        _same(g.match_donors_gp(labels, 5, gp, mask, **prm), g.match_donors(labels, 5, gt, mask, **prm))
    g.close()


# ---- soft rows -----------------------------------------------------------------------------------------------------------------------
def _check(mods, g, D, masked, lp, anchor, **prm):
    L, N, coo = dr.case_matrix()
    gp = gr.case_gp(D)
    mask, mat = _matrix(mods, masked)
    dn = mods["dn"]
    got = g.donor_posteriors_gp(gp, lp, anchor, mask, tables=True, **prm)
    tabs = g.donor_tables(dr.case_gt(D), mask, **{k: v for k, v in prm.items() if k in ("err", "ambient")})
    assert got["tab1"].tobytes() == tabs["tab1"].tobytes() and got["tab2"].tobytes() == tabs["tab2"].tobytes()
    w, kind = dn.soft_weights(gp, np.arange(L))
    twin = dn.posteriors_gp(mat, w, kind, None, None, lp, got["anchor"], got["tab1"], got["tab2"], **prm)
    hard = np.array([gr.hard_donor(d) for d in range(D)])
    r = np.arange(N)
    assert got["ll"][:, hard].tobytes() == twin["ll"][:, hard].tobytes()
    by_hard = hard[got["anchor"]]  # cells anchored at a hard donor: their pair sums with hard donors pass through no exp
    assert got["pair_ll"][by_hard][:, hard].tobytes() == twin["pair_ll"][by_hard][:, hard].tobytes()
    assert got["pair_ll"][r, got["anchor"]].tobytes() == got["ll"][r, got["anchor"]].tobytes()
    assert (got["pair_posterior"][r, got["anchor"]] == 0).all()
    assert np.array_equal(got["anchor"], got["best"] if anchor is None else anchor)
    assert np.isfinite(got["ll"]).all() and np.isfinite(got["pair_ll"]).all()
    ref = gr.reference(L, N, coo, w, kind, got["tab1"], got["tab2"], lp, got["anchor"], mask, **prm)
    res, undecided = gr.compare(ref, got)
    print(D, masked, prm, {k: round(v, 3) for k, v in res.items()}, "undecided", int(undecided.sum()))
    assert max(res.values()) <= 1.0, res
    assert undecided.sum() < 0.01 * N, int(undecided.sum())
    total = got["posterior"].sum(axis=1) + got["doublet_posterior"]
    assert (np.abs(total - 1.0) <= (2 * D + 4) * np.spacing(1.0)).all()
    sm, st = got["summary"], got["status"]
    assert [sm.n_singlet, sm.n_doublet, sm.n_ambiguous, sm.n_unassigned] == [int((st == v).sum()) for v in (0, 1, 2, 255)]
    assert list(sm.donor_cells) == np.bincount(got["best"][st == 0], minlength=64).tolist()
    _same(got, g.donor_posteriors_gp(gp, lp, anchor, mask, tables=True, **prm))
    return got


@ENGINES
@MASKED
@DONORS
def test_soft_posteriors(mods, D, masked, engine):
    """flat prior and the cell's own anchor; then a prior with a donor ruled out and given anchors"""
    g = _make(mods, engine)
    got = _check(mods, g, D, masked, None, None)
    empty = got["n_entries"] == 0
    assert empty.any() and (got["ll"][empty] == 0).all() and (got["status"][empty] == 255).all()
    lp = dr.case_prior(D)
    second = _check(mods, g, D, masked, lp, (np.arange(dr.CASE_N) % D).astype(np.uint8), doublet_rate=0.3, posterior_threshold=0.9, min_loci=3)
    if D >= 2:
        assert (second["posterior"][:, D // 2] == 0).all() and (second["best"] != D // 2).all()
    g.close()


@ENGINES
@MASKED
def test_soft_match(mods, masked, engine):
    L, N, coo = dr.case_matrix()
    mask, _ = _matrix(mods, masked)
    dn = mods["dn"]
    g = _make(mods, engine)
    labels = _labels(N)
    cells, alt, ref = g.class_tallies(labels, 5)
    worst = 0.0
    for D in dr.DONORS:
        gp = gr.case_gp(D)
        got, again = g.match_donors_gp(labels, 5, gp, mask), g.match_donors_gp(labels, 5, gp, mask)
        tab1 = g.donor_tables(dr.case_gt(D), mask)["tab1"]
        w, kind = dn.soft_weights(gp, np.arange(L))
        twin = dn.match_gp(alt, ref, cells, w, kind, None, None, mask, tab1=tab1)
        hard = np.array([gr.hard_donor(d) for d in range(D)])
        assert got["ll"][:, hard].tobytes() == twin["ll"][:, hard].tobytes()
        ll, B = gr.match_reference(alt, ref, tab1, w, kind, mask)
        worst = max(worst, gr.ratio(got["ll"], ll, B))
        assert np.isfinite(got["ll"]).all() and worst <= 1.0, (D, worst)
        # best and margin follow from the device's own sums
        want = dn._match_calls(got["ll"], cells)
        assert np.array_equal(got["best"], want["best"]) and got["margin"].tobytes() == want["margin"].tobytes()
        assert np.array_equal(got["cells"], cells) and got["best"][3] == 255 and got["margin"][3] == 0
        assert all(got[k].tobytes() == again[k].tobytes() for k in got)
    print("match: worst observed / bound", round(worst, 3))
    g.close()


# ---- the deep matrix -------------------------------------------------------------------------------------------------------------------
@ENGINES
def test_deep_counts(mods, engine):
    """counts up to 2000 on one side: exp(t_g - m) underflows to 0 and the term is still m + log(w_m)"""
    L, N, coo = gr.deep_matrix()
    dn = mods["dn"]
    g = _make(mods, engine, gr.deep_matrix)
    for D in (2, 5, 33):
        gp = gr.deep_gp(D)
        got = g.donor_posteriors_gp(gp, tables=True)
        w, kind = dn.soft_weights(gp, np.arange(L))
        assert (kind == 4).any()
        for k in ("ll", "pair_ll", "posterior", "pair_posterior", "doublet_posterior"):
            assert np.isfinite(got[k]).all(), k
        ref = gr.reference(L, N, coo, w, kind, got["tab1"], got["tab2"], None, got["anchor"], None)
        res, undecided = gr.compare(ref, got)
        print("deep", D, {k: round(v, 3) for k, v in res.items()}, "undecided", int(undecided.sum()))
        assert max(res.values()) <= 1.0, res
        cells, alt, rf = g.class_tallies((np.arange(N) % 3).astype(np.uint8), 3)
        m = g.match_donors_gp((np.arange(N) % 3).astype(np.uint8), 3, gp)
        ll, B = gr.match_reference(alt, rf, got["tab1"], w, kind)
        assert np.isfinite(m["ll"]).all() and gr.ratio(m["ll"], ll, B) <= 1.0
    g.close()


# ---- the EM state stays ----------------------------------------------------------------------------------------------------------------
@ENGINES
def test_gp_calls_leave_the_loop_alone(mods, engine):
    mask = dr.case_mask()
    x, y = _make(mods, engine), _make(mods, engine)
    want = [x.em_iteration(5.0) for _ in range(4)]
    got = []
    labels = (np.arange(dr.CASE_N) % 3).astype(np.uint8)
    for it in range(4):
        got.append(y.em_iteration(5.0))
        if it == 1:
            state = (y.excluded(), y.loci_mask())
            y.donor_weights(gr.case_gp(33))
            y.donor_posteriors_gp(gr.case_gp(33), mask=mask)
            y.match_donors_gp(labels, 3, gr.case_gp(5), mask)
            assert np.array_equal(y.excluded(), state[0]) and np.array_equal(y.loci_mask(), state[1])
    assert [bytes(s) for s in got] == [bytes(s) for s in want], engine
    assert np.array_equal(x.excluded(), y.excluded()) and np.array_equal(x.loci_mask(), y.loci_mask())
    for k, v in x.cell_outputs().items():
        assert v.tobytes() == y.cell_outputs()[k].tobytes(), k
    x.close(); y.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(mods):
    ffi = mods["ffi"]
    L, N, coo = dr.case_matrix()
    gp3 = gr.case_gp(3)
    labels = (np.arange(N) % 2).astype(np.uint8)
    lib = ffi.load_library()

    def refused(fn, match):
        with pytest.raises(ffi.CellectorError, match=match) as e:
            fn()
        assert e.value.status == 1

    def every_call(g, gp, match, n=N):
        refused(lambda: g.donor_weights(gp), match)
        refused(lambda: g.donor_posteriors_gp(gp), match)
        refused(lambda: g.match_donors_gp(labels[:n], 2, gp), match)

    g = _make(mods, 2)
    state = (g.em_iteration(5.0), g.excluded(), g.loci_mask())
    for D in (0, 65):
        every_call(g, np.ones((D, L, 3), np.float32), "1..64 are supported")
    for row, what in (((0.5, np.nan, 0.5), "a NaN in one slot"), ((0.5, -0.25, 0.75), "a negative weight"), ((0.0, 0.0, 0.0), "all zero"),
                      ((np.inf, 0.0, 0.0), "an infinite weight")):
        bad = gp3.copy()
        bad[2, 17] = row
        every_call(g, bad, "gp of donor 2 at locus 17")
        # nothing written: the outputs keep what they held
        ll, w = np.full((N, 3), 7.0), np.full((L, 3, 3), 7.0)
        assert lib.cellector_donor_posteriors_gp(g.h, bad.ctypes.data, 3, None, None, None, None, ll.ctypes.data, *([None] * 13)) == 1, what
        assert lib.cellector_donor_weights(g.h, bad.ctypes.data, 3, w.ctypes.data, None) == 1, what
        assert (ll == 7.0).all() and (w == 7.0).all(), what
    for v in (0.0, 0.5, np.nan):
        refused(lambda: g.donor_posteriors_gp(gp3, err=v), "err")
        refused(lambda: g.match_donors_gp(labels, 2, gp3, err=v), "err")
    refused(lambda: g.donor_posteriors_gp(gp3, log_prior=np.full(3, -np.inf)), "every donor")
    anchor = np.zeros(N, np.uint8)
    anchor[9] = 3
    refused(lambda: g.donor_posteriors_gp(gp3, anchor=anchor), "anchor of cell 9")
    refused(lambda: g.match_donors_gp(np.full(N, 7, np.uint8), 2, gp3), "label 7")
    assert lib.cellector_donor_posteriors_gp(g.h, None, 3, *([None] * 18)) == 1 and b"null gp" in lib.cellector_last_error(g.h)
    assert lib.cellector_donor_weights(g.h, None, 3, None, None) == 1 and b"null gp" in lib.cellector_last_error(g.h)
    g.em_begin()
    every_call(g, gp3, "in flight")
    g.em_threshold(5.0)
    every_call(g, gp3, "in flight")
    g.em_finish()
    # the ctx is as it was: the loop goes on with the bits of an undisturbed one, and the calls work
    h = _make(mods, 2)
    assert bytes(h.em_iteration(5.0)) == bytes(state[0])
    h.em_iteration(5.0)
    assert bytes(g.em_iteration(5.0)) == bytes(h.em_iteration(5.0))
    assert np.array_equal(g.excluded(), h.excluded()) and np.array_equal(g.loci_mask(), h.loci_mask())
    h.close()
    assert g.donor_posteriors_gp(gp3)["summary"].n_unassigned == int((np.arange(N) % 10 == 0).sum())
    g.close()
    g = mods["Cellector"](0)
    assert lib.cellector_donor_posteriors_gp(g.h, gp3.ctypes.data, 3, *([None] * 18)) == 1 and b"no matrix loaded" in lib.cellector_last_error(g.h)
    g.close()
    m = mods["Cellector"](devices=[0, 0])
    m.load_coo(L, N, *S._u32(coo), 0, 0)
    every_call(m, gp3, "single-device")
    assert m.em_iteration(5.0) is not None
    m.close()
