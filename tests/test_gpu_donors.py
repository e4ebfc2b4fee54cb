"""GPU: donor demultiplexing (cellector_donor_tables / cellector_donor_posteriors / cellector_match_donors;
csrc/kernels_donors.hip) on both engines, against the numpy twin cellector_amd/donors.py and tests/donor_reference.py.

The matrix is donor_reference.case_matrix(): 677 cells x 487 loci, rows of 0, 1 ... 9 entries around the prefetch depth (a few up to
18), repeated pairs, a cell count no rows-per-wave divides.  D = 1, 2, 3, 5, 9, 16, 31, 32, 33, 64: every lane width, counts that
are no power of two, the edge of the packed word, the full wave; a donor and a locus without any call.

Where the order of the operations is fixed the claim is exact: the packed words equal the definition's, the singlet, pair and match
sums equal the twin's fed the device's tables bit for bit (tobytes), the (x + x) / 2 column is the singlet sum's bits.  What passes
through the device's log or exp is held to donor_reference's derived bounds: the tables within one ulp of log (C_LOG = 2 units of
2^-53 relative; ROCm device-libs documents 1 ulp), the posteriors within the bounds of their chain.  best / second / best_pair /
status are compared exactly wherever the reference decides them by more than the bounds; the cells it does not are counted and stay
under 1 % (tests/test_donor_reference.py asserts the same share for the twin, on the CPU).  The tests never compare with planted
truth.
"""
import numpy as np
import pytest

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


def _make(mods, engine):
    L, N, coo = dr.case_matrix()
    g = mods["Cellector"](0)
    g.set_option("engine", engine)
    g.load_coo(L, N, *S._u32(coo), 0, 0)
    assert g.dims().loci_used == L and g.dims().nnz_used == len(coo[0])  # (min_alt = min_ref = 0: every locus is used)
    assert np.array_equal(g.locus_ids(), np.arange(L, dtype=np.uint64))
    return g


def _matrix(mods, masked):
    if masked not in _mat:
        L, N, coo = dr.case_matrix()
        mask = dr.case_mask() if masked else None
        _mat[masked] = (mask, mods["cl"].Matrix(L, N, coo, mask))
    return _mat[masked]


# ---- what the tables are made from -------------------------------------------------------------------------------------------------
@ENGINES
def test_locus_counts_are_the_whole_number_totals(mods, engine):
    """the A and R of the model are what cellector_locus_counts returns: the loci's alt and ref sums over all entries, exactly"""
    L, N, coo = dr.case_matrix()
    A, R = dr.totals(L, coo)
    g = _make(mods, engine)
    lc = g.locus_counts()
    assert np.array_equal(lc[:, 1], A) and np.array_equal(lc[:, 0], R)
    g.close()


@ENGINES
def test_packed_words_and_tables(mods, engine):
    L, N, coo = dr.case_matrix()
    A, R = dr.totals(L, coo)
    g = _make(mods, engine)
    for D in dr.DONORS:
        gt = dr.case_gt(D)
        for mask, prm in ((None, {}), (dr.case_mask(), dict(err=0.2, ambient=0.0)), (dr.case_mask(), dict(err=1e-6, ambient=0.9))):
            t = g.donor_tables(gt, mask, **prm)
            assert np.array_equal(t["packed"], dr.pack_reference(gt))
            p = dr.params(**prm)
            res = dr.compare_tabs(A, R, p["err"], p["ambient"], mask, t["tab1"], t["tab2"])
            print(D, prm, {k: round(v, 3) for k, v in res.items()})
            assert max(res.values()) <= 1.0, (D, prm, res)
            for gg in range(4):
                assert t["tab2"][:, 5 * gg].tobytes() == t["tab1"][:, gg].tobytes()
            if mask is not None:
                assert (t["tab1"][mask == 0] == 0).all() and (t["tab2"][mask == 0] == 0).all()
            again = g.donor_tables(gt, mask, **prm)
            assert all(t[k].tobytes() == again[k].tobytes() for k in t)
    g.close()


# ---- the cell calls ------------------------------------------------------------------------------------------------------------------
def _check(mods, g, D, masked, lp, anchor, **prm):
    L, N, coo = dr.case_matrix()
    gt = dr.case_gt(D)
    mask, mat = _matrix(mods, masked)
    dn = mods["dn"]
    got = g.donor_posteriors(gt, lp, anchor, mask, tables=True, **prm)
    gu = gt.T  # (every locus is used, in order)
    s = dn.singlet_sums(mat, got["tab1"], gu)
    assert got["ll"].tobytes() == s.tobytes(), np.abs(got["ll"] - s).max()
    p = dn.pair_sums(mat, got["tab2"], gu, got["anchor"])
    assert got["pair_ll"].tobytes() == p.tobytes(), np.abs(got["pair_ll"] - p).max()
    r = np.arange(N)
    assert got["pair_ll"][r, got["anchor"]].tobytes() == got["ll"][r, got["anchor"]].tobytes()  # (x + x) 0.5 == x
    assert (got["pair_posterior"][r, got["anchor"]] == 0).all()
    assert np.array_equal(got["anchor"], got["best"] if anchor is None else anchor)
    ref = dr.reference(L, N, coo, gt, got["tab1"], got["tab2"], lp, got["anchor"], mask, **prm)
    res, undecided = dr.compare(ref, got)
    print(D, masked, prm, {k: round(v, 3) for k, v in res.items()}, "undecided", int(undecided.sum()))
    assert max(res.values()) <= 1.0, res
    assert undecided.sum() < 0.01 * N, int(undecided.sum())
    total = got["posterior"].sum(axis=1) + got["doublet_posterior"]
    assert (np.abs(total - 1.0) <= (2 * D + 4) * np.spacing(1.0)).all()
    sm, st = got["summary"], got["status"]
    assert [sm.n_singlet, sm.n_doublet, sm.n_ambiguous, sm.n_unassigned] == [int((st == v).sum()) for v in (0, 1, 2, 255)]
    assert list(sm.donor_cells) == np.bincount(got["best"][st == 0], minlength=64).tolist()
    if D == 1:
        assert (got["second"] == 255).all() and (got["best_pair"] == 255).all() and (got["doublet_posterior"] == 0).all()
    again = g.donor_posteriors(gt, lp, anchor, mask, tables=True, **prm)
    for k, v in got.items():
        assert (bytes(v) if k == "summary" else v.tobytes()) == (bytes(again[k]) if k == "summary" else again[k].tobytes()), k
    return got


@ENGINES
@MASKED
@DONORS
def test_posteriors_flat_prior_own_anchor(mods, D, masked, engine):
    g = _make(mods, engine)
    got = _check(mods, g, D, masked, None, None)
    empty = got["n_entries"] == 0
    assert empty.any() and (got["ll"][empty] == 0).all() and (got["status"][empty] == 255).all()
    g.close()


@ENGINES
@MASKED
@DONORS
def test_posteriors_prior_with_a_donor_ruled_out_and_given_anchors(mods, D, masked, engine):
    """a log_prior with one -inf donor; anchors: every cell's WORST donor under that prior, then donor (cell mod D)"""
    g = _make(mods, engine)
    lp = dr.case_prior(D)
    first = _check(mods, g, D, masked, lp, None, doublet_rate=0.3, posterior_threshold=0.9, min_loci=3)
    if D >= 2:
        assert (first["posterior"][:, D // 2] == 0).all() and (first["best"] != D // 2).all()
    assert (first["status"][first["n_entries"] < 3] == 255).all() and (first["status"][first["n_entries"] >= 3] != 255).all()
    worst = np.argmin(np.where(np.isfinite(lp)[None, :], first["ll"] + lp[None, :], np.inf), axis=1).astype(np.uint8)
    _check(mods, g, D, masked, lp, worst)
    _check(mods, g, D, masked, None, (np.arange(dr.CASE_N) % D).astype(np.uint8), doublet_rate=0.0)
    g.close()


@ENGINES
def test_a_mask_of_zeros(mods, engine):
    """no locus left: every sum 0, every cell unassigned at min_loci 1"""
    g = _make(mods, engine)
    zeros = np.zeros(dr.CASE_L, np.uint8)
    for D in (1, 5, 64):
        got = g.donor_posteriors(dr.case_gt(D), mask=zeros, tables=True)
        assert (got["ll"] == 0).all() and (got["pair_ll"] == 0).all() and (got["n_entries"] == 0).all()
        assert (got["status"] == 255).all() and got["summary"].n_unassigned == dr.CASE_N
        assert (got["tab1"] == 0).all() and (got["tab2"] == 0).all() and (got["best"] == 0).all()
        m = g.match_donors((np.arange(dr.CASE_N) % 2).astype(np.uint8), 2, dr.case_gt(D), zeros)
        assert (m["ll"] == 0).all() and (m["best"] == 0).all()
    g.close()


# ---- classes against donors ----------------------------------------------------------------------------------------------------------
@ENGINES
@MASKED
def test_match_sums_are_the_twins(mods, masked, engine):
    L, N, coo = dr.case_matrix()
    mask, _ = _matrix(mods, masked)
    dn = mods["dn"]
    g = _make(mods, engine)
    labels = (np.arange(N) % 5).astype(np.uint8)
    labels[::7] = 255
    labels[labels == 3] = 255  # class 3 has no cell
    cells, alt, ref = g.class_tallies(labels, 5)
    for D in dr.DONORS:
        gt = dr.case_gt(D)
        got, again = g.match_donors(labels, 5, gt, mask), g.match_donors(labels, 5, gt, mask)
        tab1 = g.donor_tables(gt, mask)["tab1"]
        want = dn.match(alt, ref, cells, gt, None, None, mask, tab1=tab1)
        assert got["ll"].tobytes() == want["ll"].tobytes(), (D, np.abs(got["ll"] - want["ll"]).max())
        assert np.array_equal(got["best"], want["best"]) and got["margin"].tobytes() == want["margin"].tobytes()
        assert np.array_equal(got["cells"], cells) and got["best"][3] == 255 and got["margin"][3] == 0
        ll, B = dr.match_reference(alt, ref, tab1, gt, mask)
        assert dr._ratio(got["ll"], ll, B) <= 1.0
        assert all(got[k].tobytes() == again[k].tobytes() for k in got)
    g.close()


# ---- the EM state stays ----------------------------------------------------------------------------------------------------------------
@ENGINES
def test_donor_calls_leave_the_loop_alone(mods, engine):
    mask = dr.case_mask()
    x, y = _make(mods, engine), _make(mods, engine)
    want = [x.em_iteration(5.0) for _ in range(4)]
    got = []
    labels = (np.arange(dr.CASE_N) % 3).astype(np.uint8)
    for it in range(4):
        got.append(y.em_iteration(5.0))
        if it == 1:
            state = (y.excluded(), y.loci_mask())
            y.donor_tables(dr.case_gt(33), mask)
            y.donor_posteriors(dr.case_gt(33), mask=mask)
            y.match_donors(labels, 3, dr.case_gt(5), mask)
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
    gt3 = dr.case_gt(3)
    labels = (np.arange(N) % 2).astype(np.uint8)

    def refused(fn, match):
        with pytest.raises(ffi.CellectorError, match=match) as e:
            fn()
        assert e.value.status == 1

    def every_call(g, match, n=N):
        refused(lambda: g.donor_tables(gt3), match)
        refused(lambda: g.donor_posteriors(gt3), match)
        refused(lambda: g.match_donors(labels[:n], 2, gt3), match)

    g = _make(mods, 2)
    state = (g.em_iteration(5.0), g.excluded(), g.loci_mask())
    for D in (0, 65):
        every_call_gt = np.zeros((D, L), np.uint8)
        refused(lambda: g.donor_tables(every_call_gt), "1..64 are supported")
        refused(lambda: g.donor_posteriors(every_call_gt), "1..64 are supported")
        refused(lambda: g.match_donors(labels, 2, every_call_gt), "1..64 are supported")
    bad = gt3.copy()
    bad[2, 17] = 4
    for fn in (lambda: g.donor_tables(bad), lambda: g.donor_posteriors(bad), lambda: g.match_donors(labels, 2, bad)):
        refused(fn, "donor 2 at locus 17 is 4")
    for v in (0.0, 0.5, -0.1, np.nan):
        refused(lambda: g.donor_tables(gt3, err=v), "err")
        refused(lambda: g.donor_posteriors(gt3, err=v), "err")
        refused(lambda: g.match_donors(labels, 2, gt3, err=v), "err")
    for v in (1.0, -0.1, np.nan):
        refused(lambda: g.donor_tables(gt3, ambient=v), "ambient")
        refused(lambda: g.donor_posteriors(gt3, doublet_rate=v), "doublet_rate")
    for v in (1.5, -0.1, np.nan):
        refused(lambda: g.donor_posteriors(gt3, posterior_threshold=v), "posterior_threshold")
    refused(lambda: g.donor_posteriors(gt3, min_loci=0), "min_loci")
    for v in (np.nan, np.inf):
        refused(lambda: g.donor_posteriors(gt3, log_prior=np.array([0.0, v, 0.0])), r"log_prior\[1\]")
    refused(lambda: g.donor_posteriors(gt3, log_prior=np.full(3, -np.inf)), "every donor")
    anchor = np.zeros(N, np.uint8)
    anchor[9] = 3
    refused(lambda: g.donor_posteriors(gt3, anchor=anchor), "anchor of cell 9")
    refused(lambda: g.match_donors(np.full(N, 7, np.uint8), 2, gt3), "label 7")
    refused(lambda: g.match_donors(labels, 17, gt3), "1..16 are supported")
    lib = ffi.load_library()
    assert lib.cellector_donor_tables(g.h, None, 3, None, None, None, None, None) == 1 and b"null gt" in lib.cellector_last_error(g.h)
    assert lib.cellector_donor_posteriors(g.h, None, 3, *([None] * 18)) == 1 and b"null gt" in lib.cellector_last_error(g.h)
    assert lib.cellector_match_donors(g.h, None, 2, gt3.ctypes.data, 3, *([None] * 6)) == 1 and b"null labels" in lib.cellector_last_error(g.h)
    g.em_begin()
    every_call(g, "in flight")
    g.em_threshold(5.0)
    every_call(g, "in flight")
    g.em_finish()
    # the ctx is as it was: the loop goes on with the bits of an undisturbed one, and the calls work
    h = _make(mods, 2)
    assert bytes(h.em_iteration(5.0)) == bytes(state[0])
    h.em_iteration(5.0)
    assert bytes(g.em_iteration(5.0)) == bytes(h.em_iteration(5.0))
    assert np.array_equal(g.excluded(), h.excluded()) and np.array_equal(g.loci_mask(), h.loci_mask())
    h.close()
    assert g.donor_posteriors(gt3)["summary"].n_unassigned == int((np.arange(N) % 10 == 0).sum())
    g.close()
    g = mods["Cellector"](0)
    assert lib.cellector_donor_tables(g.h, gt3.ctypes.data, 3, None, None, None, None, None) == 1
    assert b"no matrix loaded" in lib.cellector_last_error(g.h)
    assert lib.cellector_donor_posteriors(g.h, gt3.ctypes.data, 3, *([None] * 18)) == 1 and b"no matrix loaded" in lib.cellector_last_error(g.h)
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
