"""GPU: donor panels (cellector_donor_panel / cellector_match_donors_panel; csrc/kernels_donor_panel.hip) on both engines, against the
numpy twin cellector_amd/donors.py (panel_posteriors), tests/donor_panel_reference.py and the 64-donor calls on the same ctx.

The matrix is donor_reference.case_matrix() (677 cells x 487 loci, rows of 0 ... 18 entries) and, for the edges of a wave's chunk of 64
entries, cluster_reference.hand_matrix() (rows of 0, 1, 63, 64, 65 and 1100 entries, repeated pairs, counts of 65535).  D = 1, 2, 33,
64, 65, 96, 127, 128, 129, 1000, 2048, 2049, 4096: every Q = 1 ... 64 donors per lane, the first donor past a lane's block and past a
packed word; M = 1, 2, 8, 33, 64, M > D included; a donor and a locus without any call.

Where the order of the operations is fixed the claim is exact (tobytes): packed against the definition, ll, cand_ll and cand_pair_ll
against the twin fed the device's tables, cand / best / second / anchor against the twin, every common output against
cellector_donor_posteriors where D <= 64 and the shortlist holds all donors, and the columns of ll against cellector_donor_posteriors on
64-donor subsets of a 1000- and a 4096-donor panel.  What passes through the device's exp is held to donor_panel_reference's derived
bounds; status and best_pair are compared exactly where the reference decides them, and the cells it does not stay under 1 %
(tests/test_donor_panel_reference.py asserts the same share for the twin, on the CPU).
"""
import numpy as np
import pytest

import cluster_reference as kr
import donor_panel_reference as pn
import donor_reference as dr
import test_gpu_tile_sweep as S

pytestmark = pytest.mark.gpu

ENGINES = pytest.mark.parametrize("engine", [2, 1], ids=["tiled", "csr"])
_memo = {}


@pytest.fixture(scope="module")
def mods(oracle_lib, hip_lib_path):
    from cellector_amd import Cellector, cluster, donors, ffi
    yield dict(Cellector=Cellector, ffi=ffi, cl=cluster, dn=donors)
    for k in [k for k in _memo if k[0] == "ctx"]:
        _memo.pop(k).close()


def _once(key, fn):
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def _matrix(name):
    return dr.case_matrix() if name == "case" else kr.hand_matrix()


def _load(mods, engine, name):
    L, N, coo = _matrix(name)
    g = mods["Cellector"](0)
    g.set_option("engine", engine)
    g.load_coo(L, N, *S._u32(coo), 0, 0)
    assert g.dims().loci_used == L and g.dims().nnz_used == len(coo[0])  # (min_alt = min_ref = 0: every locus is used, in order)
    return g


def _ctx(mods, engine, name="case"):
    """one ctx per (engine, matrix) for the module: the panel calls leave it as it was (asserted below)"""
    return _once(("ctx", engine, name), lambda: _load(mods, engine, name))


def _gt(name, D):
    return dr.case_gt(D, _matrix(name)[0])


def _mask(name, kind):
    L = _matrix(name)[0]
    return None if kind is None else dr.case_mask(L) if kind == "random" else np.zeros(L, np.uint8)


def _twin_matrix(mods, name, kind):
    L, N, coo = _matrix(name)
    return _once(("mat", name, kind), lambda: mods["cl"].Matrix(L, N, coo, _mask(name, kind)))


def _shared(mods, name, D, kind, lp_key, lp, got, reference):
    """the twin's singlet sums and (where asked for) the reference's singlets for the device's tables, kept for the latest (matrix, D,
    mask, prior)"""
    key = (name, D, kind, lp_key, got["tab1"].tobytes(), got["tab2"].tobytes())
    if _memo.get("shared_key") != key:
        _memo["shared"] = [mods["dn"].singlet_sums(_twin_matrix(mods, name, kind), got["tab1"], _gt(name, D).T), None]
        _memo["shared_key"] = key
    if reference and _memo["shared"][1] is None:
        L, N, coo = _matrix(name)
        _memo["shared"][1] = pn.singlets(L, N, coo, _gt(name, D), got["tab1"], lp, _mask(name, kind), got["tab2"])
    return _memo["shared"]


def _same_bytes(a, b):
    for k in a:
        assert (bytes(a[k]) if k == "summary" else a[k].tobytes()) == (bytes(b[k]) if k == "summary" else b[k].tobytes()), k


def _check(mods, g, D, M, name="case", kind=None, lp_key=None, lp=None, anchor=None, reference=True, **prm):
    L, N, coo = _matrix(name)
    gt, mask, dn = _gt(name, D), _mask(name, kind), mods["dn"]
    got = g.donor_panel(gt, M, lp, anchor, mask, ll=True, tables=True, **prm)
    Ma = min(M, D)
    assert got["cand"].shape == (N, Ma) and got["ll"].shape == (N, D) and got["packed"].shape == (L, (D + 31) // 32)
    if name == "case" or D <= 65:  # (the words do not depend on the matrix: the long matrix checks them at one D)
        assert got["packed"].tobytes() == _once(("packed", name, D), lambda: dr.pack_reference(gt)).tobytes()
    s, ref_s = _shared(mods, name, D, kind, lp_key, lp, got, reference)
    assert got["ll"].tobytes() == s.tobytes(), np.abs(got["ll"] - s).max()
    twin = dn.panel_posteriors(_twin_matrix(mods, name, kind), gt, None, None, M, lp, anchor, got["tab1"], got["tab2"], s=s, **prm)
    for k in ("cand", "best", "second", "anchor", "n_entries"):
        assert got[k].dtype == twin[k].dtype and np.array_equal(got[k], twin[k]), k
    for k in ("cand_ll", "cand_pair_ll"):
        assert got[k].tobytes() == twin[k].tobytes(), (k, np.abs(got[k] - twin[k]).max())
    r = np.arange(N)
    assert got["cand_ll"].tobytes() == got["ll"][r[:, None], got["cand"]].tobytes()
    assert np.array_equal(got["anchor"], got["best"] if anchor is None else anchor)
    at = got["cand"] == got["anchor"][:, None]
    assert got["cand_pair_ll"][at].tobytes() == got["cand_ll"][at].tobytes() and (got["cand_pair_posterior"][at] == 0).all()
    if anchor is None:
        assert at.any(axis=1).all()
    if reference:
        ref = pn.chain(ref_s, got["tab2"], M, got["anchor"], got["cand"], **prm)
        res, undecided = pn.compare(ref, got)
        print(name, D, M, kind, lp_key, prm, {k: round(v, 3) for k, v in res.items()}, "undecided", int(undecided.sum()))
        assert max(res.values()) <= 1.0, res
        assert undecided.sum() < 0.01 * N, int(undecided.sum())
    sm, st = got["summary"], got["status"]
    assert [sm.n_singlet, sm.n_doublet, sm.n_ambiguous, sm.n_unassigned] == [int((st == v).sum()) for v in (0, 1, 2, 255)]
    assert got["donor_cells"].dtype == np.uint64 and np.array_equal(got["donor_cells"], np.bincount(got["best"][st == 0], minlength=D))
    assert sm.n_present == int((got["donor_cells"] > 0).sum())
    assert np.array_equal(dn.panel_present(got), np.flatnonzero(got["donor_cells"]))
    if D == 1:
        assert (got["second"] == 65535).all() and (got["best_pair"] == 65535).all() and (got["doublet_posterior"] == 0).all()
    if Ma == 1 and anchor is None:
        assert (got["best_pair"] == 65535).all() and (got["doublet_posterior"] == 0).all()
    return got


# ---- every (D, M) ----------------------------------------------------------------------------------------------------------------------
@ENGINES
@pytest.mark.parametrize("M", pn.SHORTLISTS)
@pytest.mark.parametrize("D", pn.DONORS)
def test_flat_prior_own_anchor(mods, D, M, engine):
    g = _ctx(mods, engine)
    got = _check(mods, g, D, M)
    empty = got["n_entries"] == 0
    assert empty.any() and (got["ll"][empty] == 0).all() and (got["status"][empty] == 255).all()
    if M == 8:
        _same_bytes(got, g.donor_panel(_gt("case", D), M, ll=True, tables=True))  # a second call returns the same bytes


# ---- equality 1: the 64-donor call -----------------------------------------------------------------------------------------------------
@ENGINES
@pytest.mark.parametrize("D", [1, 2, 33, 64])
def test_equals_donor_posteriors_where_the_shortlist_holds_every_donor(mods, D, engine):
    g = _ctx(mods, engine)
    gt, N = dr.case_gt(D), dr.CASE_N
    for mask, lp, anchor, prm in ((None, None, None, {}),
                                  (dr.case_mask(), dr.case_prior(D), np.arange(N) % D, dict(doublet_rate=0.3, posterior_threshold=0.9, min_loci=3)),
                                  (None, None, None, dict(doublet_rate=0.0))):
        want = g.donor_posteriors(gt, lp, None if anchor is None else anchor.astype(np.uint8), mask, tables=True, **prm)
        got = g.donor_panel(gt, 64, lp, None if anchor is None else anchor.astype(np.uint16), mask, ll=True, tables=True, **prm)
        assert np.array_equal(got["cand"], np.tile(np.arange(D, dtype=np.uint16), (N, 1)))
        for a, b in (("ll", "ll"), ("cand_ll", "ll"), ("cand_pair_ll", "pair_ll"), ("cand_posterior", "posterior"),
                     ("cand_pair_posterior", "pair_posterior"), ("doublet_posterior", "doublet_posterior"), ("tab1", "tab1"),
                     ("tab2", "tab2"), ("status", "status"), ("n_entries", "n_entries")):
            assert got[a].tobytes() == want[b].tobytes(), (a, D, prm)
        assert got["best_posterior"].tobytes() == want["posterior"][np.arange(N), want["best"]].tobytes()
        for k in ("best", "second", "best_pair", "anchor"):
            assert np.array_equal(got[k], np.where(want[k] == 255, 65535, want[k].astype(np.uint16))), (k, D, prm)
        sm = want["summary"]
        assert np.array_equal(got["donor_cells"], np.array(sm.donor_cells[:D], np.uint64))
        assert [got["summary"].n_singlet, got["summary"].n_doublet] == [sm.n_singlet, sm.n_doublet]
        assert got["packed"].tobytes() == g.donor_tables(gt, mask)["packed"].tobytes()


# ---- equality 2: a column depends on its donor alone -----------------------------------------------------------------------------------
@ENGINES
@pytest.mark.parametrize("D", [1000, 4096])
def test_columns_equal_the_64_donor_calls_on_subsets(mods, D, engine):
    g = _ctx(mods, engine)
    gt, N = dr.case_gt(D), dr.CASE_N
    mask = dr.case_mask()
    labels = (np.arange(N) % 5).astype(np.uint8)
    labels[::7] = 255
    labels[labels == 3] = 255  # class 3 has no cell
    got = g.donor_panel(gt, 8, mask=mask, ll=True, tables=True)
    m = g.match_donors_panel(labels, 5, gt, mask)
    cells, alt, ref = g.class_tallies(labels, 5)
    want = mods["dn"].panel_match(alt, ref, cells, gt, None, None, mask, tab1=got["tab1"])  # (every locus is used, in order)
    assert m["ll"].tobytes() == want["ll"].tobytes(), np.abs(m["ll"] - want["ll"]).max()
    assert m["best"].dtype == want["best"].dtype and np.array_equal(m["best"], want["best"])
    assert m["margin"].tobytes() == want["margin"].tobytes() and np.array_equal(m["cells"], cells)
    assert m["ll"].shape == (5, D) and m["best"].dtype == np.uint16 and m["best"][3] == 65535 and m["margin"][3] == 0
    live = [0, 1, 2, 4]
    assert np.array_equal(m["best"][live], np.argmax(m["ll"][live], axis=1))
    top2 = np.sort(m["ll"][live], axis=1)[:, -2:]
    assert m["margin"][live].tobytes() == (top2[:, 1] - top2[:, 0]).tobytes()
    rng = np.random.default_rng(D)
    for _ in range(3):
        sub = rng.choice(D, 64, replace=False)  # (in any order: the column does not depend on where the donor stands)
        small = g.donor_posteriors(gt[sub], mask=mask)
        assert got["ll"][:, sub].tobytes() == small["ll"].tobytes()
        ms = g.match_donors(labels, 5, gt[sub], mask)
        assert m["ll"][:, sub].tobytes() == ms["ll"].tobytes() and np.array_equal(m["cells"], ms["cells"])
    _same_bytes(m, g.match_donors_panel(labels, 5, gt, mask))


# ---- masks, anchors, priors, rates ------------------------------------------------------------------------------------------------------
@ENGINES
@pytest.mark.parametrize("D", [65, 1000])
def test_masks_given_anchors_priors_and_rates(mods, D, engine):
    g = _ctx(mods, engine)
    N, M = dr.CASE_N, 8
    first = _check(mods, g, D, M, kind="random", doublet_rate=0.3, posterior_threshold=0.9, min_loci=3)
    assert (first["status"][first["n_entries"] < 3] == 255).all() and (first["status"][first["n_entries"] >= 3] != 255).all()
    # every cell's WORST donor: an anchor outside the shortlist
    worst = np.argmin(first["ll"], axis=1).astype(np.uint16)
    got = _check(mods, g, D, M, kind="random", anchor=worst)
    assert (~(got["cand"] == worst[:, None]).any(axis=1)).sum() > N // 2
    _check(mods, g, D, M, kind="random", anchor=(np.arange(N) % D).astype(np.uint16), doublet_rate=0.0)
    # a prior with three donors ruled out, then with all but five: the shortlist has to take donors at -inf
    lp = pn.case_prior(D, 3)
    got = _check(mods, g, D, M, kind="random", lp_key="3", lp=lp, doublet_rate=0.1)
    assert (got["cand_posterior"][np.isneginf(lp)[got["cand"]]] == 0).all() and np.isfinite(lp[got["best"]]).all()
    lp = pn.case_prior(D, D - 5)
    got = _check(mods, g, D, M, kind="random", lp_key="D-5", lp=lp, doublet_rate=0.3)
    assert np.isneginf(lp[got["cand"]]).sum(axis=1).min() >= M - 5 and np.isfinite(lp[got["best"]]).all()


@ENGINES
def test_a_mask_of_zeros(mods, engine):
    """no locus left: every sum 0, every cell unassigned at min_loci 1, the shortlist the first M donors"""
    g = _ctx(mods, engine)
    for D in (1, 65, 1000):
        got = _check(mods, g, D, 8, kind="zeros", reference=False)
        assert (got["ll"] == 0).all() and (got["cand_pair_ll"] == 0).all() and (got["n_entries"] == 0).all()
        assert (got["status"] == 255).all() and got["summary"].n_unassigned == dr.CASE_N and got["summary"].n_present == 0
        assert (got["tab1"] == 0).all() and (got["best"] == 0).all() and (got["cand"] == np.arange(min(8, D))).all()
        m = g.match_donors_panel((np.arange(dr.CASE_N) % 2).astype(np.uint8), 2, dr.case_gt(D), np.zeros(dr.CASE_L, np.uint8))
        assert (m["ll"] == 0).all() and (m["best"] == 0).all()


# ---- the edges of a wave's chunk of entries ---------------------------------------------------------------------------------------------
@ENGINES
@pytest.mark.parametrize("D", [65, 1000, 4096])
def test_rows_of_0_1_63_64_65_and_1100_entries(mods, D, engine):
    g = _ctx(mods, engine, "hand")
    got = _check(mods, g, D, 8, name="hand")
    assert got["n_entries"][[0, 1, 2, 3, 4, 5, 7]].tolist() == [0, 1, 63, 64, 65, 1100, 0]


# ---- the EM state stays; refusals -------------------------------------------------------------------------------------------------------
@ENGINES
def test_panel_calls_leave_the_loop_alone(mods, engine):
    x, y = _load(mods, engine, "case"), _load(mods, engine, "case")
    want = [x.em_iteration(5.0) for _ in range(4)]
    got = []
    labels = (np.arange(dr.CASE_N) % 3).astype(np.uint8)
    for it in range(4):
        got.append(y.em_iteration(5.0))
        if it == 1:
            state = (y.excluded(), y.loci_mask())
            y.donor_panel(dr.case_gt(129), mask=dr.case_mask())
            y.match_donors_panel(labels, 3, dr.case_gt(129), dr.case_mask())
            assert np.array_equal(y.excluded(), state[0]) and np.array_equal(y.loci_mask(), state[1])
    assert [bytes(s) for s in got] == [bytes(s) for s in want], engine
    assert np.array_equal(x.excluded(), y.excluded()) and np.array_equal(x.loci_mask(), y.loci_mask())
    for k, v in x.cell_outputs().items():
        assert v.tobytes() == y.cell_outputs()[k].tobytes(), k
    x.close(); y.close()


def test_refusals(mods):
    ffi = mods["ffi"]
    L, N, coo = dr.case_matrix()
    gt = dr.case_gt(70)
    labels = (np.arange(N) % 2).astype(np.uint8)

    def refused(fn, match):
        with pytest.raises(ffi.CellectorError, match=match) as e:
            fn()
        assert e.value.status == 1

    def every_call(g, match, n=N):
        refused(lambda: g.donor_panel(gt), match)
        refused(lambda: g.match_donors_panel(labels[:n], 2, gt), match)

    g, h = _load(mods, 2, "case"), _load(mods, 2, "case")
    state = g.em_iteration(5.0)
    assert bytes(h.em_iteration(5.0)) == bytes(state)
    for D in (0, 4097):
        big = np.zeros((D, L), np.uint8)
        refused(lambda: g.donor_panel(big), "1..4096 are supported")
        refused(lambda: g.match_donors_panel(labels, 2, big), "1..4096 are supported")
    refused(lambda: g.donor_posteriors(np.zeros((65, L), np.uint8)), "1..64 are supported")  # (the 64-donor call is as it was)
    for m in (0, 65):
        refused(lambda: g.donor_panel(gt, m), "shortlist of %d" % m)
    bad = gt.copy()
    bad[66, 17] = 4
    refused(lambda: g.donor_panel(bad), "donor 66 at locus 17 is 4")
    refused(lambda: g.match_donors_panel(labels, 2, bad), "donor 66 at locus 17 is 4")
    for v in (0.0, 0.5, np.nan):
        refused(lambda: g.donor_panel(gt, err=v), "err")
        refused(lambda: g.match_donors_panel(labels, 2, gt, err=v), "err")
    refused(lambda: g.donor_panel(gt, ambient=1.0), "ambient")
    refused(lambda: g.donor_panel(gt, doublet_rate=1.0), "doublet_rate")
    refused(lambda: g.donor_panel(gt, posterior_threshold=1.5), "posterior_threshold")
    refused(lambda: g.donor_panel(gt, min_loci=0), "min_loci")
    lp = np.zeros(70)
    lp[69] = np.nan
    refused(lambda: g.donor_panel(gt, log_prior=lp), r"log_prior\[69\]")
    refused(lambda: g.donor_panel(gt, log_prior=np.full(70, -np.inf)), "every donor")
    anchor = np.zeros(N, np.uint16)
    anchor[9] = 70
    refused(lambda: g.donor_panel(gt, anchor=anchor), "anchor of cell 9 is 70")
    refused(lambda: g.match_donors_panel(np.full(N, 7, np.uint8), 2, gt), "label 7")
    refused(lambda: g.match_donors_panel(labels, 17, gt), "1..16 are supported")
    lib = ffi.load_library()
    assert lib.cellector_donor_panel(g.h, None, 70, 8, *([None] * 23)) == 1 and b"null gt" in lib.cellector_last_error(g.h)
    assert lib.cellector_match_donors_panel(g.h, None, 2, gt.ctypes.data, 70, *([None] * 6)) == 1
    assert b"null labels" in lib.cellector_last_error(g.h)
    g.em_begin()
    every_call(g, "in flight")
    g.em_threshold(5.0)
    every_call(g, "in flight")
    g.em_finish()
    # the ctx is as it was: the loop goes on with the bits of an undisturbed one, and the calls work
    h.em_iteration(5.0)
    assert bytes(g.em_iteration(5.0)) == bytes(h.em_iteration(5.0))
    assert np.array_equal(g.excluded(), h.excluded()) and np.array_equal(g.loci_mask(), h.loci_mask())
    h.close()
    assert g.donor_panel(gt)["summary"].n_unassigned == int((np.arange(N) % 10 == 0).sum())
    g.close()
    g = mods["Cellector"](0)
    assert lib.cellector_donor_panel(g.h, gt.ctypes.data, 70, 8, *([None] * 23)) == 1 and b"no matrix loaded" in lib.cellector_last_error(g.h)
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
