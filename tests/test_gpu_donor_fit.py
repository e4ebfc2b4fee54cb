"""GPU: the fit of the called hypothesis (cellector_donor_moment_tables / cellector_donor_fit; csrc/kernels_donors.hip: k_donor_moments,
k_donor_fit) on both engines, against the numpy twin cellector_amd/donors.py and tests/donor_fit_reference.py.

The matrix is donor_reference.case_matrix(): 677 cells x 487 loci, rows of 0, 1 ... 9 entries around the prefetch depth (a few up to
18), repeated pairs, zero-total entries, counts to 40.  D = 1, 2, 3, 5, 9, 16, 31, 32, 33, 64: every lane width.

Where the order of the operations is fixed the claim is exact: the four moment sums equal the twin's fed the device's tables bit for
bit, the anchor's pair column is the singlet's bytes, the hypothesis and the status are cellector_donor_posteriors' own, the three
statistics are cellector_order_statistics' on the returned keys, the flags are call_z < threshold.  What passes through the device's
log, sqrt or a division is held to donor_fit_reference's derived bounds (the twin's z: 2 ulp); the flags are compared with the
reference's wherever it decides them, and the cells it does not stay under 1 % (tests/test_donor_fit_reference.py asserts the same for
the twin, on the CPU, under the same four variants).
"""
import ctypes as C

import numpy as np
import pytest

import class_reference as cr
import donor_fit_reference as fr
import donor_reference as dr
import test_gpu_tile_sweep as S
from test_donor_fit_reference import VARIANTS

pytestmark = pytest.mark.gpu

ENGINES = pytest.mark.parametrize("engine", [2, 1], ids=["tiled", "csr"])
DONORS = pytest.mark.parametrize("D", dr.DONORS)
MASKED = pytest.mark.parametrize("masked", [False, True], ids=["all-loci", "masked"])
_mat = {}


@pytest.fixture(scope="module")
def mods(oracle_lib, hip_lib_path):
    from cellector_amd import Cellector, cluster, donors, ffi
    return dict(Cellector=Cellector, ffi=ffi, cl=cluster, dn=donors)


def _make(mods, engine, case=None, **kw):
    L, N, coo = case or dr.case_matrix()
    g = mods["Cellector"](**kw) if kw else mods["Cellector"](0)
    g.set_option("engine", engine)
    g.load_coo(L, N, *S._u32(coo), 0, 0)
    assert g.dims().loci_used == L  # (min_alt = min_ref = 0: every locus is used, in order)
    return g


def _matrix(mods, masked):
    if masked not in _mat:
        L, N, coo = dr.case_matrix()
        mask = dr.case_mask() if masked else None
        _mat[masked] = (mask, mods["cl"].Matrix(L, N, coo, mask))
    return _mat[masked]


def _same(a, b):
    return all((bytes(a[k]) if k == "summary" else a[k].tobytes()) == (bytes(b[k]) if k == "summary" else b[k].tobytes()) for k in a)


def _exact_parts(mods, g, got, call, mat, gu, fit):
    """what holds bit for bit, whatever the matrix: the sums, the hypothesis, the keys' statistics, the flags, the summary"""
    dn = mods["dn"]
    n = len(got["call_z"])
    r = np.arange(n)
    E, V, PE, PV = dn.fit_sums(mat, got["mom1"], got["mom2"], gu, call["anchor"])
    for name, want in (("fit_e", E), ("fit_v", V), ("pair_e", PE), ("pair_v", PV)):
        assert got[name].tobytes() == want.tobytes(), (name, np.abs(got[name] - want).max())
    a = call["anchor"]
    assert got["pair_e"][r, a].tobytes() == got["fit_e"][r, a].tobytes() and got["pair_v"][r, a].tobytes() == got["fit_v"][r, a].tobytes()
    for gg in range(4):
        assert got["mom2"][:, 5 * gg].tobytes() == got["mom1"][:, gg].tobytes()
    # the hypothesis is the donor call's own
    st = call["status"]
    assert np.array_equal(got["status"], st)
    assert np.array_equal(got["hyp_a"], np.where(st == 1, a, call["best"]))
    assert np.array_equal(got["hyp_b"], np.where(st == 1, call["best_pair"], 255))
    # the twin: z within 2 ulp, everything decided from the device's numbers exactly
    tw = dn.fit_calls(call["ll"], call["pair_ll"], E, V, PE, PV, a, call["best"], call["best_pair"], st, **fit)
    for name in ("z", "pair_z", "call_z"):
        assert (np.abs(got[name] - tw[name]) <= 2 * np.spacing(np.abs(tw[name]))).all(), name
    assert np.array_equal(got["hyp_a"], tw["hyp_a"]) and np.array_equal(got["hyp_b"], tw["hyp_b"])
    zb, zp = got["z"][r, call["best"]], got["pair_z"][r, np.where(st == 1, call["best_pair"], 0)]
    assert got["call_z"].tobytes() == np.where(st == 255, 0.0, np.where(st == 1, zp, zb)).tobytes()
    assert (got["z"][got["fit_v"] == 0] == 0).all() and (got["pair_z"][got["pair_v"] == 0] == 0).all()
    keys = got["call_z"][st == 0]
    sm = got["summary"]
    k, mc = fit.get("iqr_multiple", 3.0), fit.get("min_cells", 8)
    assert sm.n_keys == len(keys)
    if len(keys) >= mc:
        want = g.order_statistics(keys, k)
        assert np.array([sm.median, sm.iqr, sm.threshold]).tobytes() == np.asarray(want, np.float64).tobytes()
        assert np.asarray(dn.order_statistics(keys, k)).tobytes() == np.asarray(want, np.float64).tobytes()
    else:
        assert np.isnan(sm.median) and np.isnan(sm.iqr) and sm.threshold == -np.inf
    flags = ((st != 255) & (got["call_z"] < sm.threshold)).astype(np.uint8)
    assert np.array_equal(got["unmatched"], flags)
    assert [sm.n_unmatched, sm.n_unmatched_singlet, sm.n_unmatched_doublet, sm.n_unmatched_ambiguous] == \
        [int(flags.sum())] + [int((flags[st == v]).sum()) for v in (0, 1, 2)]
    assert list(sm.donor_unmatched) == np.bincount(call["best"][flags != 0], minlength=64).tolist()


def _check(mods, g, D, masked, lp, anchor, prm, fit):
    L, N, coo = dr.case_matrix()
    A, R = dr.totals(L, coo)
    gt = dr.case_gt(D)
    mask, mat = _matrix(mods, masked)
    got = g.donor_fit(gt, lp, anchor, mask, tables=True, **prm, **fit)
    call = g.donor_posteriors(gt, lp, anchor, mask, tables=True, **prm)
    p = dr.params(**prm)
    res = fr.compare_moms(A, R, p["err"], p["ambient"], mask, got["mom1"], got["mom2"])
    assert max(res.values()) <= 1.0, res
    if mask is not None:
        assert (got["mom1"][mask == 0] == 0).all() and (got["mom2"][mask == 0] == 0).all()
    _exact_parts(mods, g, got, call, mat, gt.T, fit)
    refcall = dr.reference(L, N, coo, gt, call["tab1"], call["tab2"], lp, call["anchor"], mask, **prm)
    ref = fr.reference(L, N, coo, gt, refcall, got["mom1"], got["mom2"], mask, **fit)
    res2, undecided = fr.compare(ref, got)
    print(D, masked, prm, fit, {k: round(v, 3) for k, v in {**res, **res2}.items()}, "undecided", int(undecided.sum()), "keys",
          got["summary"].n_keys, "threshold", got["summary"].threshold, "unmatched", got["summary"].n_unmatched)
    assert max(res2.values()) <= 1.0, res2
    assert undecided.sum() < 0.01 * N, int(undecided.sum())
    assert _same(got, g.donor_fit(gt, lp, anchor, mask, tables=True, **prm, **fit))
    return got, call


@ENGINES
@MASKED
@DONORS
def test_fit_under_the_four_variants(mods, D, masked, engine):
    """the (prior, anchor) variants of test_gpu_donors.py and the one with hundreds of keys at every D (test_donor_fit_reference.VARIANTS)"""
    g = _make(mods, engine)
    for prior, anchor_kind, prm, fit in VARIANTS:
        lp = dr.case_prior(D) if prior else None
        anchor = None
        if anchor_kind == "worst":
            first = g.donor_posteriors(dr.case_gt(D), lp, None, _matrix(mods, masked)[0], **prm)
            anchor = np.argmin(np.where(np.isfinite(lp)[None, :], first["ll"] + lp[None, :], np.inf), axis=1).astype(np.uint8)
        elif anchor_kind == "mod":
            anchor = (np.arange(dr.CASE_N) % D).astype(np.uint8)
        got, call = _check(mods, g, D, masked, lp, anchor, prm, fit)
        empty = call["n_entries"] == 0
        assert empty.any() and (got["fit_v"][empty] == 0).all() and (got["z"][empty] == 0).all() and (got["unmatched"][empty] == 0).all()
        if D == 1:
            assert (got["hyp_b"] == 255).all() and (got["hyp_a"] == 0).all() and (got["pair_z"].tobytes() == got["z"].tobytes())
    g.close()


@ENGINES
def test_moment_tables_alone(mods, engine):
    L, N, coo = dr.case_matrix()
    A, R = dr.totals(L, coo)
    g = _make(mods, engine)
    for mask, prm in ((None, {}), (dr.case_mask(), dict(err=0.2, ambient=0.0)), (dr.case_mask(), dict(err=1e-6, ambient=0.9))):
        mom1, mom2 = g.donor_moment_tables(mask, **prm)
        p = dr.params(**prm)
        res = fr.compare_moms(A, R, p["err"], p["ambient"], mask, mom1, mom2)
        print(prm, res)
        assert max(res.values()) <= 1.0, res
        for gg in range(4):
            assert mom2[:, 5 * gg].tobytes() == mom1[:, gg].tobytes()
        got = g.donor_fit(dr.case_gt(3), mask=mask, tables=True, **prm)
        assert got["mom1"].tobytes() == mom1.tobytes() and got["mom2"].tobytes() == mom2.tobytes()
        # the donor call's tables stay the same bytes beside the fit
        t, c = g.donor_tables(dr.case_gt(3), mask, **prm), g.donor_posteriors(dr.case_gt(3), mask=mask, tables=True, **prm)
        assert t["tab1"].tobytes() == c["tab1"].tobytes() and t["tab2"].tobytes() == c["tab2"].tobytes()
    g.close()


# ---- edges ------------------------------------------------------------------------------------------------------------------------
@ENGINES
def test_edges_of_the_key_set(mods, engine):
    g = _make(mods, engine)
    N, L = dr.CASE_N, dr.CASE_L
    many = dict(doublet_rate=0.02, posterior_threshold=0.5)
    gt = dr.case_gt(5)
    # a mask that leaves some cells without entries: V = 0, z = 0, never flagged
    lo, ce = dr.case_matrix()[2][:2]
    mask = np.ones(L, np.uint8)
    mask[lo[np.isin(ce, np.arange(1, N, 25))]] = 0
    got, call = g.donor_fit(gt, mask=mask, **many), g.donor_posteriors(gt, mask=mask, **many)
    bare = call["n_entries"] == 0
    assert bare.sum() > (np.arange(N) % 10 == 0).sum() + 20 and (got["fit_v"][bare] == 0).all() and (got["z"][bare] == 0).all() and (got["pair_z"][bare] == 0).all()
    assert (got["call_z"][bare] == 0).all() and (got["unmatched"][bare] == 0).all() and (got["status"][bare] == 255).all()
    assert got["summary"].n_keys >= 8 and np.isfinite(got["summary"].threshold)
    # an all-masked call: no keys, threshold -inf
    got = g.donor_fit(gt, mask=np.zeros(L, np.uint8), tables=True, **many)
    sm = got["summary"]
    assert sm.n_keys == 0 and sm.threshold == -np.inf and np.isnan(sm.median) and sm.n_unmatched == 0
    assert not got["unmatched"].any() and (got["call_z"] == 0).all() and (got["mom1"] == 0).all() and (got["mom2"] == 0).all()
    assert (got["status"] == 255).all() and (got["hyp_b"] == 255).all()
    # fewer status-0 cells than min_cells: no threshold; exactly min_cells: one
    keys = int(g.donor_fit(gt, **many)["summary"].n_keys)
    assert keys >= 8
    got = g.donor_fit(gt, min_cells=keys + 1, **many)
    assert got["summary"].n_keys == keys and got["summary"].threshold == -np.inf and not got["unmatched"].any()
    got = g.donor_fit(gt, min_cells=keys, **many)
    assert np.isfinite(got["summary"].threshold)
    # iqr_multiple 0: the threshold is the lower quartile itself, and about a quarter of the keys lie below it
    got = g.donor_fit(gt, iqr_multiple=0.0, **many)
    sm = got["summary"]
    k = got["call_z"][got["status"] == 0]
    want = g.order_statistics(k, 0.0)
    assert sm.threshold == want[2] and sm.iqr == want[1] and 0.2 * keys < sm.n_unmatched_singlet < 0.3 * keys
    assert np.array_equal(got["unmatched"], ((got["status"] != 255) & (got["call_z"] < sm.threshold)).astype(np.uint8))
    # min_cells 4, the smallest
    assert np.isfinite(g.donor_fit(gt, min_cells=4, **many)["summary"].threshold)
    g.close()


# ---- the ctx stays ------------------------------------------------------------------------------------------------------------------
@ENGINES
def test_fit_leaves_the_donor_call_and_the_loop_alone(mods, engine):
    mask = dr.case_mask()
    x, y = _make(mods, engine), _make(mods, engine)
    want = [x.em_iteration(5.0) for _ in range(4)]
    got = []
    for it in range(4):
        got.append(y.em_iteration(5.0))
        if it == 1:
            state = (y.excluded(), y.loci_mask())
            before = y.donor_posteriors(dr.case_gt(33), mask=mask, tables=True)
            y.donor_fit(dr.case_gt(33), mask=mask, doublet_rate=0.02, posterior_threshold=0.5)
            y.donor_moment_tables(mask)
            assert _same(before, y.donor_posteriors(dr.case_gt(33), mask=mask, tables=True))
            assert np.array_equal(y.excluded(), state[0]) and np.array_equal(y.loci_mask(), state[1])
    assert [bytes(s) for s in got] == [bytes(s) for s in want], engine
    assert np.array_equal(x.excluded(), y.excluded()) and np.array_equal(x.loci_mask(), y.loci_mask())
    for k, v in x.cell_outputs().items():
        assert v.tobytes() == y.cell_outputs()[k].tobytes(), k
    x.close(); y.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(mods):
    ffi = mods["ffi"]
    L, N, coo = dr.case_matrix()
    gt3 = dr.case_gt(3)

    def refused(fn, match):
        with pytest.raises(ffi.CellectorError, match=match) as e:
            fn()
        assert e.value.status == 1

    g = _make(mods, 2)
    state = g.em_iteration(5.0)
    refused(lambda: g.donor_fit(gt3, iqr_multiple=np.nan), "iqr_multiple")
    refused(lambda: g.donor_fit(gt3, iqr_multiple=-0.5), "iqr_multiple")
    refused(lambda: g.donor_fit(gt3, min_cells=3), "min_cells")
    bad = gt3.copy()
    bad[2, 17] = 4
    refused(lambda: g.donor_fit(bad), "donor 2 at locus 17 is 4")
    for D in (0, 65):
        refused(lambda: g.donor_fit(np.zeros((D, L), np.uint8)), "1..64 are supported")
    for v in (0.0, 0.5, np.nan):
        refused(lambda: g.donor_fit(gt3, err=v), "err")
        refused(lambda: g.donor_moment_tables(err=v), "err")
    for v in (1.0, -0.1, np.nan):
        refused(lambda: g.donor_fit(gt3, ambient=v), "ambient")
        refused(lambda: g.donor_moment_tables(ambient=v), "ambient")
        refused(lambda: g.donor_fit(gt3, doublet_rate=v), "doublet_rate")
    refused(lambda: g.donor_fit(gt3, posterior_threshold=1.5), "posterior_threshold")
    refused(lambda: g.donor_fit(gt3, min_loci=0), "min_loci")
    refused(lambda: g.donor_fit(gt3, log_prior=np.array([0.0, np.nan, 0.0])), r"log_prior\[1\]")
    refused(lambda: g.donor_fit(gt3, log_prior=np.full(3, -np.inf)), "every donor")
    anchor = np.zeros(N, np.uint8)
    anchor[9] = 3
    refused(lambda: g.donor_fit(gt3, anchor=anchor), "anchor of cell 9")
    with pytest.raises(TypeError):
        g.donor_fit(gt3, no_such_parameter=1)
    # nothing is written by a refused call
    lib = ffi.load_library()
    fp = ffi.DonorFitParams(np.nan, 8)
    cz, um = np.full(N, 7.0), np.full(N, 9, np.uint8)
    sm = ffi.DonorFitSummary()
    sm.n_keys = 77
    args = [g.h, gt3.ctypes.data, 3, None, C.byref(fp), None, None, None] + [None] * 6 + [cz.ctypes.data, None, None, None, um.ctypes.data,
                                                                                        C.byref(sm), None, None]
    assert lib.cellector_donor_fit(*args) == 1 and b"iqr_multiple" in lib.cellector_last_error(g.h)
    assert (cz == 7.0).all() and (um == 9).all() and sm.n_keys == 77
    assert lib.cellector_donor_fit(g.h, None, 3, *([None] * 19)) == 1 and b"null gt" in lib.cellector_last_error(g.h)
    g.em_begin()
    refused(lambda: g.donor_fit(gt3), "in flight")
    refused(lambda: g.donor_moment_tables(), "in flight")
    g.em_threshold(5.0)
    refused(lambda: g.donor_fit(gt3), "in flight")
    g.em_finish()
    # the ctx is as it was: the loop goes on with the bits of an undisturbed one, and the call works
    h = _make(mods, 2)
    assert bytes(h.em_iteration(5.0)) == bytes(state)
    h.em_iteration(5.0)
    assert bytes(g.em_iteration(5.0)) == bytes(h.em_iteration(5.0))
    h.close()
    assert g.donor_fit(gt3)["summary"].n_keys == g.donor_posteriors(gt3)["summary"].n_singlet
    g.close()
    g = mods["Cellector"](0)
    assert lib.cellector_donor_fit(g.h, gt3.ctypes.data, 3, *([None] * 19)) == 1 and b"no matrix loaded" in lib.cellector_last_error(g.h)
    assert lib.cellector_donor_moment_tables(g.h, None, None, None, None) == 1 and b"no matrix loaded" in lib.cellector_last_error(g.h)
    g.close()
    m = mods["Cellector"](devices=[0, 0, 0])  # three logical shards
    m.load_coo(L, N, *S._u32(coo), 0, 0)
    refused(lambda: m.donor_fit(gt3), "single-device")
    refused(lambda: m.donor_moment_tables(), "single-device")
    assert m.em_iteration(5.0) is not None
    m.close()
    g = mods["Cellector"](0)
    g.set_shard(10, 40)
    g.load_coo(L, N, *S._u32(coo), 0, 0)
    refused(lambda: g.donor_fit(gt3), "set_shard")
    g.close()


# ---- recovery ---------------------------------------------------------------------------------------------------------------------
@ENGINES
def test_the_device_flags_the_cells_of_a_withheld_donor(mods, engine):
    """the planted pool (seed 5) with donor 1 taken out of gt: the device's flags are the reference's outside its undecided set"""
    L, N, coo, gt, truth, par = dr.planted_pool(5)
    g = _make(mods, engine, (L, N, coo))
    gw = gt[[0, 2, 3]]
    got = g.donor_fit(gw, tables=True)
    call = g.donor_posteriors(gw, tables=True)
    _exact_parts(mods, g, got, call, mods["cl"].Matrix(L, N, coo), gw.T, {})
    refcall = dr.reference(L, N, coo, gw, call["tab1"], call["tab2"], None, call["anchor"])
    ref = fr.reference(L, N, coo, gw, refcall, got["mom1"], got["mom2"])
    res, undecided = fr.compare(ref, got)
    print({k: round(v, 3) for k, v in res.items()}, "undecided", int(undecided.sum()), "threshold", got["summary"].threshold)
    assert max(res.values()) <= 1.0, res
    assert np.array_equal(got["unmatched"][ref["flag_ok"]], ref["unmatched"][ref["flag_ok"]])
    single = np.arange(cr.MIX_N)  # (the planted singlets; the 60 doublets stand behind them)
    lost = single[truth[single] == 1]
    assert ref["flag_ok"][single].all() and got["unmatched"][lost].all() and not got["unmatched"][np.setdiff1d(single, lost)].any()
    g.close()
