"""GPU: ambient fraction estimation (cellector_ambient_tables / cellector_ambient_profile / cellector_estimate_ambient;
csrc/kernels_ambient.hip) on both engines, against the donor calls, the numpy twin cellector_amd/ambient.py and
tests/ambient_reference.py.

The matrix is donor_reference.case_matrix(): 677 cells x 487 loci, rows of 0 ... 18 entries around the prefetch depth, repeated pairs, a
cell count no rows-per-wave divides.  G = 4, 5, 8, 15, 16, 17, 32: every lanes-per-cell width of the cell pass and both sides of each;
S = 1, 3, 33, 64: one and two packed words; NULL and case_mask(); assign with 255s, with a source that has no cell, with every cell
255; a caller's grid of unequal steps.

Where the order of the operations is fixed the claim is exact (tobytes): a grid point's table rows are cellector_donor_tables' tab1 at
that ambient fraction, a grid point's column of ll is cellector_donor_posteriors' ll[c][assign[c]] there, and ll, the folds, cell_rho
and the summary are the twin's fed the device's tables.  What passes through a square root (the se fields) is held to 2 ulp of the
twin; what passes through the device's log to ambient_reference's derived bounds.
"""
import numpy as np
import pytest

import ambient_reference as ar
import donor_reference as dr
import test_gpu_tile_sweep as S_

pytestmark = pytest.mark.gpu

ENGINES = pytest.mark.parametrize("engine", [2, 1], ids=["tiled", "csr"])
MASKED = pytest.mark.parametrize("masked", [False, True], ids=["all-loci", "masked"])
SOURCES = pytest.mark.parametrize("S", ar.SOURCES)
KIND = {1: "mixed", 3: "hole", 33: "mixed", 64: "hole"}
_mat = {}


@pytest.fixture(scope="module")
def mods(oracle_lib, hip_lib_path):
    from cellector_amd import Cellector, ambient, cluster, ffi
    return dict(Cellector=Cellector, ffi=ffi, cl=cluster, am=ambient)


def _make(mods, engine, case=None):
    L, N, coo = case or dr.case_matrix()
    g = mods["Cellector"](0)
    g.set_option("engine", engine)
    g.load_coo(L, N, *S_._u32(coo), 0, 0)
    assert g.dims().loci_used == L and g.dims().nnz_used == len(coo[0])  # (min_alt = min_ref = 0: every locus is used)
    assert np.array_equal(g.locus_ids(), np.arange(L, dtype=np.uint64))
    return g


def _matrix(mods, masked):
    if masked not in _mat:
        L, N, coo = dr.case_matrix()
        mask = dr.case_mask() if masked else None
        _mat[masked] = (mask, mods["cl"].Matrix(L, N, coo, mask))
    return _mat[masked]


def _same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def _within_2ulp(got, want):
    got, want = np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(np.asarray(want, np.float64))
    fin = np.isfinite(want)
    return (np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
            and (np.abs(got[fin] - want[fin]) <= 2 * np.spacing(np.abs(want[fin]))).all())


def _check(mods, g, S, rho, assign, masked, err=0.02, min_loci=3, donors_at=None):
    L, N, coo = dr.case_matrix()
    A, R = dr.totals(L, coo)
    gt = dr.case_gt(S)
    mask, mat = _matrix(mods, masked)
    G = len(rho)
    got = g.ambient_profile(gt, assign, rho, err, min_loci, mask, tables=True)
    # the tables: inside the bound of the reference, the call of their own, the donor tables at every third grid point
    r_tab = ar.compare_tab(A, R, rho, err, mask, got["tab"])
    assert r_tab <= 1.0, r_tab
    assert _same(g.ambient_tables(rho, err, mask)["tab"], got["tab"])
    part = assign != 255
    for j in (donors_at if donors_at is not None else (0, G // 2, G - 1)):
        d = g.donor_posteriors(gt, mask=mask, tables=True, err=err, ambient=float(rho[j]))
        assert _same(d["tab1"], got["tab"][:, :, j]), j
        assert _same(got["ll"][part, j], d["ll"][part, assign[part]]), (j, np.abs(got["ll"][part, j] - d["ll"][part, assign[part]]).max())
        assert np.array_equal(got["n_entries"][part], d["n_entries"][part])
    # the twin fed the device's tables
    tw = mods["am"].profile(mat, gt, assign, rho, tab=got["tab"], err=err, min_loci=min_loci)
    for k in ("ll", "total", "source_total", "cell_rho"):
        assert _same(got[k], tw[k]), (k, S, G, masked)
    assert np.array_equal(got["n_entries"], tw["n_entries"]) and np.array_equal(got["source_cells"], tw["source_cells"])
    assert _within_2ulp(got["cell_se"], tw["cell_se"])
    # the reference's bounds
    res, _ = ar.compare(N, coo, gt, assign, mask, got)
    print(S, G, masked, "tab", round(r_tab, 3), {k: round(v, 3) for k, v in res.items()})
    assert max(res.values()) <= 1.0, res
    out = ~part | (got["n_entries"] < min_loci)
    assert np.isnan(got["cell_rho"][out]).all() and np.isnan(got["cell_se"][out]).all() and not np.isnan(got["cell_rho"][~out]).any()
    assert (got["ll"][~part] == 0).all() and (got["n_entries"][~part] == 0).all()
    return got


@ENGINES
@MASKED
@SOURCES
def test_profile_over_every_grid_width(mods, S, masked, engine):
    g = _make(mods, engine)
    assign = ar.case_assign(S, KIND[S])
    for G in ar.GRIDS:
        got = _check(mods, g, S, ar.case_grid(G), assign, masked)
        if KIND[S] == "hole":
            assert got["source_cells"][S // 2] == 0 and (got["source_total"][S // 2] == 0).all()
    again = g.ambient_profile(dr.case_gt(S), assign, ar.case_grid(ar.GRIDS[-1]), 0.02, 3, _matrix(mods, masked)[0], tables=True)
    assert all(_same(got[k], again[k]) for k in got)
    g.close()


@ENGINES
def test_tables_are_the_donor_tables_at_every_grid_point(mods, engine):
    g = _make(mods, engine)
    gt = dr.case_gt(3)
    for G, mask, err in ((4, None, 0.01), (17, dr.case_mask(), 0.2), (32, dr.case_mask(), 1e-6)):
        rho = ar.case_grid(G)
        tab = g.ambient_tables(rho, err, mask)["tab"]
        for j in range(G):
            assert _same(tab[:, :, j], g.donor_tables(gt, mask, err=err, ambient=float(rho[j]))["tab1"]), (G, j)
        if mask is not None:
            assert (tab[mask == 0] == 0).all()
    g.close()


@ENGINES
def test_a_callers_grid_and_nobody_taking_part(mods, engine):
    g = _make(mods, engine)
    rho = ar.case_grid_uneven()
    _check(mods, g, 3, rho, ar.case_assign(3), True, err=0.01, min_loci=1, donors_at=range(len(rho)))
    _check(mods, g, 33, rho[:5], ar.case_assign(33, "hole"), False)
    got = _check(mods, g, 3, ar.case_grid(4), ar.case_assign(3, "none"), False)
    assert (got["total"] == 0).all() and (got["source_total"] == 0).all() and (got["source_cells"] == 0).all()
    assert np.isnan(got["cell_rho"]).all()
    zeros = np.zeros(dr.CASE_L, np.uint8)  # no locus left: every sum 0, nobody has min_loci entries
    got = g.ambient_profile(dr.case_gt(3), ar.case_assign(3), ar.case_grid(8), mask=zeros, tables=True)
    assert (got["ll"] == 0).all() and (got["tab"] == 0).all() and (got["n_entries"] == 0).all() and np.isnan(got["cell_rho"]).all()
    g.close()


def _summary_is_the_twins(got, tw, S):
    for k in ("rho", "curvature", "log_likelihood", "lo", "hi", "j_star", "at_boundary", "rounds", "n_cells_used"):
        assert _same(np.float64(got[k]), np.float64(tw[k])), (k, got[k], tw[k])
    assert _same(got["source_rho"], tw["source_rho"][:S]) and np.array_equal(got["source_cells"], tw["source_cells"][:S])
    assert _within_2ulp(got["se"], tw["se"]) and _within_2ulp(got["source_se"], tw["source_se"][:S])
    assert _same(got["cell_rho"], tw["cell_rho"]) and _within_2ulp(got["cell_se"], tw["cell_se"])
    assert np.array_equal(got["n_entries"], tw["n_entries"])


@ENGINES
def test_estimate_on_the_case_matrix_is_the_twins(mods, engine):
    g = _make(mods, engine)
    for S, masked, kind, prm in ((33, True, "hole", dict(grid=8, rounds=5, err=0.02, min_loci=3)), (3, False, "mixed", {}),
                                 (1, True, "mixed", dict(grid=32, rounds=1, lo=0.1, hi=0.9)), (3, False, "none", dict(grid=4))):
        gt, assign = dr.case_gt(S), ar.case_assign(S, kind)
        mask, mat = _matrix(mods, masked)
        got = g.estimate_ambient(gt, assign, mask, **prm)
        tw = mods["am"].estimate(mat, gt, assign, tables_of=lambda rho: g.ambient_tables(rho, prm.get("err", 0.01), mask)["tab"], **prm)
        _summary_is_the_twins(got, tw, S)
        assert prm.get("lo", 0.0) <= got["rho"] <= prm.get("hi", 0.5) and got["summary"].rounds == prm.get("rounds", 3)
        assert np.isnan(got["source_rho"][got["source_cells"] == 0]).all()
        again = g.estimate_ambient(gt, assign, mask, **prm)
        assert bytes(again["summary"]) == bytes(got["summary"]) and _same(again["cell_rho"], got["cell_rho"])
    g.close()


@ENGINES
def test_estimate_recovers_a_planted_ambient_fraction(mods, engine):
    planted = 0.08
    L, N, coo, gt, assign = ar.planted(planted, 0)
    g = _make(mods, engine, (L, N, coo))
    got = g.estimate_ambient(gt, assign)
    print("estimate", got["rho"], "se", got["se"], "z", abs(got["rho"] - planted) / got["se"])
    assert got["curvature"] < 0 and abs(got["rho"] - planted) <= 4.0 * got["se"]
    assert not got["at_boundary"] and got["n_cells_used"] == N and got["source_cells"].tolist() == [180, 90, 30]
    tw = mods["am"].estimate(mods["cl"].Matrix(L, N, coo), gt, assign, tables_of=lambda rho: g.ambient_tables(rho)["tab"])
    _summary_is_the_twins(got, tw, 3)
    ok = np.isfinite(got["cell_se"])
    assert ok.sum() > 0.9 * N and np.median(got["cell_se"][ok]) > 5 * got["se"]  # (a cell alone knows far less than the pool)
    # a fourth source without any call takes the third donor's cells: its profile is rounding noise, which the vertex rule does not fit
    gt4 = np.concatenate([gt, np.full((1, L), 3, np.uint8)])
    a4 = np.where(assign == 2, 3, assign).astype(np.uint8)
    got = g.estimate_ambient(gt4, a4)
    tw = mods["am"].estimate(mods["cl"].Matrix(L, N, coo), gt4, a4, tables_of=lambda rho: g.ambient_tables(rho)["tab"])
    _summary_is_the_twins(got, tw, 4)
    assert got["source_cells"].tolist() == [180, 90, 0, 30] and np.isnan(got["source_rho"][2]) and np.isnan(got["source_se"][2])
    assert got["source_se"][3] == np.inf and got["source_rho"][3] in tw["grid"] and np.isfinite(got["source_se"][:2]).all()
    mine = a4 == 3
    assert (got["cell_se"][mine] == np.inf).all() and np.isin(got["cell_rho"][mine], ar.case_grid(16)).all()
    g.close()


# ---- the EM state stays ----------------------------------------------------------------------------------------------------------------
@ENGINES
def test_ambient_calls_leave_the_loop_alone(mods, engine):
    mask = dr.case_mask()
    x, y = _make(mods, engine), _make(mods, engine)
    want = [x.em_iteration(5.0) for _ in range(4)]
    got = []
    for it in range(4):
        got.append(y.em_iteration(5.0))
        if it == 1:
            state = (y.excluded(), y.loci_mask())
            y.ambient_tables(ar.case_grid(16), 0.01, mask)
            y.ambient_profile(dr.case_gt(33), ar.case_assign(33), ar.case_grid(17), mask=mask)
            y.estimate_ambient(dr.case_gt(3), ar.case_assign(3), mask)
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
    gt3, a3, rho = dr.case_gt(3), ar.case_assign(3), ar.case_grid(8)

    def refused(fn, match):
        with pytest.raises(ffi.CellectorError, match=match) as e:
            fn()
        assert e.value.status == 1

    def every_call(g, match, n=N):
        refused(lambda: g.ambient_tables(rho), match)
        refused(lambda: g.ambient_profile(gt3, a3[:n], rho), match)
        refused(lambda: g.estimate_ambient(gt3, a3[:n]), match)

    g = _make(mods, 2)
    state = (g.em_iteration(5.0), g.excluded(), g.loci_mask())
    for S in (0, 65):
        refused(lambda: g.ambient_profile(np.zeros((S, L), np.uint8), np.full(N, 255, np.uint8), rho), "1..64 are supported")
        refused(lambda: g.estimate_ambient(np.zeros((S, L), np.uint8), np.full(N, 255, np.uint8)), "1..64 are supported")
    bad = gt3.copy()
    bad[2, 17] = 4
    refused(lambda: g.ambient_profile(bad, a3, rho), "source 2 at locus 17 is 4")
    refused(lambda: g.estimate_ambient(bad, a3), "source 2 at locus 17 is 4")
    bad_a = a3.copy()
    bad_a[9] = 3
    refused(lambda: g.ambient_profile(gt3, bad_a, rho), "assign of cell 9 is 3")
    refused(lambda: g.estimate_ambient(gt3, bad_a), "assign of cell 9 is 3")
    for G in (3, 33):
        refused(lambda: g.ambient_tables(ar.case_grid(G)), "4..32 are supported")
        refused(lambda: g.ambient_profile(gt3, a3, ar.case_grid(G)), "4..32 are supported")
        refused(lambda: g.estimate_ambient(gt3, a3, grid=G), "4..32 are supported")
    for v in (1.0, -0.1, np.nan, np.inf):
        r = rho.copy()
        r[5] = v
        refused(lambda: g.ambient_tables(r), r"rho\[5\]")
        refused(lambda: g.ambient_profile(gt3, a3, r), r"rho\[5\]")
    for v in (0.0, 0.5, -0.1, np.nan):
        refused(lambda: g.ambient_tables(rho, err=v), "err")
        refused(lambda: g.ambient_profile(gt3, a3, rho, err=v), "err")
        refused(lambda: g.estimate_ambient(gt3, a3, err=v), "err")
    for lo, hi in ((-0.1, 0.5), (0.3, 0.3), (0.4, 0.2), (0.0, 1.0), (np.nan, 0.5), (0.0, np.nan)):
        refused(lambda: g.estimate_ambient(gt3, a3, lo=lo, hi=hi), "0 <= lo < hi < 1")
    for v in (0, 9):
        refused(lambda: g.estimate_ambient(gt3, a3, rounds=v), "1..8 are supported")
    refused(lambda: g.ambient_profile(gt3, a3, rho, min_loci=0), "min_loci")
    refused(lambda: g.estimate_ambient(gt3, a3, min_loci=0), "min_loci")
    lib = ffi.load_library()
    err = lambda: lib.cellector_last_error(g.h)
    assert lib.cellector_ambient_tables(g.h, None, 8, 0.01, None, None) == 1 and b"null rho" in err()
    assert lib.cellector_ambient_profile(g.h, gt3.ctypes.data, 3, a3.ctypes.data, None, 8, 0.01, 1, *([None] * 9)) == 1 and b"null rho" in err()
    assert lib.cellector_ambient_profile(g.h, None, 3, a3.ctypes.data, rho.ctypes.data, 8, 0.01, 1, *([None] * 9)) == 1 and b"null gt" in err()
    assert lib.cellector_ambient_profile(g.h, gt3.ctypes.data, 3, None, rho.ctypes.data, 8, 0.01, 1, *([None] * 9)) == 1 and b"null assign" in err()
    assert lib.cellector_estimate_ambient(g.h, None, 3, a3.ctypes.data, *([None] * 6)) == 1 and b"null gt" in err()
    assert lib.cellector_estimate_ambient(g.h, gt3.ctypes.data, 3, None, *([None] * 6)) == 1 and b"null assign" in err()
    g.em_begin()
    every_call(g, "in flight")
    g.em_threshold(5.0)
    every_call(g, "in flight")
    g.em_finish()
    # the ctx is as it was: the loop goes on with the bits of an undisturbed one, and the calls work (with every output NULL too)
    h = _make(mods, 2)
    assert bytes(h.em_iteration(5.0)) == bytes(state[0])
    h.em_iteration(5.0)
    assert bytes(g.em_iteration(5.0)) == bytes(h.em_iteration(5.0))
    assert np.array_equal(g.excluded(), h.excluded()) and np.array_equal(g.loci_mask(), h.loci_mask())
    h.close()
    assert lib.cellector_ambient_profile(g.h, gt3.ctypes.data, 3, a3.ctypes.data, rho.ctypes.data, 8, 0.01, 1, *([None] * 9)) == 0
    assert lib.cellector_estimate_ambient(g.h, gt3.ctypes.data, 3, a3.ctypes.data, *([None] * 6)) == 0
    assert g.estimate_ambient(gt3, a3)["n_cells_used"] == int((a3 != 255).sum())
    g.close()
    g = mods["Cellector"](0)
    assert lib.cellector_ambient_tables(g.h, rho.ctypes.data, 8, 0.01, None, None) == 1 and b"no matrix loaded" in lib.cellector_last_error(g.h)
    assert lib.cellector_estimate_ambient(g.h, gt3.ctypes.data, 3, a3.ctypes.data, *([None] * 6)) == 1
    assert b"no matrix loaded" in lib.cellector_last_error(g.h)
    g.close()
    m = mods["Cellector"](devices=[0, 0])
    m.load_coo(L, N, *S_._u32(coo), 0, 0)
    every_call(m, "single-device")
    assert m.em_iteration(5.0) is not None
    m.close()
    g = mods["Cellector"](0)
    g.set_shard(10, 40)
    g.load_coo(L, N, *S_._u32(coo), 0, 0)
    every_call(g, "set_shard", n=30)
    g.close()
