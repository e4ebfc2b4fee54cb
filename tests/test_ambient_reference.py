"""CPU: the numpy twin of the ambient calls (cellector_amd/ambient.py) against the 80-bit statement of the model in
tests/ambient_reference.py on the matrix the GPU test uses, the sensitivity of the bounds (one entry under the wrong genotype row),
the concavity of every profile, the recovery of a planted ambient fraction by the reference, and the flat profile of a source
without any call.

Recovery: ambient_reference.planted, 300 cells x 400 loci, 3 donors, rho in {0, 0.03, 0.08, 0.2}, seeds 0 - 3.  The cap is 4 standard
errors of the reference's own estimate; no seed had to be replaced.
"""
import math

import numpy as np
import pytest

import ambient_reference as ar
import donor_reference as dr
from cellector_amd import ambient, cluster, donors

_memo = {}


def _once(key, fn):
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def _mat(masked):
    L, N, coo = dr.case_matrix()
    mask = dr.case_mask() if masked else None
    return mask, _once(("mat", masked), lambda: cluster.Matrix(L, N, coo, mask))


CASES = [(S, G, masked, kind) for S, G in zip(ar.SOURCES, (16, 5, 17, 32)) for masked in (False, True)
         for kind in (("mixed", "hole") if masked else ("mixed",))] + [(3, 4, False, "none"), (3, 9, True, "uneven")]


@pytest.mark.parametrize("S, G, masked, kind", CASES)
def test_twin_is_inside_the_references_bounds(S, G, masked, kind):
    L, N, coo = dr.case_matrix()
    A, R = dr.totals(L, coo)
    mask, mat = _mat(masked)
    gt = dr.case_gt(S)
    rho = ar.case_grid_uneven() if kind == "uneven" else ar.case_grid(G)
    assign = ar.case_assign(S, "mixed" if kind == "uneven" else kind)
    if kind != "uneven":
        assert ambient.grid(0.0, 0.5, G).tobytes() == rho.tobytes()
    got = ambient.profile(mat, gt, assign, rho, A, R, err=0.02, min_loci=3)
    assert ar.compare_tab(A, R, rho, 0.02, mask, got["tab"]) <= 1.0
    res, ref = ar.compare(N, coo, gt, assign, mask, got)
    print(S, G, masked, kind, {k: round(v, 3) for k, v in res.items()})
    assert max(res.values()) <= 1.0, res
    out = (assign == 255) | (got["n_entries"] < 3)
    assert np.isnan(got["cell_rho"][out]).all() and np.isnan(got["cell_se"][out]).all()
    assert not np.isnan(got["cell_rho"][~out]).any() and (got["cell_se"][~out] > 0).all()
    assert (got["ll"][assign == 255] == 0).all() and (got["n_entries"][assign == 255] == 0).all()
    assert ((got["cell_rho"][~out] >= rho[0]) & (got["cell_rho"][~out] <= rho[-1])).all()
    if kind == "none":
        assert (got["total"] == 0).all() and (got["source_cells"] == 0).all()
    if kind == "hole" and S >= 2:
        assert got["source_cells"][S // 2] == 0 and (got["source_total"][S // 2] == 0).all()
    # the column of a grid point is the donor calls' singlet sum at that ambient fraction, bit for bit
    for j in (0, G // 2, len(rho) - 1):
        tab1 = got["tab"][:, :, j]
        s = donors.singlet_sums(mat, tab1, gt.T)
        part = assign != 255
        assert got["ll"][part, j].tobytes() == s[part, assign[part]].tobytes()

    # one entry scored under the wrong genotype row: per cell the first entry with exactly one non-zero count, its row g replaced by
    # (g + 1) mod 4.  The sum moves by the entry's term, alt (la' - la) or ref (lb' - lb): more than 100 bounds wherever the rows differ
    lo, ce, al, re, g = ref["rows"]
    one = (al > 0) != (re > 0)
    first = np.zeros(len(ce), bool)
    idx = np.flatnonzero(one)
    first[idx[np.unique(ce[idx], return_index=True)[1]]] = True
    tab = got["tab"].astype(ar.LD)
    comp = np.where(al[first] > 0, 0, 1)
    r = np.arange(first.sum())
    was, now = tab[lo[first], g[first]][r, :, comp], tab[lo[first], (g[first] + 1) % 4][r, :, comp]
    moved = np.abs((al[first] + re[first]).astype(ar.LD)[:, None] * (now - was)).astype(np.float64)
    differ = now != was
    if kind != "none":
        assert first.sum() > 0.5 * (ref["n_entries"] > 0).sum() and differ.mean() > 0.9
    assert (moved[differ] > 100 * ref["B_ll"][ce[first]][differ]).all()


def test_tables_carry_the_donor_tables_at_equal_ambient():
    L, N, coo = dr.case_matrix()
    A, R = dr.totals(L, coo)
    mask = dr.case_mask()
    rho = ar.case_grid_uneven()
    tab = ambient.tables(A, R, rho, 0.01, mask)
    for j, r in enumerate(rho):
        assert tab[:, :, j].tobytes() == donors.tables(A, R, 0.01, float(r), mask)[0].tobytes()
    assert (tab[mask == 0] == 0).all() and np.isfinite(tab).all() and (tab[mask != 0] < 0).all()


def test_fold_is_the_cluster_objectives_fold():
    rng = np.random.default_rng(4)
    ll = rng.normal(size=(1000, 5)) * 100
    assign = np.zeros(1000, np.uint8)
    total, src, cells = ambient.fold(ll, assign, 2)
    assert total.tobytes() == cluster.objective_sum(ll).tobytes() and src[0].tobytes() == total.tobytes()
    assert (src[1] == 0).all() and cells.tolist() == [1000, 0]


def test_vertex_rule_by_hand():
    rho = np.array([0.0, 0.1, 0.3, 0.4])
    f = lambda x: -3.0 * (x - 0.22) ** 2 + 1.0
    v = ambient.vertex(rho, f(rho))
    assert v["j_star"] == 2 and abs(v["rho"] - 0.22) < 1e-12 and abs(v["curvature"] + 6.0) < 1e-9
    assert abs(v["se"] - 1.0 / math.sqrt(6.0)) < 1e-12
    v = ambient.vertex(rho, f(rho + 0.5))  # the maximum left of the grid: clamped at rho[0]
    assert v["j_star"] == 0 and v["rho"] == 0.0 and np.isfinite(v["se"])
    v = ambient.vertex(rho, np.zeros(4))   # flat
    assert v["j_star"] == 0 and v["rho"] == 0.0 and v["se"] == math.inf and v["curvature"] == 0.0
    v = ambient.vertex(rho, rho * rho)     # convex: the grid point, no standard error
    assert v["j_star"] == 3 and v["rho"] == 0.4 and v["se"] == math.inf and v["curvature"] > 0
    w = ambient.vertex(rho, np.stack([f(rho), np.zeros(4)]))
    assert w["j_star"].tolist() == [2, 0] and w["se"][1] == math.inf
    got = ar.vertex_reference(rho, f(rho))
    assert got[0] == 2 and abs(got[1] - 0.22) < 1e-12


@pytest.mark.parametrize("rho", ar.PLANT_RHOS)
def test_reference_recovers_the_planted_ambient_fraction(rho):
    worst = 0.0
    for seed in ar.PLANT_SEEDS:
        L, N, coo, gt, assign = ar.planted(rho, seed)
        ref = ar.estimate_reference(L, N, coo, gt, assign)
        z = abs(ref["rho"] - rho) / ref["se"]
        worst = max(worst, z)
        print(f"rho {rho} seed {seed}: estimate {ref['rho']:.5f} se {ref['se']:.5f} z {z:.2f} at_boundary {ref['at_boundary']}")
        assert ref["curvature"] < 0 and 0.0005 < ref["se"] < 0.01
        assert z <= 4.0, (rho, seed, ref["rho"], ref["se"])
        assert 0.0 <= ref["rho"] <= 0.5
        assert ref["at_boundary"] == int(ref["rho"] == 0.0)
        if rho > 0.02:
            assert not ref["at_boundary"]
        # concavity: the second divided differences of every round's total are negative
        for grid, total in zip(ref["grids"], ref["totals"]):
            d = np.diff(total) / np.diff(grid.astype(ar.LD))
            assert (np.diff(d) < 0).all(), (rho, seed)
        # the twin finds the same maximum: the same cell of every round's grid, an estimate a small share of the se away.  (Its totals
        # carry a rounding error near 300 u |total| ~ 1e-9; over the last round's step h ~ 6e-4 and a curvature near -1e5 that moves
        # the vertex by about 1e-9 / (h |c|) ~ 2e-11, against 1e-3 se ~ 3e-6.)
        mat = _once(("plant", rho, seed), lambda: cluster.Matrix(L, N, coo))
        A, R = dr.totals(L, coo)
        tw = ambient.estimate(mat, gt, assign, A, R)
        assert tw["j_star"] == ref["j_star"] and tw["lo"] == ref["lo"] and tw["hi"] == ref["hi"]
        assert abs(tw["rho"] - ref["rho"]) < 1e-3 * ref["se"] and abs(tw["se"] - ref["se"]) < 1e-6 * ref["se"]
        assert tw["at_boundary"] == ref["at_boundary"] and tw["n_cells_used"] == N
        d = np.diff(tw["total"]) / np.diff(tw["grid"])
        assert (np.diff(d) < 0).all()
        assert np.array_equal(tw["source_cells"][:3], [180, 90, 30])
        ok = np.isfinite(ref["source_se"])
        assert np.allclose(tw["source_rho"][:3][ok], ref["source_rho"][ok], atol=1e-3 * ref["se"], rtol=0)
    print(f"rho {rho}: worst |estimate - rho| / se = {worst:.2f}")


def test_zero_ambient_clamps_at_the_boundary():
    """of the rho = 0 pools at least one has its unclamped vertex below 0: the estimate is exactly lo and at_boundary is set"""
    hits = 0
    for seed in ar.PLANT_SEEDS:
        ref = ar.estimate_reference(*ar.planted(0.0, seed))
        assert ref["rho"] >= 0.0
        assert ref["at_boundary"] == int(ref["rho"] == 0.0)
        hits += ref["at_boundary"]
    assert hits >= 1


def _no_call_pool():
    """a fourth source whose every call is 3 takes the third donor's cells; the third source is left without a cell"""
    L, N, coo, gt, assign = ar.planted(0.08, 0)
    gt4 = np.concatenate([gt, np.full((1, L), 3, np.uint8)])
    a4 = assign.copy()
    a4[assign == 2] = 3
    return L, N, coo, gt4, a4, _once("no-call", lambda: ar.estimate_reference(L, N, coo, gt4, a4))


def test_a_source_without_a_cell_and_a_source_without_a_call():
    """The first gets NaN.  The second's theta is soup at every rho up to the rounding of ((1 - rho) soup) + (rho soup), within 3 u of
    soup: its profile is flat to 6 u sum (alt + ref soup / (1 - soup)) over its cells' entries.  That is rounding noise of either sign,
    far below the 2^-40 of the value the vertex rule asks of a step: c >= 0, se = +inf and rho = rho[j*], as for an exactly flat one.
    (Without that floor the parabola through the noise of this pool had curvature -4.2e-07 and se 1541.)"""
    L, N, coo, gt4, a4, ref = _no_call_pool()
    assert ref["source_cells"].tolist() == [180, 90, 0, 30]
    assert np.isnan(ref["source_rho"][2]) and np.isnan(ref["source_se"][2])
    A, R = dr.totals(L, coo)
    soup = (A + 1.0) / ((A + R) + 2.0)
    lo, ce, al, re = coo
    mine = a4[ce] == 3
    flat = 6 * ar.U * (al[mine] + re[mine] * soup[lo[mine]] / (1.0 - soup[lo[mine]])).sum()
    y = ref["source_total"][3]
    print("spread", float(y.max() - y.min()), "bound", flat, "floor", float(ar.FLAT * abs(y[0])))
    assert 0 < float(y.max() - y.min()) <= flat < 1e-3 * float(ar.FLAT * abs(y).min())
    print("curvature", ref["source_curvature"][3], "se", ref["source_se"][3], "rho", ref["source_rho"][3], "j*", ref["source_j"][3])
    assert ref["source_curvature"][3] >= 0 and ref["source_se"][3] == math.inf
    assert ref["source_rho"][3] == ref["grids"][-1][ref["source_j"][3]]
    assert np.isfinite(ref["source_se"][:2]).all() and ref["curvature"] < 0  # (the sources that bear on rho are resolved)
    tw = ambient.estimate(cluster.Matrix(L, N, coo), gt4, a4, A, R)
    assert np.isnan(tw["source_rho"][2]) and tw["source_cells"][:4].tolist() == [180, 90, 0, 30]
    assert tw["source_se"][3] == math.inf and tw["source_rho"][3] in tw["grid"] and np.isfinite(tw["source_se"][:2]).all()
    assert abs(tw["rho"] - ref["rho"]) < 1e-3 * ref["se"]


def test_the_vertex_rule_does_not_fit_rounding_noise():
    rho = ar.case_grid(8)
    y = np.full(8, -5000.0)
    noise = y + np.array([0, 1, -2, 3, -1, 2, 0, -3]) * np.spacing(5000.0)  # a few ulps either way
    v = ambient.vertex(rho, noise)
    assert v["j_star"] == 3 and v["curvature"] == 0.0 and v["se"] == math.inf and v["rho"] == rho[3]
    assert ar.vertex_reference(rho, noise)[1:] == (float(rho[3]), math.inf, 0.0)
    # one resolved step is enough: the parabola is fitted
    y2 = y.copy()
    y2[3] += 5000.0 * 2.0 ** -39
    v = ambient.vertex(rho, y2)
    assert v["curvature"] < 0 and np.isfinite(v["se"]) and ar.vertex_reference(rho, y2)[3] < 0
