"""CPU: the numpy twin of the donor pair fractions (cellector_amd/pair_fraction.py) against the 80-bit statement of the model in
tests/pair_fraction_reference.py on the matrix the GPU test uses; the three identity columns (f = 0.5, 1, 0) against donors.py; the
sensitivity of the bounds (a table indexed 4 g_b + g_a, a grid read in reverse); the recovery of planted shares by the reference; the
kinds of the planted cells; the flat profile of a pair that shares every genotype.

Sensitivity, measured with the reference alone on donor_reference.case_matrix() under pair_fraction_reference.case_pairs: of the cells
that take part and have an entry, those without an entry that bears on f (a read at a locus where the pair's two thetas differ) are
D = 2: 4.0 % (4.9 % under case_mask()), D = 3: 0.8 % (0 %), D = 33 and D = 64: 1.3 % (0 %); the cap is 5 %.  (Before case_pairs
stepped such cells on to another donor the figure was 5.6 % at D = 64 and 6.5 % under the mask; D = 2 has one pair and nothing to
step to.)  The tenth of the case matrix' rows that hold no entry at all are not counted: their sums are 0.0 under any table, and no
pair rule gives them an entry; with them the share of the cells that take part is 10.7 % ... 16.7 %, printed beside the other.  Every
cell with such an entry is wrong by more than 100 bounds at some grid point under either mistake.

Recovery: pair_fraction_reference.planted, seeds 0 - 2, 300 cells per planted share and seed, the default grid j / 16, parent depth
1 + Poisson(2).  Measured with the 80-bit reference against the PLANTED share: the worst |estimate - f| / se over the 3600 cells is
4.30 (f = 0.5, seed 2), the cap is that plus a quarter; the mean estimate per planted share is 0.9944 / 0.5015 / 0.3023 / 0.1541 for
f = 1 / 0.5 / 0.3 / 0.15 (at 1 the estimate is clamped from above, so its mean lies below), median se 0.040 / 0.033 / 0.031 / 0.025.
Kinds at min_fraction 0.1: all 900 planted singlets "toward a" (the lowest estimate 0.921), all 1800 cells planted at 0.5 and 0.3
"balanced" (0.395 ... 0.644 and 0.199 ... 0.391); of the 900 planted at 0.15, 884 are balanced and 16 "toward b" (reported, not
asserted).  At parent depth 1 + Poisson(1) one planted singlet of 900 came out at 0.883: the depth was raised, not the condition.
"""
import math

import numpy as np
import pytest

import ambient_reference as ar
import donor_reference as dr
import pair_fraction_reference as pf
from cellector_amd import cluster, donors, pair_fraction

_memo = {}
ERR, AMB = 0.02, 0.05
WORST_Z = 4.30  # measured (the module docstring); the cap is a quarter above it


def _once(key, fn):
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def _mat(masked):
    L, N, coo = dr.case_matrix()
    mask = dr.case_mask() if masked else None
    return mask, _once(("mat", masked), lambda: cluster.Matrix(L, N, coo, mask))


def _grid(G):
    return None if G == "default" else pf.case_grid_uneven() if G == "uneven" else pf.case_grid(G)


CASES = [(D, G, masked) for D in pf.DONORS for G in ar.GRIDS for masked in (False, True)] + \
        [(D, G, masked) for D in (3, 64) for G in ("uneven", "default") for masked in (False, True)]


@pytest.mark.parametrize("D, G, masked", CASES)
def test_twin_is_inside_the_references_bounds(D, G, masked):
    L, N, coo = dr.case_matrix()
    A, R = dr.totals(L, coo)
    mask, mat = _mat(masked)
    gt = dr.case_gt(D)
    a, b = pf.case_pairs(D)
    frac = _grid(G)
    got = pair_fraction.pair_fractions(mat, gt.T, a, b, frac, A, R, params=dict(min_loci=3), err=ERR, ambient=AMB)
    frac = got["frac"]
    if G == "default":
        assert frac.tobytes() == pf.DEFAULT_GRID.tobytes() and len(frac) == 17 and frac[8] == 0.5
    r_tab = pf.compare_tab(A, R, frac, ERR, AMB, mask, got["tab"])
    res, ref = pf.compare(N, coo, gt, a, b, mask, got)
    print(D, G, masked, "tab", round(r_tab, 3), {k: round(v, 3) for k, v in res.items()})
    assert r_tab <= 1.0 and max(res.values()) <= 1.0, (r_tab, res)
    part = a != 255
    out = ~part | (got["n_entries"] < 3)
    assert np.isnan(got["cell_frac"][out]).all() and np.isnan(got["cell_se"][out]).all() and (got["kind"][out] == 255).all()
    assert not np.isnan(got["cell_frac"][~out]).any() and (got["cell_se"][~out] > 0).all() and (got["kind"][~out] <= 3).all()
    assert ((got["cell_frac"][~out] >= 0.0) & (got["cell_frac"][~out] <= 1.0)).all()
    assert (got["ll"][~part] == 0).all() and (got["n_entries"][~part] == 0).all() and (got["j_star"][~part] == 0).all()
    assert ((got["kind"] == 3) == (got["cell_se"] == np.inf)).all()
    s = got["summary"]
    assert s["n_balanced"] + s["n_toward_a"] + s["n_toward_b"] + s["n_flat"] + s["n_none"] == N and s["n_none"] == out.sum()
    assert s["donor_cells"].sum() == s["n_toward_a"] + s["n_toward_b"]

    # the three identity columns: the donor calls' tables and sums, bit for bit
    tab1, tab2 = donors.tables(A, R, ERR, AMB, mask)
    anchor = np.where(part, a, 0)
    s1, p2 = donors.singlet_sums(mat, tab1, gt.T), donors.pair_sums(mat, tab2, gt.T, anchor)
    r = np.flatnonzero(part)
    seen = 0
    for j, f in enumerate(frac):
        if f == 0.5:
            assert got["tab"][:, :, j].tobytes() == tab2.tobytes()
            assert got["ll"][r, j].tobytes() == p2[r, b[r]].tobytes()
        elif f == 1.0:
            assert got["tab"][:, :, j].tobytes() == tab1[:, np.repeat(np.arange(4), 4)].tobytes()
            assert got["ll"][r, j].tobytes() == s1[r, a[r]].tobytes()
        elif f == 0.0:
            assert got["tab"][:, :, j].tobytes() == tab1[:, np.tile(np.arange(4), 4)].tobytes()
            assert got["ll"][r, j].tobytes() == s1[r, b[r]].tobytes()
        else:
            continue
        seen += 1
    assert seen == (3 if len(frac) % 2 else 2)

    # sensitivity: the table indexed 4 g_b + g_a, and the grid read in reverse: more than 100 bounds at some grid point in every cell
    # with an entry that bears on f
    inf = pf.informative(N, coo, gt, a, b, A, R, ERR, AMB, mask)
    has = part & (ref["n_entries"] > 0)
    share = (has & ~inf).sum() / has.sum()
    print(f"D {D} masked {masked}: {has.sum()} cells with an entry, {share:.3%} of them without one that bears on f; of all {part.sum()} "
          f"that take part {(part & ~inf).sum() / part.sum():.3%}")
    assert share <= 0.05
    swapped = pf.cell_reference(N, coo, gt, a, b, got["tab"], mask, index=lambda ga, gb: 4 * gb + ga)["ll"]
    for name, wrong in (("swapped", swapped), ("reversed", ref["ll"][:, ::-1])):
        off = (np.abs(wrong - ref["ll"]).astype(np.float64) > 100 * ref["B_ll"]).any(axis=1)
        assert off[inf].all(), (name, np.flatnonzero(inf & ~off)[:10])
        assert not off[~has].any()


def test_tables_by_hand_and_masked_rows():
    L, N, coo = dr.case_matrix()
    A, R = dr.totals(L, coo)
    mask = dr.case_mask()
    tab = pair_fraction.tables(A, R, None, 0.01, 0.03, mask)
    assert tab.shape == (L, 16, 17, 2) and (tab[mask == 0] == 0).all() and np.isfinite(tab).all() and (tab[mask != 0] < 0).all()
    th = donors.thetas(A, R, 0.01, 0.03)
    l, ga, gb, j = 11, 2, 0, 3
    assert mask[l] and tab[l, 4 * ga + gb, j, 0] == np.log((3 / 16.0 * th[l, ga]) + ((1.0 - 3 / 16.0) * th[l, gb]))
    # the diagonal knows nothing of f beyond the rounding of (f x) + ((1 - f) x): 3 u of theta or of 1 - theta (>= 0.0097), so an
    # absolute 3 u / 0.0097 < 4e-14 of their logarithms, and two roundings of a log below 5 in size
    d = tab[:, [0, 5, 10, 15]]
    assert (np.abs(d - d[:, :, 8:9]) <= 4e-14).all()


def test_kinds_by_hand():
    f = np.array([0.95, 0.9, 0.9000001, 0.05, 0.1, 0.5, 0.7, 0.5, 0.5])
    se = np.array([0.1, 0.1, 0.1, 0.1, 0.1, 0.1, np.inf, 0.1, 0.1])
    cnt = np.array([5, 5, 5, 5, 5, 5, 5, 2, 5])
    a = np.array([0, 0, 0, 0, 0, 0, 0, 0, 255])
    assert pair_fraction.kinds(f, se, cnt, a, 0.1, 3).tolist() == [1, 0, 1, 2, 0, 0, 3, 255, 255]
    assert pair_fraction.kinds(f, se, cnt, a, 0.0, 1).tolist() == [0, 0, 0, 0, 0, 0, 3, 0, 255]
    ref = pf.fractions_reference(np.array([0.0, 0.5, 1.0, 2.0]), np.zeros((2, 4), pf.LD), np.array([3, 0]), np.array([0, 0]))
    assert ref["kind"].tolist() == [3, 255] and ref["cell_se"][0] == math.inf and np.isnan(ref["cell_se"][1])
    for k in pair_fraction.DEFAULTS:
        assert pair_fraction.DEFAULTS[k] == pf.DEFAULTS[k]
    assert pair_fraction.DEFAULT_GRID.tobytes() == pf.DEFAULT_GRID.tobytes()


def _planted(seed):
    def run():
        L, N, coo, gt, a, b, f = pf.planted(seed)
        return pf.estimate_reference(L, N, coo, gt, a, b)
    return pf.planted(seed), _once(("planted", seed), run)


def test_reference_recovers_the_planted_shares():
    """the figures of the module docstring: worst z 4.30, asserted at 4.55; the means within 0.01 of the planted share"""
    worst, ests = 0.0, {f: [] for f in pf.PLANT_FS}
    for seed in pf.PLANT_SEEDS:
        (L, N, coo, gt, a, b, f), ref = _planted(seed)
        mine = a != 255
        assert mine.sum() == pf.PLANT_PER_F * len(pf.PLANT_FS) and np.isfinite(ref["cell_se"][mine]).all()
        z = np.abs(ref["cell_frac"] - f) / ref["cell_se"]
        for fv in pf.PLANT_FS:
            m = f == fv
            ests[fv].append(ref["cell_frac"][m])
            print(f"seed {seed} f {fv}: mean {ref['cell_frac'][m].mean():.4f} median se {np.median(ref['cell_se'][m]):.4f} worst z {z[m].max():.2f}")
        worst = max(worst, float(z[mine].max()))
        # concavity: the second divided differences of every planted cell's profile are negative
        d = np.diff(ref["ll"][mine], axis=1) / np.diff(pf.DEFAULT_GRID.astype(pf.LD))
        assert (np.diff(d, axis=1) < 0).all()
    print(f"worst |estimate - f| / se = {worst:.2f}")
    assert worst <= WORST_Z + 0.25
    for fv in pf.PLANT_FS:
        mean = np.concatenate(ests[fv]).mean()
        assert abs(mean - fv) < 0.01, (fv, mean)


def test_kinds_of_the_planted_cells():
    low = []
    for seed in pf.PLANT_SEEDS:
        (L, N, coo, gt, a, b, f), ref = _planted(seed)
        assert (ref["kind"][f == 1.0] == 1).all(), ref["cell_frac"][f == 1.0].min()
        assert (ref["kind"][(f == 0.5) | (f == 0.3)] == 0).all()
        assert (ref["kind"][a == 255] == 255).all() and np.isnan(ref["cell_frac"][a == 255]).all()
        low.append(ref["kind"][f == 0.15])
    low = np.concatenate(low)
    print(f"planted at 0.15: {(low == 0).sum()} balanced, {(low == 2).sum()} toward b, {((low != 0) & (low != 2)).sum()} other")


def test_twin_finds_the_references_estimates():
    """The twin's sums carry (n + 1) u of rounding, near 1e-13 on a profile whose steps are near 0.1: the vertex moves by a share of the
    se far below 1e-6.  The same grid cell, the same kind wherever the reference's estimate is not within 1e-6 of a threshold."""
    (L, N, coo, gt, a, b, f), ref = _planted(0)
    A, R = dr.totals(L, coo)
    tw = pair_fraction.pair_fractions(cluster.Matrix(L, N, coo), gt.T, a, b, None, A, R)
    mine = a != 255
    assert np.array_equal(tw["j_star"][mine], ref["j_star"][mine])
    assert (np.abs(tw["cell_frac"][mine] - ref["cell_frac"][mine]) < 1e-6 * ref["cell_se"][mine]).all()
    assert (np.abs(tw["cell_se"][mine] - ref["cell_se"][mine]) < 1e-6 * ref["cell_se"][mine]).all()
    clear = mine & (np.abs(ref["cell_frac"] - 0.1) > 1e-6) & (np.abs(ref["cell_frac"] - 0.9) > 1e-6)
    assert np.array_equal(tw["kind"][clear], ref["kind"][clear]) and (tw["kind"][~mine] == 255).all()
    assert tw["summary"]["n_none"] == (~mine).sum()


def test_a_pair_that_shares_every_genotype_is_flat():
    """theta is (f x) + ((1 - f) x), x only up to a rounding that differs with f: the profile is noise of a few ulps, which the vertex
    rule's "unresolved" floor calls flat: se = +inf, kind 3, the estimate a grid point"""
    L, N, coo = dr.case_matrix()
    A, R = dr.totals(L, coo)
    gt = dr.case_gt(3)
    gt[2] = gt[0]
    a, b = np.zeros(N, np.uint8), np.full(N, 2, np.uint8)
    _, mat = _mat(False)
    tw = pair_fraction.pair_fractions(mat, gt.T, a, b, None, A, R)
    ref = pf.estimate_reference(L, N, coo, gt, a, b)
    has = ref["n_entries"] > 0
    for got in (tw, ref):
        assert (got["cell_se"][has] == np.inf).all() and (got["kind"][has] == 3).all() and (got["kind"][~has] == 255).all()
        assert np.isin(got["cell_frac"][has], pf.DEFAULT_GRID).all()
    spread = (ref["ll"].max(axis=1) - ref["ll"].min(axis=1)).astype(np.float64)
    assert (spread[has] <= 2.0 ** -40 * np.abs(ref["ll"][has, 8]).astype(np.float64)).all()
    # against a donor that differs the same cells are resolved
    ref = pf.estimate_reference(L, N, coo, dr.case_gt(3), a, b)
    inf = pf.informative(N, coo, dr.case_gt(3), a, b, A, R, 0.01, 0.03)
    assert np.isfinite(ref["cell_se"][inf]).all() and (ref["kind"][inf] != 3).all() and inf.sum() > 0.8 * has.sum()
