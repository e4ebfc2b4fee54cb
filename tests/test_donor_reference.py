"""CPU: the numpy twin of the donor calls (cellector_amd/donors.py) against the 80-bit statement of the model in
tests/donor_reference.py, the tables against mpmath, the (x + x) / 2 invariant, the share of cells the bounds leave undecided on the
GPU test's inputs, and the planted pool: the reference finds every planted singlet's donor and every planted doublet's pair.

The planted pool is the 900 x 600 three-genotype mixture of the refine tests at its own depth (~240 entries per cell, totals
1 + Geometric(0.7)) with 60 cross-genotype doublets, the donors' genotypes called from the planted classes, a decoy donor and 10 % of
the calls blanked.  The reference reaches every assertion below at that depth: the depth was not raised.
"""
import numpy as np
import pytest

import class_reference as cr
import donor_reference as dr
from cellector_amd import cluster, donors

_memo = {}


def _once(key, fn):
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def _twin_and_reference(D, masked, prior, anchor_kind, **prm):
    L, N, coo = dr.case_matrix()
    gt = dr.case_gt(D)
    mask = dr.case_mask() if masked else None
    A, R = dr.totals(L, coo)
    lp = dr.case_prior(D) if prior else None
    mat = _once(("mat", masked), lambda: cluster.Matrix(L, N, coo, mask))
    anchor = None
    if anchor_kind == "worst":
        first = donors.posteriors(mat, gt, A, R, lp)
        anchor = np.argmin(np.where(np.isfinite(first["x"]), first["x"], np.inf), axis=1).astype(np.uint8)
    elif anchor_kind == "mod":
        anchor = (np.arange(N) % D).astype(np.uint8)
    got = donors.posteriors(mat, gt, A, R, lp, anchor, **prm)
    ref = dr.reference(L, N, coo, gt, got["tab1"], got["tab2"], lp, got["anchor"], mask, **prm)
    return got, ref, (L, N, coo, gt, mask, A, R)


@pytest.mark.parametrize("D", dr.DONORS)
@pytest.mark.parametrize("masked", [False, True], ids=["all-loci", "masked"])
def test_twin_is_inside_the_references_bounds(D, masked):
    for prior, anchor_kind, prm in ((False, "best", {}), (True, "worst", dict(doublet_rate=0.3, posterior_threshold=0.9, min_loci=3)),
                                    (False, "mod", dict(doublet_rate=0.0))):
        got, ref, _ = _twin_and_reference(D, masked, prior, anchor_kind, **prm)
        res, undecided = dr.compare(ref, got)
        print(D, masked, prior, anchor_kind, {k: round(v, 3) for k, v in res.items()}, "undecided", int(undecided.sum()))
        assert max(res.values()) <= 1.0, res
        # the bounds leave under 1 % of the cells undecided on the inputs the GPU test uses
        assert undecided.sum() < 0.01 * len(undecided), undecided.sum()
        n = len(got["best"])
        assert np.array_equal(got["posterior"].shape, (n, D))
        if anchor_kind == "best":
            assert np.array_equal(got["anchor"], got["best"])
        # the anchor's pair column is its singlet sum, bit for bit, and takes no part in the chain
        r = np.arange(n)
        assert got["pair_ll"][r, got["anchor"]].tobytes() == got["ll"][r, got["anchor"]].tobytes()
        assert (got["pair_posterior"][r, got["anchor"]] == 0).all()
        total = got["posterior"].sum(axis=1) + got["doublet_posterior"]
        assert (np.abs(total - 1.0) <= (2 * D + 4) * np.spacing(1.0)).all()
        empty = ref["n_entries"] == 0
        assert empty.any() and (got["ll"][empty] == 0).all() and (got["status"][empty] == 255).all()
        if D == 1 or anchor_kind == "mod":
            assert (got["doublet_posterior"] == 0).all()
        if D == 1:
            assert (got["second"] == 255).all() and (got["best_pair"] == 255).all()


def test_tables_against_mpmath_and_the_half_sum_invariant():
    mpmath = pytest.importorskip("mpmath")
    L, N, coo = dr.case_matrix()
    A, R = dr.totals(L, coo)
    mask = dr.case_mask()
    for err, ambient in ((0.01, 0.03), (0.2, 0.0), (1e-6, 0.9)):
        tab1, tab2 = donors.tables(A, R, err, ambient, mask)
        res = dr.compare_tabs(A, R, err, ambient, mask, tab1, tab2)
        assert max(res.values()) <= 1.0, res
        assert (tab1[mask == 0] == 0).all() and (tab2[mask == 0] == 0).all()
        for g in range(4):
            assert tab2[:, 5 * g].tobytes() == tab1[:, g].tobytes()  # (x + x) 0.5 == x
        th = dr.theta_double(A, R, err, ambient)
        with mpmath.workprec(200):
            for l in (0, 1, 7, 100, L - 1):
                if not mask[l]:
                    continue
                for g in range(4):
                    for b in range(4):
                        t = 0.5 * (th[l, g] + th[l, b])
                        for j, v in enumerate((mpmath.log(mpmath.mpf(float(t))), mpmath.log(mpmath.mpf(float(1.0 - t))))):
                            assert abs(mpmath.mpf(float(tab2[l, 4 * g + b, j])) - v) <= dr.C_LOG * dr.U * abs(v), (l, g, b, j)
        # theta stays inside (0, 1): every logarithm is finite
        assert np.isfinite(tab1).all() and np.isfinite(tab2).all() and (tab1[mask != 0] < 0).all()


def test_packing_is_two_bits_per_donor():
    for D in dr.DONORS:
        gt = dr.case_gt(D)
        ids = np.arange(3, dr.CASE_L, 2)
        packed = donors.pack(gt, ids)
        assert packed.shape == (len(ids), (D + 31) // 32)
        assert np.array_equal(packed, dr.pack_reference(gt[:, ids]))
        assert np.array_equal(donors.unpack(packed, D), gt[:, ids].T)


def test_match_sums_are_inside_the_references_bounds():
    L, N, coo = dr.case_matrix()
    A, R = dr.totals(L, coo)
    labels = (np.arange(N) % 5).astype(np.uint8)
    labels[::7] = 255
    labels[labels == 3] = 255  # class 3 has no cell
    cells, alt, ref = (x[:5] for x in cr.tallies(L, coo, labels, 5))
    for D in (1, 3, 33, 64):
        gt = dr.case_gt(D)
        for mask in (None, dr.case_mask()):
            got = donors.match(alt, ref, cells, gt, A, R, mask)
            want, B = dr.match_reference(alt, ref, donors.tables(A, R, mask=mask)[0], gt, mask)
            assert dr._ratio(got["ll"], want, B) <= 1.0
            assert got["best"][3] == 255 and got["margin"][3] == 0 and (got["best"][[0, 1, 2, 4]] < D).all()
            assert (got["margin"] >= 0).all() and (np.isinf(got["margin"][[0, 1, 2, 4]]).all() if D == 1 else True)


def test_reference_recovers_the_planted_pool():
    L, N, coo, gt, truth, par = dr.planted_pool()
    A, R = dr.totals(L, coo)
    tab1, tab2 = donors.tables(A, R)
    ref = dr.reference(L, N, coo, gt, tab1, tab2)
    single = np.arange(cr.MIX_N)
    assert np.array_equal(ref["best"][single], truth[single]), int((ref["best"][single] != truth[single]).sum())
    assert (ref["status"][single] == 0).all(), np.bincount(ref["status"][single], minlength=3)
    dbl = np.arange(N - len(par), N)
    assert (ref["status"][dbl] == 1).all(), np.bincount(ref["status"][dbl], minlength=3)
    pair = np.sort(np.stack([ref["anchor"][dbl], ref["best_pair"][dbl]], axis=1), axis=1)
    assert np.array_equal(pair, par), int((pair != par).any(axis=1).sum())
    assert (ref["best"] != 3).all() or (ref["best"][single] != 3).all()  # nobody is the decoy
    # the twin agrees with it on every cell here, and a class labelling names its donors
    got = donors.posteriors(cluster.Matrix(L, N, coo), gt, A, R)
    res, undecided = dr.compare(ref, got)
    assert max(res.values()) <= 1.0 and not undecided[single].any(), res
    labels = truth.copy()
    cells, alt, refc = (x[:3] for x in cr.tallies(L, coo, labels, 3))
    m = donors.match(alt, refc, cells, gt, A, R)
    assert m["best"].tolist() == [0, 1, 2] and (m["margin"] > 100).all()
