"""CPU: the numpy twin of the donor panel (cellector_amd/donors.py: panel_shortlist, panel_posteriors, panel_present) against the
80-bit statement in tests/donor_panel_reference.py at every (D, M) of the GPU test, its equality with donors.posteriors where the
panel model reduces to the 64-donor one, and the planted claim: the three donors of the planted pool hidden among 97 and 297 decoys
are found, every planted doublet is called with its planted pair, and no decoy gets a status-0 cell.
"""
import numpy as np
import pytest

import class_reference as cr
import donor_panel_reference as pn
import donor_reference as dr
from cellector_amd import cluster, donors

_memo = {}


def _once(key, fn):
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def _case(masked):
    L, N, coo = dr.case_matrix()
    mask = dr.case_mask() if masked else None
    A, R = dr.totals(L, coo)
    return L, N, coo, mask, A, R, _once(("mat", masked), lambda: cluster.Matrix(L, N, coo, mask))


def _shared(D, masked):
    """what depends on (D, mask, prior) alone, kept for the latest such key: the 4096-donor reference is 200 MB"""
    key = (D, masked)
    if _memo.get("shared_key") != key:
        L, N, coo, mask, A, R, mat = _case(masked)
        gt = dr.case_gt(D)
        lp = pn.case_prior(D, 3) if masked else None
        tab1, tab2 = donors.tables(A, R, mask=mask)
        _memo["shared"] = (gt, lp, tab1, tab2, donors.singlet_sums(mat, tab1, gt.T), pn.singlets(L, N, coo, gt, tab1, lp, mask, tab2))
        _memo["shared_key"] = key
    return _memo["shared"]


def _twin_against_reference(D, M, masked, **prm):
    L, N, coo, mask, A, R, mat = _case(masked)
    gt, lp, tab1, tab2, s, S = _shared(D, masked)
    got = donors.panel_posteriors(mat, gt, A, R, M, lp, tab1=tab1, tab2=tab2, s=s, **prm)
    Ma = min(M, D)
    assert got["cand"].shape == (N, Ma) and got["cand"].dtype == np.uint16
    assert (np.diff(got["cand"].astype(np.int64), axis=1) > 0).all() and (got["cand"] < D).all()
    ref = pn.chain(S, tab2, M, got["anchor"], got["cand"], **prm)
    res, undecided = pn.compare(ref, got)
    print(D, M, masked, {k: round(v, 3) for k, v in res.items()}, "undecided", int(undecided.sum()))
    assert max(res.values()) <= 1.0, res
    # the bounds leave under 1 % of the cells undecided on the inputs the GPU test uses
    assert undecided.sum() < 0.01 * N, (D, M, int(undecided.sum()))
    at = got["cand"] == got["anchor"][:, None]
    assert got["cand_pair_ll"][at].tobytes() == got["cand_ll"][at].tobytes() and (got["cand_pair_posterior"][at] == 0).all()
    assert at.any(axis=1).all() and np.array_equal(got["anchor"], got["best"])  # (the best singlet is always shortlisted)
    if D == 1:
        assert (got["second"] == 65535).all() and (got["best_pair"] == 65535).all() and (got["doublet_posterior"] == 0).all()
    if Ma == 1:
        assert (got["best_pair"] == 65535).all()
    sm, st = got["summary"], got["status"]
    assert [sm["n_singlet"], sm["n_doublet"], sm["n_ambiguous"], sm["n_unassigned"]] == [int((st == v).sum()) for v in (0, 1, 2, 255)]
    assert np.array_equal(got["donor_cells"], np.bincount(got["best"][st == 0], minlength=D))
    assert np.array_equal(donors.panel_present(got), np.flatnonzero(got["donor_cells"]))
    assert donors.panel_present(got, 2).tolist() == np.flatnonzero(got["donor_cells"] >= 2).tolist()


@pytest.mark.parametrize("M", pn.SHORTLISTS)
@pytest.mark.parametrize("D", pn.DONORS)
def test_twin_is_inside_the_references_bounds(D, M):
    """every (D, M) of the GPU test, M > D included: the flat prior, all loci, default parameters"""
    _twin_against_reference(D, M, False)


@pytest.mark.parametrize("M", [2, 8, 64])
@pytest.mark.parametrize("D", [2, 33, 65, 129, 1000])
def test_twin_under_a_mask_and_a_prior_with_donors_ruled_out(D, M):
    _twin_against_reference(D, M, True, doublet_rate=0.3, posterior_threshold=0.9, min_loci=3)


def test_shortlist_order_and_ties():
    u = np.array([[1.0, 3.0, 3.0, -np.inf, 2.0, -np.inf], [-np.inf, -np.inf, 0.0, -np.inf, -np.inf, -np.inf]])
    assert donors.panel_shortlist(u, 1).tolist() == [[1], [2]]
    assert donors.panel_shortlist(u, 2).tolist() == [[1, 2], [0, 2]]
    assert donors.panel_shortlist(u, 3).tolist() == [[1, 2, 4], [0, 1, 2]]
    assert donors.panel_shortlist(u, 5).tolist() == [[0, 1, 2, 3, 4], [0, 1, 2, 3, 4]]
    assert donors.panel_shortlist(u, 64).tolist() == [list(range(6))] * 2


@pytest.mark.parametrize("D", [1, 2, 33, 64])
@pytest.mark.parametrize("masked", [False, True], ids=["all-loci", "masked"])
def test_twin_equals_the_64_donor_twin_bit_for_bit(D, masked):
    """with D <= 64 and shortlist >= D the panel model IS the donor model: every common output, indices widened"""
    L, N, coo, mask, A, R, mat = _case(masked)
    gt = dr.case_gt(D)
    for lp, anchor, prm in ((None, None, {}), (dr.case_prior(D), (np.arange(N) % D), dict(doublet_rate=0.3, posterior_threshold=0.9, min_loci=3)),
                            (None, None, dict(doublet_rate=0.0))):
        want = donors.posteriors(mat, gt, A, R, lp, None if anchor is None else anchor.astype(np.uint8), **prm)
        got = donors.panel_posteriors(mat, gt, A, R, 64, lp, anchor, **prm)
        assert np.array_equal(got["cand"], np.tile(np.arange(D, dtype=np.uint16), (N, 1)))
        for a, b in (("ll", "ll"), ("cand_ll", "ll"), ("cand_pair_ll", "pair_ll"), ("cand_posterior", "posterior"),
                     ("cand_pair_posterior", "pair_posterior"), ("doublet_posterior", "doublet_posterior")):
            assert got[a].tobytes() == want[b].tobytes(), (a, D)
        assert got["best_posterior"].tobytes() == want["posterior"][np.arange(N), want["best"]].tobytes()
        for k in ("best", "second", "best_pair", "anchor"):
            assert np.array_equal(got[k], np.where(want[k] == 255, 65535, want[k].astype(np.uint16))), k
        assert np.array_equal(got["status"], want["status"]) and np.array_equal(got["n_entries"], want["n_entries"])
        assert np.array_equal(got["donor_cells"], want["summary"]["donor_cells"])


@pytest.mark.parametrize("D", [100, 300])
@pytest.mark.parametrize("seed", [5, 6, 7])
def test_the_planted_donors_are_found_in_a_panel(seed, D):
    L, N, coo, gt, rows, truth, par = pn.planted_panel(seed, D)
    A, R = dr.totals(L, coo)
    tab1, tab2 = donors.tables(A, R)
    mat = _once(("pool", seed), lambda: cluster.Matrix(L, N, coo))
    got = donors.panel_posteriors(mat, gt, A, R, 8, tab1=tab1, tab2=tab2)
    S = pn.singlets(L, N, coo, gt, tab1)
    ref = pn.chain(S, tab2, 8, got["anchor"], got["cand"])
    res, undecided = pn.compare(ref, got)
    print(seed, D, {k: round(v, 3) for k, v in res.items()}, "undecided", int(undecided.sum()), np.bincount(got["status"], minlength=3))
    assert max(res.values()) <= 1.0, res
    single, dbl = np.arange(cr.MIX_N), np.arange(N - len(par), N)
    for out in (got, ref):
        assert np.array_equal(out["best"][single], rows[truth[single]]), int((out["best"][single] != rows[truth[single]]).sum())
        assert (out["status"][single] == 0).all(), np.bincount(out["status"][single], minlength=3)
        assert (out["status"][dbl] == 1).all(), np.bincount(out["status"][dbl], minlength=3)
        pair = np.sort(np.stack([out["anchor"][dbl], out["best_pair"][dbl]], axis=1), axis=1)
        assert np.array_equal(pair, rows[par]), int((pair != rows[par]).any(axis=1).sum())
        decoy = ~np.isin(out["best"], rows)
        assert not (decoy & (out["status"] == 0)).any()
    assert np.array_equal(donors.panel_present(got), rows)
    assert got["summary"]["n_present"] == 3 and donors.panel_present(got, 10 ** 6).size == 0
