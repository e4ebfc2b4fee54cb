"""CPU: the numpy twin of the donor fit (cellector_amd/donors.py: moment_tables, fit_sums, fit) against the 80-bit statement of the
model in tests/donor_fit_reference.py; the moment tables against mpmath; the diagonal invariant; the share of cells the bounds leave
undecided on the GPU test's inputs; what one dropped entry does to the sums; and the planted pool with one of its donors withheld:
at the default parameters the reference flags every singlet of the withheld donor and no cell the remaining donors explain.

Realised margins of the planted pools (printed by test_reference_flags_the_cells_of_a_withheld_donor; DESIGN.md 3.2q holds a copy):
the z of the called hypothesis of the kept cells, the z of the withheld singlets, each against the run's threshold.
"""
import numpy as np
import pytest

import class_reference as cr
import donor_fit_reference as fr
import donor_reference as dr
from cellector_amd import cluster, donors

_memo = {}
# (prior, anchor, the donor call's parameters, the fit's): the three variants of test_donor_reference.py, and one whose calls leave
# hundreds of status-0 cells at every D, at the fit's defaults.  The three form a threshold from 64 keys on: their calls leave a
# dozen keys at some D, one cell of undecided status then moves a quartile by a whole key spacing, and the reference decides no flag
# near it (the cap on undecided cells below is a condition on the inputs).
VARIANTS = ((False, "best", {}, dict(min_cells=64)),
            (True, "worst", dict(doublet_rate=0.3, posterior_threshold=0.9, min_loci=3), dict(min_cells=64)),
            (False, "mod", dict(doublet_rate=0.0), dict(min_cells=64, iqr_multiple=1.5)),
            (False, "best", dict(doublet_rate=0.02, posterior_threshold=0.5), {}))


def _once(key, fn):
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def _twin_and_reference(D, masked, prior, anchor_kind, prm, fit):
    """the twin's fit and the reference's on donor_reference's case, under the (prior, anchor) variants of test_donor_reference.py"""
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
    got = donors.fit(mat, gt, A, R, lp, anchor, **prm, **fit)
    call = dr.reference(L, N, coo, gt, got["call"]["tab1"], got["call"]["tab2"], lp, got["call"]["anchor"], mask, **prm)
    ref = fr.reference(L, N, coo, gt, call, got["mom1"], got["mom2"], mask, **fit)
    return got, ref, call


@pytest.mark.parametrize("D", dr.DONORS)
@pytest.mark.parametrize("masked", [False, True], ids=["all-loci", "masked"])
def test_twin_is_inside_the_references_bounds(D, masked):
    for prior, anchor_kind, prm, fit in VARIANTS:
        got, ref, call = _twin_and_reference(D, masked, prior, anchor_kind, prm, fit)
        res, undecided = fr.compare(ref, got)
        print(D, masked, prior, anchor_kind, {k: round(v, 3) for k, v in res.items()}, "undecided", int(undecided.sum()),
              "threshold", float(ref["threshold"]), "interval", ref["t_lo"], ref["t_hi"], "keys", len(ref["keys"]))
        assert max(res.values()) <= 1.0, res
        # the bounds leave under 1 % of the cells undecided on the inputs the GPU test uses: the reference alone decides that
        assert undecided.sum() < 0.01 * len(undecided), int(undecided.sum())
        n = len(got["call_z"])
        r = np.arange(n)
        a = got["call"]["anchor"]
        for x, y in (("pair_e", "fit_e"), ("pair_v", "fit_v")):  # mom2[l][5 g] is mom1[l][g]: the anchor's pair column is its singlet's
            assert got[x][r, a].tobytes() == got[y][r, a].tobytes()
        empty = call["n_entries"] == 0
        assert empty.any() and (got["fit_v"][empty] == 0).all() and (got["z"][empty] == 0).all() and (got["unmatched"][empty] == 0).all()
        assert (got["call_z"][got["status"] == 255] == 0).all() and (got["unmatched"][got["status"] == 255] == 0).all()
        assert (got["hyp_b"][got["status"] != 1] == 255).all() and (got["hyp_b"][got["status"] == 1] != 255).all()
        if D == 1:
            assert (got["hyp_b"] == 255).all() and (got["hyp_a"] == 0).all()
        sm = got["summary"]
        assert sm["n_keys"] == int((got["status"] == 0).sum()) == len(ref["keys"])
        assert sm["n_unmatched"] == int(got["unmatched"].sum()) == sm["n_unmatched_singlet"] + sm["n_unmatched_doublet"] + sm["n_unmatched_ambiguous"]
        if sm["n_keys"] >= fit.get("min_cells", 8):
            want = fr.order_statistics(got["call_z"][got["status"] == 0], fit.get("iqr_multiple", 3.0))
            for name, w in zip(("median", "iqr", "threshold"), want):
                assert abs(sm[name] - float(w)) <= 16 * np.spacing(max(abs(float(x)) for x in want)), name
        else:
            assert sm["threshold"] == -np.inf and np.isnan(sm["median"]) and np.isnan(sm["iqr"]) and sm["n_unmatched"] == 0


def test_moment_tables_against_mpmath_and_the_diagonal_invariant():
    L, N, coo = dr.case_matrix()
    A, R = dr.totals(L, coo)
    mask = dr.case_mask()
    for err, ambient in ((0.01, 0.03), (0.2, 0.0), (1e-6, 0.9)):
        mom1, mom2 = donors.moment_tables(A, R, err, ambient, mask)
        res = fr.compare_moms(A, R, err, ambient, mask, mom1, mom2)
        print(err, ambient, res)
        assert max(res.values()) <= 1.0, res
        assert (mom1[mask == 0] == 0).all() and (mom2[mask == 0] == 0).all()
        for g in range(4):
            assert mom2[:, 5 * g].tobytes() == mom1[:, g].tobytes()  # (x + x) 0.5 == x
        # a mean of logs of probabilities is below 0, a variance is not; theta = 0.5 has d = 0 and v = 0
        assert (mom1[mask != 0][:, :, 0] < 0).all() and (mom1[:, :, 1] >= 0).all() and (mom2[:, :, 1] >= 0).all()
        assert np.isfinite(mom1).all() and np.isfinite(mom2).all()
    mpmath = pytest.importorskip("mpmath")
    for err, ambient in ((0.01, 0.03), (0.2, 0.0), (1e-6, 0.9)):
        mom1, mom2 = donors.moment_tables(A, R, err, ambient, mask)
        th = dr.theta_double(A, R, err, ambient)
        _, _, (_, b2) = fr.mom_reference(A, R, err, ambient, mask)
        with mpmath.workprec(200):
            for l in (0, 1, 7, 100, L - 1):
                if not mask[l]:
                    continue
                for g in range(4):
                    for b in range(4):
                        t = 0.5 * (th[l, g] + th[l, b])
                        t, rest = mpmath.mpf(float(t)), mpmath.mpf(float(1.0 - t))
                        la, lb = mpmath.log(t), mpmath.log(rest)
                        want = (t * la + rest * lb, t * rest * (la - lb) ** 2)
                        for j in range(2):
                            assert abs(mpmath.mpf(float(mom2[l, 4 * g + b, j])) - want[j]) <= b2[l, 4 * g + b, j], (l, g, b, j)


def test_one_dropped_entry_moves_the_sums_by_more_than_100_bounds():
    """every cell with an entry of total > 0 (a locus' h is never 0): without that entry E differs by more than 100 of its bounds"""
    L, N, coo = dr.case_matrix()
    A, R = dr.totals(L, coo)
    D = 5
    gt = dr.case_gt(D)
    mom1, mom2 = donors.moment_tables(A, R)
    anchor = (np.arange(N) % D).astype(np.uint8)
    lo, ce, al, re = coo
    live = np.flatnonzero((al + re) > 0)
    first = live[np.unique(ce[live], return_index=True)[1]]  # one entry of total > 0 per cell that has one
    keep = np.ones(len(lo), bool)
    keep[first] = False
    (E, V, PE, PV), (B_E, B_V, B_PE, B_PV) = fr.sums_reference(N, coo, gt, mom1, mom2, anchor)
    (E2, V2, PE2, PV2), _ = fr.sums_reference(N, [x[keep] for x in coo], gt, mom1, mom2, anchor)
    cells = ce[first]
    assert len(cells) > 0.85 * N
    for full, less, B in ((E, E2, B_E), (PE, PE2, B_PE)):
        moved = np.abs(full - less).astype(np.float64)[cells]
        assert (moved > 100 * B[cells]).all(), float((moved / B[cells]).min())
    # the variance moves as far except where the dropped entry's theta lies at 0.5 (d = 0, v = 0: a het call, or a no-call at a balanced
    # locus); the twin sees the same change
    movedV = np.abs(V - V2).astype(np.float64)[cells]
    assert (movedV > 100 * B_V[cells]).mean() > 0.9
    mat2 = cluster.Matrix(L, N, [x[keep] for x in coo])
    tw = donors.fit_sums(cluster.Matrix(L, N, coo), mom1, mom2, gt.T, anchor)
    tw2 = donors.fit_sums(mat2, mom1, mom2, gt.T, anchor)
    assert (np.abs(tw[0] - tw2[0])[cells] > 100 * B_E[cells]).all()
    other = np.setdiff1d(np.arange(N), cells)
    assert tw[0][other].tobytes() == tw2[0][other].tobytes()


def _pool_run(seed, withheld):
    """the reference's fit of the planted pool with donor `withheld` (None: nobody) taken out of gt"""
    L, N, coo, gt, truth, par = dr.planted_pool(seed)
    A, R = dr.totals(L, coo)
    rows = [d for d in range(len(gt)) if d != withheld]
    g = gt[rows]
    tab1, tab2 = _once(("tabs", seed), lambda: donors.tables(A, R))
    mom1, mom2 = _once(("moms", seed), lambda: donors.moment_tables(A, R))
    call = dr.reference(L, N, coo, g, tab1, tab2)
    return fr.reference(L, N, coo, g, call, mom1, mom2), truth, par, N


@pytest.mark.parametrize("seed", [5, 6, 7])
def test_reference_flags_the_cells_of_a_withheld_donor(seed):
    for withheld in (None, 0, 1, 2):
        ref, truth, par, N = _pool_run(seed, withheld)
        flags = ref["unmatched"] != 0
        single = np.arange(cr.MIX_N)
        dbl = np.arange(N - len(par), N)
        lost = single[truth[single] == withheld] if withheld is not None else single[:0]
        kept = np.setdiff1d(single, lost)
        dbl_lost = dbl[(par == withheld).any(axis=1)] if withheld is not None else dbl[:0]
        dbl_kept = np.setdiff1d(dbl, dbl_lost)
        cz, thr = ref["call_z"].astype(np.float64), float(ref["threshold"])
        explained = np.concatenate([kept, dbl_kept])
        print(f"seed {seed} withheld {withheld}: keys {len(ref['keys'])} median {float(ref['median']):.3f} iqr {float(ref['iqr']):.3f} "
              f"threshold {thr:.3f} [{ref['t_lo']:.3f}, {ref['t_hi']:.3f}]; lowest kept z {cz[explained].min():.3f} "
              f"(margin {cz[explained].min() - thr:.3f}); "
              + (f"highest withheld singlet z {cz[lost].max():.3f} (margin {thr - cz[lost].max():.3f}), median {np.median(cz[lost]):.1f}; "
                 f"doublets with the withheld parent flagged {int(flags[dbl_lost].sum())} of {len(dbl_lost)}, their z "
                 f"{cz[dbl_lost].min():.2f} .. {cz[dbl_lost].max():.2f}" if withheld is not None else "nobody withheld")
              + f"; status of the withheld singlets {np.bincount(ref['status'][lost], minlength=3).tolist()}")
        assert flags[lost].all(), int((~flags[lost]).sum())
        assert not flags[kept].any(), int(flags[kept].sum())
        assert not flags[dbl_kept].any(), int(flags[dbl_kept].sum())
        if withheld is None:
            assert not flags.any()
        # the reference decides these flags by more than its bounds
        assert ref["flag_ok"][lost].all() and ref["flag_ok"][explained].all()


def test_twin_agrees_with_the_reference_on_a_planted_pool():
    L, N, coo, gt, truth, par = dr.planted_pool(5)
    A, R = dr.totals(L, coo)
    g = gt[[0, 2, 3]]
    got = donors.fit(cluster.Matrix(L, N, coo), g, A, R)
    call = dr.reference(L, N, coo, g, got["call"]["tab1"], got["call"]["tab2"])
    ref = fr.reference(L, N, coo, g, call, got["mom1"], got["mom2"])
    res, undecided = fr.compare(ref, got)
    assert max(res.values()) <= 1.0, res
    assert undecided.sum() < 0.01 * N
    assert np.array_equal(got["unmatched"][~undecided], ref["unmatched"][~undecided]) and got["unmatched"].sum() >= (truth == 1).sum()
