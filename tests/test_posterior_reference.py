"""The posterior phase's high-precision reference (tests/posterior_reference.py) checked on the CPU: its chain against mpmath, the
whole of it against the oracle, and — on every (matrix, exclusion set) case tests/test_gpu_posterior_sweep.py uses — that the
comparison it defines can see the doublet set: almost every cell's doublet_posterior is observable, a doublet sum that is off by
the cell's smallest term moves an output by more than 100 bounds, and a doublet sum that lacks one term is rejected."""
import warnings

import numpy as np
import pytest

import posterior_reference as pr
import tile_reference as tr

LD = np.longdouble
CASES = [(m, s) for m in pr.MATRICES for s in pr.set_names(m)]
G_CPU = {"row-lengths": 0, "tier2": 8, "shallow-ragged": 0, "second-trip": 0}  # t2_tiles of the widest geometry a case runs under


def _g(mname):
    """the largest number of partial sums any run of the GPU file gives this matrix (engine 1 has 6): the widest bound, hence the
    hardest one for the sensitivity claim"""
    return max(pr.WAVE_STEPS, pr.g_max(pr.matrix(mname)[0], G_CPU[mname]))


def test_alpha_betas_and_priors_on_the_clamps():
    """the edges of main.rs:240-259 as numbers: the empty set leaves minority alpha = beta = 1 to the bit and mf0 below both clamps;
    every cell excluded gives mf = 1, lp_maj = -inf and majority alpha = beta = 1; the doublet set takes the unclamped mf0"""
    L, N, coo, _ = pr.matrix("tier2")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for sname in pr.SETS:
            exc = pr.exclusion_set("tier2", sname)
            n = int(exc.sum())
            lc, alt_min, ref_min = pr.tallies(L, coo, exc)
            (a0, b0), (a1, b1), (a2, b2), (lp_min, lp_maj, lp_dbl) = pr.posterior_alpha_betas(lc, alt_min, ref_min, n, N)
            mf0 = pr.priors(n, N)[0]
            assert mf0 == (n + 1.0) / (N + 1.0)
            assert lp_min == np.log(max(mf0, 0.01)) and lp_dbl == np.log(N / 1000.0 / 100.0 * max(mf0, 0.1))
            assert np.array_equal(a2, (lc[:, 1] - alt_min) * mf0 + alt_min + 1.0)  # whole-number tallies: the same bits either way
            if sname == "empty":
                assert (a0 == 1.0).all() and (b0 == 1.0).all() and mf0 < 0.01 and lp_min == np.log(0.01)
                assert np.array_equal(a1, lc[:, 1] * 0.01 + 1.0)
            if sname == "below-0.01":
                assert mf0 < 0.01 and (n + 2.0) / (N + 1.0) >= 0.01 and lp_min == np.log(0.01)
            if sname == "above-0.01":
                assert 0.01 <= mf0 < 0.011 and lp_min == np.log(mf0)
            if sname == "planted":
                assert 0.01 < mf0 < 0.1 and lp_dbl == np.log(N / 1000.0 / 100.0 * 0.1)
            if sname == "above-0.1":
                assert mf0 > 0.1 and lp_dbl == np.log(N / 1000.0 / 100.0 * mf0)
            if sname == "all":
                assert mf0 == 1.0 and lp_maj == -np.inf and (a1 == 1.0).all() and (b1 == 1.0).all() and lp_min == 0.0
            else:
                assert np.isfinite(lp_maj)


def _chain_tolerance(ch, i):
    """the longdouble chain's own error: a dozen operations of 2^-64 relative, each at the size of the value it makes"""
    mags = [abs(float(ch[k][i])) for k in ("log_num", "log_maj", "log_dbl", "l1", "den") if np.isfinite(ch[k][i])]
    return 2.0 ** -64 * (2.0 * sum(mags) + 16.0)


def test_chain_against_mpmath():
    """420 cells of the row-length matrix under five sets, among them lp_maj = -inf (all), cells without entries, the cell whose
    log doublet_posterior is -677 (all-but-one), the largest and the smallest x_p and x_d of every set"""
    n_checked, seen_empty, seen_low = 0, 0, 0
    rng = np.random.default_rng(5)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # lp_maj = -inf must go through without a warning
        for sname in ("empty", "planted", "every-second", "all-but-one", "all"):
            ref = pr.case("row-lengths", sname)
            ch = ref["chain"]
            assert all(np.isfinite(ch[k]).all() for k in ("x_p", "x_d", "posterior", "doublet_posterior", "den")), sname
            pick = set(rng.choice(ref["N"], 70, replace=False).tolist())
            pick |= {int(np.argmin(ch["x_d"])), int(np.argmax(ch["x_d"])), int(np.argmin(ch["x_p"])), int(np.argmax(ch["x_p"]))}
            pick |= set(np.nonzero(ref["count"] == 0)[0][:10].tolist())
            s = [r["ll_ld"] for r in ref["sums"]]
            for i in sorted(pick):
                x_p, x_d = pr.chain_mp(s[0][i], s[1][i], s[2][i], ref["lp"])
                tol = _chain_tolerance(ch, i)
                assert abs(float(pr._mpf(ch["x_p"][i]) - x_p)) <= tol, (sname, i, float(ch["x_p"][i]), float(x_p), tol)
                assert abs(float(pr._mpf(ch["x_d"][i]) - x_d)) <= tol, (sname, i, float(ch["x_d"][i]), float(x_d), tol)
                n_checked += 1
                seen_empty += int(ref["count"][i] == 0)
                seen_low += int(min(float(x_p), float(x_d)) < -650.0)
            if sname == "all":
                assert ref["lp"][1] == -np.inf and (ch["log_maj"] == -np.inf).all() and np.array_equal(ch["l1"], ch["log_num"])
    assert n_checked >= 400 and seen_empty >= 10 and seen_low >= 1, (n_checked, seen_empty, seen_low)


def test_a_cell_without_entries_has_the_priors_quotient():
    """s = 0 in all three sets: posterior = mf / (mf + (1 - mf) + doublet prior), the same for every such cell"""
    for sname in ("empty", "planted", "all"):
        ref = pr.case("row-lengths", sname)
        empty = ref["count"] == 0
        assert empty.sum() > 1000
        pri = np.exp(np.asarray(ref["lp"], LD))
        want = pri[0] / pri.sum()
        got = ref["chain"]["posterior"][empty]
        assert (got == got[0]).all() and abs(float(got[0] / want) - 1.0) < 2.0 ** -60
        assert all((r["ll"][empty] == 0).all() and (r["b_ll"][empty] == 0).all() for r in ref["sums"])


@pytest.mark.parametrize("mname", pr.MATRICES)
def test_reference_against_the_oracle(oracle_lib, mname):
    """the set the oracle's own EM run reaches; Oracle.posteriors() at the tolerances every comparison with the oracle uses: 1e-7 on
    the sums, 1e-6 on the posteriors"""
    ob = oracle_lib
    L, N, coo, _ = pr.matrix(mname)
    ob.set_threads(ob.host_threads())
    try:
        o = ob.Oracle.from_coo(L, N, *(np.ascontiguousarray(x, np.uint32) for x in coo), 0, 0)
        o.run(5.0, 30)
        exc = o.excluded() != 0
        assert 0 < exc.sum() < N
        po = o.posteriors()
        o.close()
    finally:
        ob.set_threads(1)
    ref = pr.reference(L, N, coo, exc)
    np.testing.assert_allclose(ref["sums"][0]["ll"], po["ll_minority"], rtol=0, atol=1e-7)
    np.testing.assert_allclose(ref["sums"][1]["ll"], po["ll_majority"], rtol=0, atol=1e-7)
    np.testing.assert_allclose(ref["chain"]["posterior"].astype(np.float64), po["posterior"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(ref["chain"]["doublet_posterior"].astype(np.float64), po["doublet_posterior"], rtol=0, atol=1e-6)


@pytest.mark.parametrize("mname,sname", CASES, ids=[f"{m}/{s}" for m, s in CASES])
def test_the_doublet_set_is_visible(mname, sname):
    """Observability: at most 0.1 % of the cells have a reference doublet_posterior below 1e-290 (the GPU test could not see the
    doublet sum in them), and in the row-length matrix every row length keeps an observable cell.
    Sensitivity: s_dbl shifted by the smallest |term| of the cell's doublet terms moves posterior or doublet_posterior by more than
    100 bounds, in every cell with a non-zero term and an observable doublet_posterior.
    The bound holds an honest evaluation: the device's operations in numpy doubles, from the sums rounded to double, pass compare().
    Mutant: the same evaluation from a doublet sum that lacks its smallest term is rejected in every one of those cells, by the
    posteriors alone (ll_minority and ll_majority are untouched and stay inside)."""
    ref = pr.case(mname, sname)
    G = _g(mname)
    ch = ref["chain"]
    hidden = ch["doublet_posterior"] < pr.OBSERVABLE
    assert hidden.sum() <= 0.001 * ref["N"], (mname, sname, int(hidden.sum()))
    if mname == "row-lengths":
        import test_gpu_tile_sweep as S
        coo = S._row_length_coo()[2]
        ks = np.bincount(coo[1][(coo[0] >= pr.BLU) & (coo[0] < 2 * pr.BLU)], minlength=ref["N"])
        for k in np.unique(ks):
            assert (~hidden[ks == k]).any(), (sname, int(k))
    cells, moved = pr.sensitivity(ref, G)
    assert cells.sum() >= 0.7 * ref["N"]
    assert (moved[cells] > 100.0).all(), (mname, sname, float(moved[cells].min()))

    s = [r["ll"] for r in ref["sums"]]
    p, d = pr.chain_double(*s, ref["lp"])
    honest = dict(ll_minority=s[0], ll_majority=s[1], posterior=p, doublet_posterior=d)
    res = pr.compare(ref, honest, G)
    assert all(bad.size == 0 for _, bad in res.values()), pr.describe(ref, honest, res, G)
    honest_worst = max(w for w, _ in res.values())
    s_mut = (ref["sums"][2]["ll_ld"] + np.where(cells, ref["min_term"], 0.0).astype(LD)).astype(np.float64)
    p, d = pr.chain_double(s[0], s[1], s_mut, ref["lp"])
    res = pr.compare(ref, dict(honest, posterior=p, doublet_posterior=d), G)
    caught = np.zeros(ref["N"], bool)
    caught[res["posterior"][1]] = True
    caught[res["doublet_posterior"][1]] = True
    assert res["ll_minority"][1].size == 0 and res["ll_majority"][1].size == 0
    assert np.array_equal(caught, cells), (mname, sname, int(cells.sum()), int(caught.sum()))
    print(f"  {mname}/{sname}: {int(hidden.sum())} hidden cells, a shift by the smallest term moves an output by at least "
          f"{moved[cells].min():.2e} bounds, honest doubles worst / bound {honest_worst:.3g}")


def test_compare_rejects_what_the_rule_names():
    """a negative or a large value where the reference is not observable; NaN; a sum off by two bounds"""
    ref = pr.case("row-lengths", "all-but-one")
    G = _g("row-lengths")
    ch = ref["chain"]
    i = int(np.argmin(ch["doublet_posterior"]))
    assert ch["doublet_posterior"][i] < pr.OBSERVABLE
    s = [r["ll"] for r in ref["sums"]]
    p, d = pr.chain_double(*s, ref["lp"])
    good = dict(ll_minority=s[0], ll_majority=s[1], posterior=p, doublet_posterior=d)
    assert all(bad.size == 0 for _, bad in pr.compare(ref, good, G).values())
    for v in (-1e-300, 1e-279, np.nan, np.inf):
        dd = d.copy()
        dd[i] = v
        assert pr.compare(ref, dict(good, doublet_posterior=dd), G)["doublet_posterior"][1].tolist() == [i], v
    for v in (0.0, 1e-281, float(d[i])):
        dd = d.copy()
        dd[i] = v
        assert pr.compare(ref, dict(good, doublet_posterior=dd), G)["doublet_posterior"][1].size == 0, v
    j = int(np.argmax(ref["count"]))
    sm = s[0].copy()
    sm[j] += 2.5 * pr.bounds(ref, G)["B"][0][j]
    assert pr.compare(ref, dict(good, ll_minority=sm), G)["ll_minority"][1].tolist() == [j]
    empty = int(np.nonzero(ref["count"] == 0)[0][0])
    sm = s[0].copy()
    sm[empty] = 5e-324
    assert pr.compare(ref, dict(good, ll_minority=sm), G)["ll_minority"][1].tolist() == [empty]
