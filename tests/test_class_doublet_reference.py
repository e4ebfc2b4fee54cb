"""CPU: the reference of the K-class doublet scoring (tests/class_doublet_reference.py) held to mpmath and to the reference of the
posterior phase, shown to see what the GPU tests rely on it to see, and the conditions those tests need of their inputs.

(a) step 6 in longdouble against mpmath on a handful of cells, and the twin's double chain (cellector_amd.classes.doublet_chain)
    within the device's bound of it.
(b) K = 2 with reference_scales / reference_doublet_scales is calculate_posteriors: the pair alpha / beta are posterior_reference's
    doublet set bit for bit, the pair sum is its third sum, and posterior / doublet_posterior agree with its chain within the two
    references' bounds added (its nested logsumexp and this chain differ only by rounding).
(c) sensitivity: an entry left out of one pair's distribution moves that pair's sum, and a denominator formed without each cell's
    smallest live pair term moves a posterior, by more than 100 bounds on every group of cases; the factors are printed.
(d) the held-out refine on class_reference.mixture() plus 60 synthetic cross-genotype doublets (cellector_amd.doublets), parents
    thinned at 0 and at 0.5, from the truth and from a noisy labelling, driven by the 80-bit sums: no cell of any step is inside a
    band, and the reference's best, best_pair and call equal the twin's in every cell of every step.  Measured at the fixed point
    (3 steps from the truth, 4 from the noisy start, at both rates): of the planted doublets that carry a label 60 / 60 (truth)
    and 55 / 55 (noisy; the other 5 are unlabelled at the start and stay so) are held, every one with the right pair; 0 of the
    906 singlets are held; every labelled singlet of the 900 has its planted genotype; no cell has 0.01 < doublet posterior <
    0.99.  The GPU test compares with the twin, not with these shares.
(e) conditions: on every case of tests/test_gpu_class_doublets.py's sweep the reference leaves at most 1 cell in 1000 out of a
    comparison (inside a band, or with a doublet posterior below OBSERVABLE).  Measured: 0 cells everywhere but K = 16 on
    row-lengths (1 of 5420 with all loci, 3 under the mask: best_pair between pairs whose floored priors are equal).
"""
import numpy as np
import pytest

import class_doublet_reference as dr
import class_reference as cr
import posterior_reference as pr
from cellector_amd import classes as cl


def test_chain_against_mpmath():
    ref = dr.case("tier2", 3, "draw", False)
    ch, live = ref["chain"], ref["live"]
    b = dr.bounds(ref, cr.g_any(ref["L"]))
    ll = np.stack([s["ll"] for s in ref["sums"]])
    llp = np.stack([s["ll"] for s in ref["psums"]])
    tw = cl.doublet_chain(ll, llp, ref["lp"], ref["lpp"], live)
    cells = np.concatenate([np.arange(6), np.nonzero(ref["count"] == 0)[0][:2], [ref["N"] - 1]])
    slack_all = sum(0.5 * np.spacing(np.abs(s["ll"])) for s in ref["sums"] + ref["psums"])  # the twin starts from the ROUNDED sums
    for i in cells:
        post, q = dr.chain_mp([s["ll_ld"][i] for s in ref["sums"]], [s["ll_ld"][i] for s in ref["psums"]], ref["lp"], ref["lpp"], live)
        for k in range(3):
            want = float(post[k])
            if want >= pr.OBSERVABLE:
                assert abs(float(ch["posterior"][k][i]) - want) <= 2.0 ** -58 * want
                assert abs(tw["posterior"][k, i] - want) <= (b["rel"][k, i] + 2 * slack_all[i]) * want, (i, k)
        want = float(sum(q))
        assert abs(float(ch["doublet_posterior"][i]) - want) <= 2.0 ** -58 * want
        assert abs(tw["doublet_posterior"][i] - want) <= (b["rel_d"][i] + 2 * slack_all[i]) * want, i
    clear = ~dr.left_out(ref, cr.g_any(ref["L"]))
    for k in ("best", "call"):
        assert np.array_equal(tw[k][clear], ch[k][clear]), k
    assert np.array_equal(tw["best_pair"][clear], ch["best_pair"][clear])


@pytest.mark.parametrize("mname", list(pr.MATRICES))
def test_k2_is_calculate_posteriors(mname):
    G = cr.g_any(pr.matrix(mname)[0])
    for which in cr.K2_SETS:
        ref, two = dr.case(mname, 2, which, False), pr.case(mname, which)
        assert np.array_equal(ref["pab"][0][0], two["ab"][2][0]) and np.array_equal(ref["pab"][0][1], two["ab"][2][1]), which
        assert np.array_equal(ref["psums"][0]["ll"], two["sums"][2]["ll"])
        assert ref["lpp"][0] == two["lp"][2]
        ps, lpp = cl.reference_doublet_scales(int(two["excluded"].sum()), two["N"])
        assert list(ps) == ref["ps"] and abs(lpp[0] - ref["lpp"][0]) <= np.spacing(abs(lpp[0]))
        b, b2 = dr.bounds(ref, G), pr.bounds(two, G)
        for name, mine, rel, rel2 in (("posterior", ref["chain"]["posterior"][0], b["rel"][0], b2["rel_p"]),
                                      ("doublet_posterior", ref["chain"]["doublet_posterior"], b["rel_d"], b2["rel_d"])):
            want = two["chain"][name]
            seen = want >= pr.OBSERVABLE
            d = np.abs(mine - want)[seen].astype(np.float64) / want[seen].astype(np.float64)
            assert (d <= (rel + rel2)[seen]).all(), (which, name, float((d / (rel + rel2)[seen]).max()))
            assert (mine[~seen] < pr.UNOBSERVED_BELOW).all()


GROUPS = [(m, K, masked) for m in pr.MATRICES for K in (2, 3, 5) for masked in (False, True)] + [("row-lengths", 16, False),
                                                                                                  ("row-lengths", 16, True)]
IDS = [f"{m}-K{K}-{'mask' if x else 'all'}" for m, K, x in GROUPS]


@pytest.mark.parametrize("mname,K,masked", GROUPS, ids=IDS)
def test_sensitivity_and_conditions(mname, K, masked):
    L, N, coo, _ = pr.matrix(mname)
    G = cr.g_any(L)
    lo, ce, al, re = coo
    rng = np.random.default_rng(K + N)
    lost = {}
    for which in [w for k, w in dr.case_names(mname) if k == K]:
        ref = dr.case(mname, K, which, masked)
        # (e) the condition the GPU sweep needs of this case
        out = int(dr.left_out(ref, G).sum())
        print(f"  {mname} K {K} {which} {'masked' if masked else 'all loci'}: {out} of {N} cells left out of a comparison")
        assert 1000 * out <= N, (which, out)
        # (c) an entry of a cell of the pair left out of the pair's tallies
        used = np.ones(len(lo), bool) if ref["mask"] is None else ref["mask"][lo] != 0
        lab = dr.unheld(ref["labels"], ref["held"])[ce]
        for p in ref["chain"]["ps"][:3]:
            a, b = dr.pairs(K)[p]
            cand = np.nonzero(used & ((lab == a) | (lab == b)) & (al + re > 0))[0]
            j = int(cand[rng.integers(len(cand))])
            moved = dr.drop_one_pair_entry(ref, coo, G, p, j)
            assert moved > dr.SENSITIVE, (which, p, j, moved)
        lost[which] = dr.drop_smallest_pair_term(ref, G)
    print(f"  {mname} K {K} {'masked' if masked else 'all loci'}: a lost smallest pair term moves an output by (bounds) {lost}")
    assert max(lost.values()) > dr.SENSITIVE, lost


@pytest.mark.parametrize("rate", dr.RATES)
@pytest.mark.parametrize("which", dr.DOUBLET_STARTS)
def test_refine_cases_stay_clear_of_the_bands(which, rate):
    L, N, coo, truth, par = dr.doublet_mixture(rate)
    start, K = dr.doublet_start(which, rate)
    tw = cl.refine_doublets(L, coo, start, K, cr.ll_fn_80bit(N, coo), max_iter=20)
    assert tw["summary"]["converged"] == 1 and 2 <= tw["summary"]["iterations"] <= 10
    G = cr.g_any(L)
    for t, st in enumerate(tw["steps"]):
        ref = dr.reference(L, N, coo, st["labels_in"], K, st["held_in"])
        out = int(dr.left_out(ref, G).sum())
        print(f"  {which} rate {rate} step {t}: moved {st['n_moved']}, cells inside a band {out}, unheld sizes {ref['cells']}")
        assert out == 0
        ch = ref["chain"]
        assert np.array_equal(ch["best"], st["best"]) and np.array_equal(ch["call"], st["call"])
        assert np.array_equal(ch["best_pair"], st["best_pair"])
    held, lab = tw["held"] != 0, tw["labels"]
    d = np.arange(N) >= N - dr.N_DOUBLETS
    labelled = start != cr.UNLABELLED
    right = held[d] & (tw["best_pair"][d] == par).all(axis=1)
    mid = int(((tw["doublet_posterior"] > 0.01) & (tw["doublet_posterior"] < 0.99)).sum())
    sel = ~d & labelled & (np.arange(N) < cr.MIX_N)
    print(f"  {which} rate {rate}: steps {tw['summary']['iterations']}, planted doublets held {int(held[d].sum())} of {int((d & labelled).sum())} "
          f"labelled ({dr.N_DOUBLETS} planted), with the right pair {int(right.sum())}, singlets held {int(held[~d].sum())} of "
          f"{int((~d).sum())}, labelled singlets with the planted genotype {(lab[sel] == truth[sel]).mean():.4f}, cells with 0.01 < "
          f"doublet posterior < 0.99: {mid}")
    assert (lab[~labelled] == cr.UNLABELLED).all() and not held[~labelled].any()
    assert tw["summary"]["n_held"] == int(held.sum())
    # min_loci: with 2 the one-entry cells keep their labels and flags whatever their scores are
    tw2 = cl.refine_doublets(L, coo, start, K, cr.ll_fn_80bit(N, coo), max_iter=20, min_loci=2)
    one = slice(cr.MIX_N, cr.MIX_N + 6)
    assert np.array_equal(tw2["labels"][one], start[one]) and not tw2["held"][one].any()
