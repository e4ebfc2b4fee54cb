"""CPU: the reference of the K-genotype class scoring (tests/class_reference.py) held to mpmath, to the two-class reference of the
posterior phase, to its conservation law, and shown to see what the GPU tests rely on it to see.

(a) step 6 in longdouble and in double against mpmath on a handful of cells; cellector_amd.classes' twin chain likewise.
(b) K = 2 with reference_scales: alpha / beta are the bits of posterior_reference's minority / majority sets and the two per-cell
    sums are its ll_minority / ll_majority (the same evaluation: equal, which is inside any bound).
(c) over the classes and the unlabelled cells the tallies add up to the locus totals, in the reference and in the twin.
(d) on every case of tests/test_gpu_classes.py — a matrix with its K = 2 labellings (every matrix, the second-trip one included,
    takes the exclusion sets "three", "planted" and "every-second"), its K = 3 draw or its K = 16 draw, over all loci or under
    the mask — an entry left out of one class' tally, or a denominator formed without its smallest live term, moves some output
    by more than 100 bounds.  The entry is asserted on every single labelling.  The lost term is asserted on every case, i.e.
    over its labellings, and printed per labelling: one labelling cannot show it on its own — second-trip, K = 2, the planted
    set, where every cell has at least 86 entries and the two populations are far apart, so that the smaller posterior is at
    most 1.6e-31 (all loci) / 5.1e-19 (masked) in ANY cell and the loss moves every output by at most 2.9e-20 / 1.6e-07 bounds;
    the other two sets of the same case move one by more than 1e11 bounds.
(e) on every refine case and step the cells inside the margin band (labels not compared on the GPU) are at most 1 % of the cells.
    Measured here: no cell of any step is inside the band; the twin's final labels equal the planted truth in every labelled cell
    of the 900 (share 1.0) from both starts, and the "empties" start loses its fourth class on the first step.
"""
import numpy as np
import pytest

import class_reference as cr
import posterior_reference as pr
import tile_reference as tr
from cellector_amd import classes as cl



def test_chain_against_mpmath():
    ref = cr.case("tier2", 3, "draw", False)
    ch, lp, live = ref["chain"], ref["lp"], ref["live"]
    b = cr.bounds(ref, cr.g_any(ref["L"]))
    ll = np.stack([s["ll"] for s in ref["sums"]])
    pd, bd, qd = cr.chain_double(ll, lp, live)
    tw = cl.posterior_chain(ll, lp, live)
    cells = np.concatenate([np.arange(6), np.nonzero(ref["count"] == 0)[0][:2], [ref["N"] - 1]])
    for i in cells:
        post, rest = cr.chain_mp([s["ll_ld"][i] for s in ref["sums"]], lp, live)
        for k in range(3):
            want = float(post[k])
            if want < pr.OBSERVABLE:
                continue
            assert abs(float(ch["posterior"][k][i]) - want) <= 2.0 ** -58 * want
            # the double chain starts from the ROUNDED sums: half an ulp of each more than the device's bound
            slack = sum(0.5 * np.spacing(abs(s["ll"][i])) for s in ref["sums"])
            for got in (pd[k, i], tw["posterior"][k, i]):
                assert abs(got - want) <= (b["rel"][k, i] + 2 * slack) * want, (i, k)
        assert int(ch["best"][i]) == bd[i] == tw["best"][i]
    assert np.array_equal(qd, tw["qual"]) and np.array_equal(bd, tw["best"])


@pytest.mark.parametrize("mname", [m for m in pr.MATRICES])
def test_k2_is_the_two_class_reference(mname):
    for K, which in cr.case_names(mname):
        if K != 2:
            continue
        ref, two = cr.case(mname, 2, which, False), pr.case(mname, which)
        for k in (0, 1):
            assert np.array_equal(ref["ab"][k][0], two["ab"][k][0]) and np.array_equal(ref["ab"][k][1], two["ab"][k][1]), (which, k)
            assert np.array_equal(ref["sums"][k]["ll"], two["sums"][k]["ll"])
        assert ref["lp"][0] == two["lp"][0] and ref["lp"][1] == two["lp"][1]
        sc, lp = cl.reference_scales(int(two["excluded"].sum()), two["N"])
        assert list(sc) == ref["scale"] and list(lp) == ref["log_prior"]


@pytest.mark.parametrize("masked", [False, True])
def test_shared_sums_are_cell_reference(masked):
    """class_reference.CellSums against tile_reference.cell_reference: the same values to the bit"""
    L, N, coo, _ = pr.matrix("tier2")
    ref = cr.case("tier2", 3, "draw", masked)
    for k in range(3):
        want = tr.cell_reference(N, *coo, ref["ab"][k][0], ref["ab"][k][1], ref["mask"])
        for key in ("ll", "ll_ld", "count", "abs_ll", "b_ll", "loci_used"):
            assert np.array_equal(ref["sums"][k][key] if key != "loci_used" else cr.CellSums(N, coo, ref["mask"]).cnt, want[key]), key


@pytest.mark.parametrize("mname", ["tier2", "row-lengths"])
def test_conservation(mname):
    L, N, coo, _ = pr.matrix(mname)
    lo, ce, al, re = coo
    tot_a = np.bincount(lo, weights=al.astype(np.float64), minlength=L).astype(np.uint64)
    tot_r = np.bincount(lo, weights=re.astype(np.float64), minlength=L).astype(np.uint64)
    for K in (1, 3, 16):
        lab = cr.case_labels(mname, K, "draw")[0]
        cells, alt, ref = cr.tallies(L, coo, lab, K)
        assert np.array_equal(alt.sum(axis=0), tot_a) and np.array_equal(ref.sum(axis=0), tot_r) and cells.sum() == N
        tc, ta, tref = cl.class_tallies(L, coo, lab, K)
        assert np.array_equal(ta, alt[:K]) and np.array_equal(tref, ref[:K]) and np.array_equal(tc, cells[:K].astype(np.uint64))


GROUPS = [(m, K, masked) for m in pr.MATRICES for K in (2, 3, 16) for masked in (False, True)]


@pytest.mark.parametrize("mname,K,masked", GROUPS, ids=[f"{m}-K{K}-{'mask' if x else 'all'}" for m, K, x in GROUPS])
def test_sensitivity(mname, K, masked):
    L, N, coo, _ = pr.matrix(mname)
    G = cr.g_any(L)
    lo, ce, al, re = coo
    rng = np.random.default_rng(K + N)
    lost = {}
    for which in [w for k, w in cr.case_names(mname) if k == K]:
        ref = cr.case(mname, K, which, masked)
        used = np.ones(len(lo), bool) if ref["mask"] is None else ref["mask"][lo] != 0
        lab = ref["labels"][ce]
        for k in [k for k in range(K) if ref["live"][k]][:3]:
            cand = np.nonzero(used & (lab == k) & (al + re > 0))[0]
            j = int(cand[rng.integers(len(cand))])
            moved = cr.drop_one_entry(ref, coo, G, k, j)
            assert moved > cr.SENSITIVE, (which, k, j, moved)
        lost[which] = cr.drop_smallest_term(ref, G)
    print(f"  {mname} K {K} {'masked' if masked else 'all loci'}: a lost smallest term moves an output by (bounds) {lost}")
    assert max(lost.values()) > cr.SENSITIVE, lost


@pytest.mark.parametrize("which", cr.REFINE_STARTS)
def test_refine_cases_stay_clear_of_the_band(which):
    L, N, coo, truth = cr.mixture()
    start, K = cr.refine_start(which)
    tw = cl.refine(L, coo, start, K, cr.ll_fn_80bit(N, coo), max_iter=20)
    assert tw["summary"]["converged"] == 1 and 2 <= tw["summary"]["iterations"] <= 10
    G = cr.g_any(L)
    for t, st in enumerate(tw["steps"]):
        ref = cr.reference(L, N, coo, st["labels_in"], K)
        share = cr.bounds(ref, G)["in_band"].mean()
        print(f"  {which} step {t}: moved {st['n_moved']}, cells inside the band {share:.4f}, sizes {ref['cells']}")
        assert share <= 0.01
        assert np.array_equal(ref["chain"]["best"], st["best"])
    lab = tw["labels"]
    sel = (start != cr.UNLABELLED) & (np.arange(N) < cr.MIX_N)
    print(f"  {which}: final labels equal to the planted truth: {(lab[sel] == truth[sel]).mean():.4f}")
    assert (lab[start == cr.UNLABELLED] == cr.UNLABELLED).all()
    if which == "empties":
        assert tw["summary"]["class_cells"][3] == 0 and (start == 3).sum() == 3
    # min_loci: with 2 the one-entry cells keep their labels whatever their best class is
    tw2 = cl.refine(L, coo, start, K, cr.ll_fn_80bit(N, coo), max_iter=20, min_loci=2)
    assert np.array_equal(tw2["labels"][cr.MIX_N:], start[cr.MIX_N:])
