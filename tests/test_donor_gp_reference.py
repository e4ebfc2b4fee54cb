"""CPU: tests/donor_gp_reference.py against mpmath; the numpy twin of the soft donor calls (cellector_amd/donors.py, soft_*) within the
derived bounds of that reference; its bytes under one-hot and no-call rows; the sensitivity of the sums to one row; the planted pool
with degraded calls."""
import numpy as np
import pytest

import donor_gp_reference as gr
import donor_reference as dr
from cellector_amd import cluster, donors as dn

L, N, COO = dr.case_matrix()
A, R = dr.totals(L, COO)
IDS = np.arange(L)
_mat = {}


def _matrix(masked):
    if masked not in _mat:
        mask = dr.case_mask() if masked else None
        _mat[masked] = (mask, cluster.Matrix(L, N, COO, mask), dn.tables(A, R, mask=mask))
    return _mat[masked]


def test_the_cases_cover_what_they_claim():
    l1, c1 = gr.head_locus()
    for D in dr.DONORS:
        gp, gt = gr.case_gp(D), dr.case_gt(D)
        w, kind = dn.soft_weights(gp, IDS)
        rw, rk = gr.weights_reference(gp)
        assert w.tobytes() == rw.tobytes() and kind.tobytes() == rk.tobytes()
        called = gt.T < 3
        forced = (IDS == l1)[:, None] & (np.arange(D) == 0)[None, :]  # (donor 0 at the head locus is soft whatever case_gt says)
        assert np.array_equal((kind == 3) & ~forced, ~called & ~forced)  # the no-calls are kept
        share = (kind[called] < 3).mean()
        assert 0.4 < share < 0.75, share  # about half of the called rows are one-hot (the hard donors: all of theirs)
        x = gp.transpose(1, 0, 2)[kind == 4].astype(np.float64)
        tot = x.sum(axis=1)
        assert ((x > 0).sum(axis=1) == 3).any()
        for z in range(3):
            assert ((x[:, z] == 0) & ((x > 0).sum(axis=1) == 2)).any(), z
        assert (np.abs(tot - 2.5) < 1e-6).any() and (x == np.float32(1e-30)).any() and (x == 2.0 ** -149).any()
        assert kind[l1, 0] == 4 and gp[0, l1, 0] == 0  # the head entries fall on a soft row that rules 0/0 out
        assert np.array_equal(dn.hard_codes(gp), gr.hard_reference(gp))
    # ... and at (alt 0, ref 40) the largest t_g IS that of 0/0
    tab1 = dn.tables(A, R)[0]
    t = 0.0 * tab1[l1, :3, 0] + 40.0 * tab1[l1, :3, 1]
    assert np.argmax(t) == 0
    # the deep matrix: t_g - m below -745 under some soft row
    Ld, Nd, (lo, ce, al, re) = gr.deep_matrix()
    assert max(al.max(), re.max()) == 2000 and Nd < 100
    td = dn.tables(*dr.totals(Ld, (lo, ce, al, re)))[0]
    t = al[:, None] * td[lo, :3, 0] + re[:, None] * td[lo, :3, 1]
    assert (t.min(axis=1) - t.max(axis=1)).min() < -745


def test_reference_agrees_with_mpmath():
    import mpmath
    mpmath.mp.prec = 200
    D = 5
    gp = gr.case_gp(D)
    w, kind = dn.soft_weights(gp, IDS)
    tab1, tab2 = dn.tables(A, R)
    lo, ce, al, re = dr._rows(COO, None)
    w4 = gr._four(w, kind)
    term, B = gr._terms(al, re, tab1[lo], w4[lo], kind[lo] == 4, 0)
    a = np.zeros(N, np.int64)
    ww = (w4[lo, a[ce]][:, None, :, None] * w4[lo][:, :, None, :]).reshape(len(lo), D, 16)
    term2, B2 = gr._terms(al, re, tab2[lo], ww, (kind[lo, 0] == 4)[:, None] | (kind[lo] == 4), 1)
    rng = np.random.default_rng(5)
    soft = np.argwhere(kind[lo] == 4)
    picks = soft[rng.choice(len(soft), 60, replace=False)]
    heads = np.flatnonzero((al + re == 40) & ((al == 0) | (re == 0)))
    picks = np.concatenate([picks, [(e, 0) for e in heads]])
    mp = mpmath.mpf

    def mix(ts, ws):
        P = [i for i, x in enumerate(ws) if x > 0]
        m = max(ts[i] for i in P)
        return m + mpmath.log(sum(mp(float(ws[i])) * mpmath.exp(ts[i] - m) for i in P))

    for e, d in picks:
        ts = [mp(int(al[e])) * mp(float(tab1[lo[e], g, 0])) + mp(int(re[e])) * mp(float(tab1[lo[e], g, 1])) for g in range(3)]
        want = mix(ts, w[lo[e], d])
        assert abs(mp(float(term[e, d])) - want) <= mp(2.0 ** -52) * abs(want) + mp(1e-300), (e, d)
        ts = [mp(int(al[e])) * mp(float(tab2[lo[e], j, 0])) + mp(int(re[e])) * mp(float(tab2[lo[e], j, 1])) for j in range(16)]
        want = mix(ts, ww[e, d])
        assert abs(mp(float(term2[e, d])) - want) <= mp(2.0 ** -52) * abs(want) + mp(1e-300), (e, d)
    assert (B[kind[lo] == 4] > 0).all() and (B2 > 0).all()


@pytest.mark.parametrize("masked", [False, True], ids=["all-loci", "masked"])
@pytest.mark.parametrize("D", dr.DONORS)
def test_twin_stays_within_the_bound(D, masked):
    """numpy's exp and log are good to an ulp, as the device's: the twin is held to the device's bound"""
    mask, mat, (tab1, tab2) = _matrix(masked)
    w, kind = dn.soft_weights(gr.case_gp(D), IDS)
    for lp, anchor, prm in ((None, None, {}), (dr.case_prior(D), (np.arange(N) % D).astype(np.uint8),
                                               dict(doublet_rate=0.3, posterior_threshold=0.9, min_loci=3))):
        got = dn.posteriors_gp(mat, w, kind, A, R, lp, anchor, tab1, tab2, **prm)
        ref = gr.reference(L, N, COO, w, kind, tab1, tab2, lp, got["anchor"], mask, **prm)
        res, undecided = gr.compare(ref, got)
        print(D, masked, {k: round(v, 3) for k, v in res.items()}, int(undecided.sum()))
        assert max(res.values()) <= 1.0, res
        assert undecided.sum() < 0.01 * N
        r = np.arange(N)
        assert got["pair_ll"][r, got["anchor"]].tobytes() == got["ll"][r, got["anchor"]].tobytes()
    labels = (np.arange(N) % 5).astype(np.int64)
    alt, rf = np.zeros((5, L), np.int64), np.zeros((5, L), np.int64)
    lo, ce, al, re = COO
    np.add.at(alt, (labels[ce], lo), al)
    np.add.at(rf, (labels[ce], lo), re)
    got = dn.soft_match_sums(alt, rf, tab1, w, kind, mask)
    ll, B = gr.match_reference(alt, rf, tab1, w, kind, mask)
    assert gr.ratio(got, ll, B) <= 1.0


def test_twin_on_the_deep_matrix():
    Ld, Nd, coo = gr.deep_matrix()
    tab1, tab2 = dn.tables(*dr.totals(Ld, coo))
    mat = cluster.Matrix(Ld, Nd, coo, None)
    for D in (2, 5, 33):
        w, kind = dn.soft_weights(gr.deep_gp(D), np.arange(Ld))
        got = dn.posteriors_gp(mat, w, kind, None, None, tab1=tab1, tab2=tab2)
        assert np.isfinite(got["ll"]).all() and np.isfinite(got["pair_ll"]).all() and np.isfinite(got["posterior"]).all()
        ref = gr.reference(Ld, Nd, coo, w, kind, tab1, tab2, None, got["anchor"], None)
        res, _ = gr.compare(ref, got)
        assert max(res.values()) <= 1.0, res


@pytest.mark.parametrize("masked", [False, True], ids=["all-loci", "masked"])
@pytest.mark.parametrize("D", dr.DONORS)
def test_one_hot_and_no_call_rows_are_the_hard_bytes(D, masked):
    mask, mat, (tab1, tab2) = _matrix(masked)
    gt = dr.case_gt(D)
    gp = dn.one_hot(gt)
    assert np.array_equal(dn.hard_codes(gp), gt)
    w, kind = dn.soft_weights(gp, IDS)
    assert np.array_equal(kind, gt.T)
    s = dn.soft_singlet_sums(mat, tab1, w, kind)
    assert s.tobytes() == dn.singlet_sums(mat, tab1, gt.T).tobytes()
    anchor = (np.arange(N) % D).astype(np.uint8)
    assert dn.soft_pair_sums(mat, tab2, w, kind, anchor, s).tobytes() == dn.pair_sums(mat, tab2, gt.T, anchor).tobytes()
    alt = np.random.default_rng(1).integers(0, 50, (3, L))
    rf = np.random.default_rng(2).integers(0, 50, (3, L))
    assert dn.soft_match_sums(alt, rf, tab1, w, kind, mask).tobytes() == dn.match_sums(alt, rf, tab1, gt.T, mask).tobytes()
    # under soft rows the donors that are hard throughout keep those bytes
    gps = gr.case_gp(D)
    ws, ks = dn.soft_weights(gps, IDS)
    hard = np.array([gr.hard_donor(d) for d in range(D)])
    assert (ks[:, hard] < 4).all()
    assert dn.soft_singlet_sums(mat, tab1, ws, ks)[:, hard].tobytes() == dn.singlet_sums(mat, tab1, dn.hard_codes(gps).T)[:, hard].tobytes()


@pytest.mark.parametrize("D", dr.DONORS)
def test_one_row_moves_a_sum_by_more_than_100_bounds(D):
    """the bound is a statement about rounding, not about the model: one weight row replaced by its argmax is far outside it"""
    mask, mat, (tab1, tab2) = _matrix(False)
    gp = gr.case_gp(D)
    w, kind = dn.soft_weights(gp, IDS)
    ref = gr.reference(L, N, COO, w, kind, tab1, tab2)
    l1, c1 = gr.head_locus()
    gp2 = gp.copy()
    gp2[0, l1] = dn.one_hot(dn.hard_codes(gp[:1, l1:l1 + 1]))[0, 0]
    w2, k2 = dn.soft_weights(gp2, IDS)
    assert k2[l1, 0] < 4 and kind[l1, 0] == 4
    s = dn.soft_singlet_sums(mat, tab1, w2, k2)
    moved = np.abs(s[:, 0] - ref["s"][:, 0].astype(np.float64)) / np.where(ref["B_s"][:, 0] > 0, ref["B_s"][:, 0], np.inf)
    assert moved[c1] > 100 and moved.max() > 100, moved.max()


@pytest.mark.parametrize("seed", [5, 6, 7])
def test_planted_pool_with_degraded_calls(seed):
    """half of the called rows carry a GP whose argmax is a wrong genotype (truth 0.35, a wrong one 0.60, the third 0.05): the
    mixture over GP gives at least 99 % of the singlets their planted donor, and at least 30 more than the argmax calls do"""
    Lp, Np, coo, gp, truth = gr.degraded_pool(seed)
    mat = cluster.Matrix(Lp, Np, coo, None)
    tab1 = dn.tables(*dr.totals(Lp, coo))[0]
    ids = np.arange(Lp)
    w, kind = dn.soft_weights(gp, ids)
    soft = dn.soft_singlet_sums(mat, tab1, w, kind)
    hard = dn.singlet_sums(mat, tab1, dn.hard_codes(gp).T)
    single = truth != 255
    n_soft = int((np.argmax(soft, axis=1)[single] == truth[single]).sum())
    n_hard = int((np.argmax(hard, axis=1)[single] == truth[single]).sum())
    print("seed", seed, "singlets", int(single.sum()), "hard calls", n_hard, "mixture over GP", n_soft)
    assert n_soft >= 0.99 * single.sum() and n_soft >= n_hard + 30, (n_soft, n_hard, int(single.sum()))
