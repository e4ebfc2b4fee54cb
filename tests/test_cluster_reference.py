"""CPU: cellector_amd/cluster.py (the numpy twin of the clustering calls) against tests/cluster_reference.py (80-bit), what the bounds
let be seen, the start draw against a scalar restatement, and the recovery of a planted three-genotype mixture.

Recovery: class_reference.mixture(seed) for seeds 5, 6, 7 (900 real cells x 600 loci, genotypes at 70 / 20 / 10 %), K = 3, R = 16,
cluster seeds 1, 2, 3, default parameters: every one of the first MIX_N cells carries its genotype under the best permutation.  All
nine (mixture, seed) pairs of the first choice pass; none was replaced.  The nine fits run with sums="dense" (the ordered sums cost
0.2 s per iteration at J = 48 and a fit takes 100 to 170 iterations); one fit with the ordered sums at R = 2 shows that the two modes
end in the same partition.  With R = 1 four of the nine runs stop in a local optimum (531, 528, 551, 557 cells of 900 agree): the
restarts matter, which is asserted as "at least one".
"""
import numpy as np
import pytest

import class_reference as cr
import cluster_reference as kr
from cellector_amd import cluster as cl

MIXTURES, SEEDS = (5, 6, 7), (1, 2, 3)
_mat = {}


def _matrix(name, masked):
    key = (name, masked)
    if key not in _mat:
        L, N, coo = kr.matrices()[name]
        mask = kr.case_mask(L) if masked else None
        _mat[key] = (L, N, coo, mask, cl.Matrix(L, N, coo, mask))
    return _mat[key]


@pytest.mark.parametrize("masked", [False, True], ids=["all-loci", "masked"])
@pytest.mark.parametrize("name", ["row-lengths", "tier2", "hand"])
def test_twin_steps_within_the_reference_bounds(name, masked):
    L, N, coo, mask, mat = _matrix(name, masked)
    for K, R in kr.COLUMNS:
        J = K * R
        tab = kr.case_tab(L, J)
        for temp in (None, kr.case_temp(N)):
            got = cl.e_step(mat, tab, K, R, temp)
            ref = kr.e_reference(L, N, coo, tab, K, R, temp, mask)
            res = kr.compare_e(ref, got)
            assert max(res.values()) <= 1.0, (name, masked, K, R, temp is not None, res)
            sums = got["w"].reshape(N, R, K).sum(axis=2)
            assert (np.abs(sums - 1.0) <= 4 * np.spacing(1.0)).all()
            empty = ref["entries"] == 0
            assert (name != "hand" or empty.any()) and (got["w"][empty] == 1.0 / K).all() and (got["s"][empty] == 0.0).all()
        w = kr.case_w(N, K, R)
        got = cl.m_step(mat, w)
        ref = kr.m_reference(L, N, coo, w, 0.01, mask)
        res = kr.compare_m(ref, got)
        assert max(res.values()) <= 1.0, (name, masked, K, R, res)
        assert kr.compare_tab(got["theta"], mask, got["tab"]) <= 1.0
        if mask is not None:
            off = mask == 0
            assert (got["theta"][:, off] == 0.5).all() and (got["A"][:, off] == 0).all() and (got["tab"][off] == 0).all()
        none = ref["entries"] == 0
        assert (got["theta"][:, none] == 0.5).all()


def test_a_dropped_entry_is_seen():
    """one entry left out of a cell's sum / a locus' tally moves them by many bounds"""
    L, N, coo, _, mat = _matrix("hand", False)
    K, R = 3, 1
    tab, w = kr.case_tab(L, K * R), kr.case_w(N, K, R)
    e_ref, m_ref = kr.e_reference(L, N, coo, tab, K, R), kr.m_reference(L, N, coo, w)
    rng = np.random.default_rng(1)
    seen_e = seen_m = 0
    for j in rng.choice(len(coo[0]), 40, replace=False):
        if coo[2][j] + coo[3][j] == 0:
            continue  # (an entry without reads adds 0 to both)
        less = [np.delete(x, j) for x in coo]
        e = cl.e_step(cl.Matrix(L, N, less), tab, K, R)
        c = coo[1][j]
        moved = np.abs(e["s"][c] - e_ref["s"][c].astype(np.float64)) / e_ref["B_s"][c]
        assert moved.min() > 100.0, (j, moved)
        seen_e += 1
        m = cl.m_step(cl.Matrix(L, N, less), w)
        l = coo[0][j]
        live = w[c] * (coo[2][j] + coo[3][j]) > 1e-6 * m_ref["T"][:, l].astype(np.float64)
        moved = np.abs(m["T"][:, l] - m_ref["T"][:, l].astype(np.float64)) / m_ref["B_T"][:, l]
        assert (moved[live] > 100.0).all(), (j, moved)
        seen_m += int(live.any())
    assert seen_e >= 30 and seen_m >= 20


def _mix64(z):
    z &= (1 << 64) - 1
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & ((1 << 64) - 1)
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & ((1 << 64) - 1)
    return z ^ (z >> 31)


def test_start_draw_is_the_scalar_formula():
    G, M = 0x9E3779B97F4A7C15, (1 << 64) - 1
    for seed, L, J, floor in ((4, 7, 3, 0.01), (0, 5, 64, 0.01), (2 ** 63 + 5, 3, 48, 0.2), (123456789, 1000, 6, 0.05)):
        th = cl.start_theta(seed, L, J, floor)
        assert th.shape == (L, J) and (th >= floor).all() and (th <= 1.0 - floor).all()
        for l, j in ((0, 0), (L - 1, J - 1), (L // 2, J // 3)):
            u = (_mix64(_mix64((seed * G + G) & M) + ((l * J + j + 1) * G & M)) >> 11) * 2.0 ** -53
            assert th[l, j] == floor + (1.0 - 2.0 * floor) * u, (seed, l, j)
    assert not np.array_equal(cl.start_theta(1, 50, 6), cl.start_theta(2, 50, 6))


def test_best_permutation():
    truth = np.array([0, 0, 1, 2, 2, 255, 1], np.uint8)
    lab = np.array([2, 2, 0, 1, 1, 0, 255], np.uint8)
    perm, agree = cl.best_permutation(lab, truth, 3)
    assert perm == [1, 2, 0] and agree == 5


_recovered = {}


def _fit(ms, seed, R):
    key = (ms, seed, R)
    if key not in _recovered:
        L, N, coo, truth = cr.mixture(ms)
        if ms not in _mat:
            _mat[ms] = cl.Matrix(L, N, coo)
        f = cl.fit(L, N, _mat[ms], 3, R, seed, sums="dense")
        _recovered[key] = (f, cl.best_permutation(f["labels"][:cr.MIX_N], truth[:cr.MIX_N], 3)[1])
    return _recovered[key]


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("ms", MIXTURES)
def test_recovers_the_planted_genotypes(ms, seed):
    f, agree = _fit(ms, seed, 16)
    assert agree == cr.MIX_N, (ms, seed, agree)
    assert f["objective"][f["best_restart"]] == f["objective"].max() and f["best_restart"] == int(np.argmax(f["objective"]))
    assert f["cluster_cells"].sum() + f["n_unlabelled"] == cr.MIX_N + 6 and f["n_unlabelled"] == 0
    assert f["stages"] == 9 and len(f["iterations_per_stage"]) == 9 and max(f["iterations_per_stage"]) <= 50


def test_restarts_matter():
    agrees = [_fit(ms, seed, 1)[1] for ms in MIXTURES for seed in SEEDS]
    assert any(a < cr.MIX_N for a in agrees), agrees


def test_ordered_and_dense_fits_agree_on_the_partition():
    L, N, coo, truth = cr.mixture(5)
    mat = cl.Matrix(L, N, coo)
    a = cl.fit(L, N, mat, 3, 2, 3, anneal_steps=4, max_iter=8)
    b = cl.fit(L, N, mat, 3, 2, 3, anneal_steps=4, max_iter=8, sums="dense")
    assert np.array_equal(a["labels"], b["labels"]) and a["best_restart"] == b["best_restart"]
    assert np.allclose(a["objective"], b["objective"], rtol=1e-9)
    two = cl.fit(L, N, mat, 3, 2, 3, anneal_steps=4, max_iter=8, min_loci=2)
    assert (two["labels"][cr.MIX_N:] == cl.UNLABELLED).all() and two["n_unlabelled"] == 6
    assert np.array_equal(two["labels"][:cr.MIX_N], a["labels"][:cr.MIX_N])
