"""GPU: genotype clusters without labels (cellector_cluster / cellector_cluster_e_step / cellector_cluster_m_step;
csrc/kernels_cluster.hip) on both engines, against the numpy twin cellector_amd/cluster.py and tests/cluster_reference.py.

Step calls.  Where the order of the sums is fixed the claim is exact: the M step's A, T and theta and the E step's s equal the twin's
bit for bit (tobytes).  What passes through the device's log or exp is held to cluster_reference's derived bounds: tab within
C_LOG = 2 units of 2^-53 relative (one ulp of log; ROCm device-libs documents 1 ulp for the f64 log and exp), w and objective within
the bounds of their chains.  Every (cell, restart) row of w adds up to 1 within 4 ulps; a cell without entries gets 1 / K.  Each call
twice: identical bits.  A step call between two loop iterations leaves the loop's bits alone.

Whole call.  The three mixtures of class_reference, K = 3, R = 16, cluster seeds 1, 2, 3 (the nine pairs of the CPU test): every one of
the first MIX_N cells carries its genotype under the best permutation; the invariants of the summary; min_loci; determinism; another
seed gives another objective vector; the labels fed to refine_classes converge within three steps.  Trajectories are not compared
with the twin's: the device's log / exp may end a stage an iteration apart.
"""
import os

import numpy as np
import pytest

import class_reference as cr
import cluster_reference as kr
import test_gpu_tile_sweep as S

pytestmark = pytest.mark.gpu

ENGINES = pytest.mark.parametrize("engine", [2, 1], ids=["tiled", "csr"])
MATRICES = pytest.mark.parametrize("name", ["row-lengths", "tier2", "hand"])
MASKED = pytest.mark.parametrize("masked", [False, True], ids=["all-loci", "masked"])
COLS = pytest.mark.parametrize("KR", kr.COLUMNS, ids=[f"J{K * R}" for K, R in kr.COLUMNS])
_mat, _ref = {}, {}


@pytest.fixture(scope="module")
def mods(oracle_lib, hip_lib_path):
    from cellector_amd import Cellector, cluster, ffi
    return dict(Cellector=Cellector, ffi=ffi, cl=cluster)


def _make(mods, engine, L, N, coo):
    g = mods["Cellector"](0)
    g.set_option("engine", engine)
    g.load_coo(L, N, *S._u32(coo), 0, 0)
    assert g.dims().loci_used == L and g.dims().nnz_used == len(coo[0])  # (min_alt = min_ref = 0: every locus is used)
    return g


def _matrix(mods, name, masked):
    if (name, masked) not in _mat:
        L, N, coo = kr.matrices()[name]
        mask = kr.case_mask(L) if masked else None
        _mat[(name, masked)] = (L, N, coo, mask, mods["cl"].Matrix(L, N, coo, mask))
    return _mat[(name, masked)]


def _once(key, fn):
    if key not in _ref:
        _ref[key] = fn()
    return _ref[key]


# ---- the M step: exact ---------------------------------------------------------------------------------------------------------------
@ENGINES
@COLS
@MASKED
@MATRICES
def test_m_step_is_the_twins(mods, name, masked, KR, engine):
    K, R = KR
    L, N, coo, mask, mat = _matrix(mods, name, masked)
    w = kr.case_w(N, K, R)
    want = _once(("m", name, masked, KR), lambda: mods["cl"].m_step(mat, w))
    g = _make(mods, engine, L, N, coo)
    got, again = g.cluster_m_step(w, mask), g.cluster_m_step(w, mask)
    for k in ("A", "T", "theta"):
        assert got[k].tobytes() == want[k].tobytes(), (k, np.abs(got[k] - want[k]).max())
    ratio = kr.compare_tab(got["theta"], mask, got["tab"])
    print(f"tab: worst / bound {ratio:.3f}")
    assert ratio <= 1.0
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k
    if mask is not None:
        assert (got["tab"][mask == 0] == 0).all() and (got["theta"][:, mask == 0] == 0.5).all()
    g.close()


# ---- the E step: s exact, w and objective inside their bounds --------------------------------------------------------------------------
@ENGINES
@COLS
@MASKED
@MATRICES
def test_e_step_sums_are_the_twins(mods, name, masked, KR, engine):
    K, R = KR
    L, N, coo, mask, mat = _matrix(mods, name, masked)
    tab = _once(("m", name, masked, KR), lambda: mods["cl"].m_step(mat, kr.case_w(N, K, R)))["tab"]
    g = _make(mods, engine, L, N, coo)
    for tname, temp in (("T=1", None), ("temps", kr.case_temp(N))):
        s_want = _once(("s", name, masked, KR), lambda: mods["cl"].e_sums(mat, tab))
        ref = _once(("e", name, masked, KR, tname), lambda: kr.e_reference(L, N, coo, tab, K, R, temp, mask))
        got, again = g.cluster_e_step(tab, K, R, temp, mask), g.cluster_e_step(tab, K, R, temp, mask)
        assert got["s"].tobytes() == s_want.tobytes(), (tname, np.abs(got["s"] - s_want).max())
        res = kr.compare_e(ref, got)
        print(tname, {k: round(v, 3) for k, v in res.items()})
        assert max(res.values()) <= 1.0, (tname, res)
        sums = got["w"].reshape(N, R, K).sum(axis=2)
        assert (np.abs(sums - 1.0) <= 4 * np.spacing(1.0)).all(), tname
        empty = ref["entries"] == 0
        assert (got["w"][empty] == 1.0 / K).all() and (got["s"][empty] == 0.0).all()
        for k in got:
            assert got[k].tobytes() == again[k].tobytes(), (tname, k)
    g.close()


# ---- the EM state stays ----------------------------------------------------------------------------------------------------------------
@ENGINES
@pytest.mark.parametrize("name", ["tier2", "row-lengths"])
def test_cluster_calls_leave_the_loop_alone(mods, name, engine):
    L, N, coo, mask, mat = _matrix(mods, name, True)
    x, y = _make(mods, engine, L, N, coo), _make(mods, engine, L, N, coo)
    want = [x.em_iteration(5.0) for _ in range(4)]
    got = []
    for it in range(4):
        got.append(y.em_iteration(5.0))
        if it == 1:
            state = (y.excluded(), y.loci_mask())
            m = y.cluster_m_step(kr.case_w(N, 3, 1), mask)
            y.cluster_e_step(m["tab"], 3, 1, None, mask)
            y.cluster(2, 2, seed=1, anneal_steps=2, max_iter=2)
            assert np.array_equal(y.excluded(), state[0]) and np.array_equal(y.loci_mask(), state[1])
    assert [bytes(s) for s in got] == [bytes(s) for s in want], (name, engine)
    assert np.array_equal(x.excluded(), y.excluded()) and np.array_equal(x.loci_mask(), y.loci_mask())
    for k, v in x.cell_outputs().items():
        assert v.tobytes() == y.cell_outputs()[k].tobytes(), k
    x.close(); y.close()


# ---- the whole call ----------------------------------------------------------------------------------------------------------------------
@ENGINES
@pytest.mark.parametrize("ms", [5, 6, 7])
def test_recovers_the_planted_genotypes(mods, ms, engine):
    cl = mods["cl"]
    L, N, coo, truth = cr.mixture(ms)
    g = _make(mods, engine, L, N, coo)
    runs = {}
    for seed in (1, 2, 3):
        r = runs[seed] = g.cluster(3, 16, seed=seed)
        perm, agree = cl.best_permutation(r["labels"][:cr.MIX_N], truth[:cr.MIX_N], 3)
        s = r["summary"]
        print(f"mixture {ms} seed {seed}: {agree} of {cr.MIX_N}, best restart {s.best_restart}, iterations {list(s.iterations_per_stage)[:s.stages]}")
        assert agree == cr.MIX_N, (ms, seed, agree)
        assert r["objective"][s.best_restart] == r["objective"].max() and s.best_restart == int(np.argmax(r["objective"]))
        assert sum(s.cluster_cells) + s.n_unlabelled == N and s.n_unlabelled == 0
        assert list(s.cluster_cells)[:3] == np.bincount(r["labels"], minlength=3).tolist() and sum(list(s.cluster_cells)[3:]) == 0
        assert s.stages == 9 and s.iterations == sum(s.iterations_per_stage) and max(s.iterations_per_stage) <= 50
        assert np.array_equal(r["labels"], np.argmax(r["ll"], axis=0))
        assert (np.abs(r["posterior"].sum(axis=0) - 1.0) <= 4 * np.spacing(1.0)).all()
        assert (r["theta"] >= 0.01).all() and (r["theta"] <= 0.99).all()
    again = g.cluster(3, 16, seed=1)
    for k in ("labels", "ll", "posterior", "theta", "objective"):
        assert again[k].tobytes() == runs[1][k].tobytes(), k
    assert bytes(again["summary"]) == bytes(runs[1]["summary"])
    assert not np.array_equal(runs[1]["objective"], runs[2]["objective"])
    two = g.cluster(3, 16, seed=1, min_loci=2)
    assert (two["labels"][cr.MIX_N:] == 255).all() and two["summary"].n_unlabelled == 6
    assert np.array_equal(two["labels"][:cr.MIX_N], runs[1]["labels"][:cr.MIX_N])
    assert sum(two["summary"].cluster_cells) + 6 == N
    # the clusters are a fixed point of the hard EM, or next to one
    ref = g.refine_classes(runs[1]["labels"], 3, max_iter=3)
    assert ref["summary"].converged == 1 and ref["summary"].iterations <= 3
    assert cl.best_permutation(ref["labels"][:cr.MIX_N], truth[:cr.MIX_N], 3)[1] == cr.MIX_N
    g.close()


def test_masked_cluster_and_default_restarts(mods):
    """a mask takes loci out of the fit (theta 0.5 there); n_restarts None = min(16, 64 // K)"""
    L, N, coo, truth = cr.mixture(5)
    mask = kr.case_mask(L)
    g = _make(mods, 2, L, N, coo)
    r = g.cluster(3, seed=2, mask=mask)
    assert len(r["objective"]) == 16 and (r["theta"][:, mask == 0] == 0.5).all()
    assert mods["cl"].best_permutation(r["labels"][:cr.MIX_N], truth[:cr.MIX_N], 3)[1] == cr.MIX_N
    assert len(g.cluster(5, seed=2, anneal_steps=2, max_iter=2)["objective"]) == 12
    g.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(mods):
    ffi = mods["ffi"]
    L, N, coo = kr.hand_matrix()
    w3, tab3 = kr.case_w(N, 3, 1), kr.case_tab(L, 3)

    def refused(fn, match):
        with pytest.raises(ffi.CellectorError, match=match) as e:
            fn()
        assert e.value.status == 1

    def every_call(g, match, n=N):
        refused(lambda: g.cluster(3, 2), match)
        refused(lambda: g.cluster_m_step(w3[:n]), match)
        refused(lambda: g.cluster_e_step(tab3, 3, 1), match)

    g = _make(mods, 2, L, N, coo)
    state = (g.em_iteration(5.0), g.excluded(), g.loci_mask())
    for K in (0, 1, 17):
        refused(lambda: g.cluster(K, 1), "2..16 are supported")
        refused(lambda: g.cluster_e_step(np.zeros((L, max(K, 1), 2)), K, 1), "2..16 are supported")
    refused(lambda: g.cluster(3, 0), "at least one restart")
    refused(lambda: g.cluster(3, 22), "at most 64")
    refused(lambda: g.cluster_e_step(np.zeros((L, 64, 2)), 16, 5), "at most 64")
    refused(lambda: g.cluster_m_step(np.zeros((N, 65))), "1..64 are supported")
    refused(lambda: g.cluster_m_step(np.zeros((N, 0))), "1..64 are supported")
    for floor in (0.0, 0.5, -0.1, np.nan):
        refused(lambda: g.cluster(3, 2, theta_floor=floor), "theta_floor")
        refused(lambda: g.cluster_m_step(w3, theta_floor=floor), "theta_floor")
    for steps in (0, 17):
        refused(lambda: g.cluster(3, 2, anneal_steps=steps), "anneal_steps")
    for v in (0.0, -1.0, np.inf, np.nan):
        refused(lambda: g.cluster(3, 2, anneal_base=v), "anneal_base")
        refused(lambda: g.cluster(3, 2, tol=v), "tol")
    refused(lambda: g.cluster(3, 2, min_loci=0), "min_loci")
    for bad in (np.nan, -1e-300):
        w = w3.copy()
        w[7, 2] = bad
        refused(lambda: g.cluster_m_step(w), "cell 7, column 2")
    for bad in (np.nan, -1.0, 0.999):
        t = np.ones(N)
        t[9] = bad
        refused(lambda: g.cluster_e_step(tab3, 3, 1, t), "temp of cell 9")
    lib = ffi.load_library()
    assert lib.cellector_cluster_m_step(g.h, None, 3, None, 0.01, None, None, None, None) == 1 and b"null w" in lib.cellector_last_error(g.h)
    assert lib.cellector_cluster_e_step(g.h, None, 3, 1, None, None, None, None, None) == 1 and b"null tab" in lib.cellector_last_error(g.h)
    g.em_begin()
    every_call(g, "in flight")
    g.em_threshold(5.0)
    every_call(g, "in flight")
    g.em_finish()
    # the ctx is as it was: the loop goes on with the bits of an undisturbed one, and the calls work
    h = _make(mods, 2, L, N, coo)
    assert bytes(h.em_iteration(5.0)) == bytes(state[0])
    h.em_iteration(5.0)
    assert bytes(g.em_iteration(5.0)) == bytes(h.em_iteration(5.0))
    assert np.array_equal(g.excluded(), h.excluded()) and np.array_equal(g.loci_mask(), h.loci_mask())
    h.close()
    assert g.cluster(2, 2, anneal_steps=2, max_iter=2)["summary"].iterations == 4
    assert g.cluster(2, 1, max_iter=0)["summary"].iterations == 0  # (no iteration: the start's own E step)
    g.close()
    g = mods["Cellector"](0)
    refused(lambda: g.cluster(3, 2), "no matrix loaded")
    lib = ffi.load_library()
    assert lib.cellector_cluster_m_step(g.h, w3.ctypes.data, 3, None, 0.01, None, None, None, None) == 1
    assert lib.cellector_cluster_e_step(g.h, tab3.ctypes.data, 3, 1, None, None, None, None, None) == 1
    assert b"no matrix loaded" in lib.cellector_last_error(g.h)
    g.close()
    m = mods["Cellector"](devices=[0, 0])
    m.load_coo(L, N, *S._u32(coo), 0, 0)
    every_call(m, "single-device")
    assert m.em_iteration(5.0) is not None
    m.close()
    g = mods["Cellector"](0)
    g.set_shard(10, 40)
    g.load_coo(L, N, *S._u32(coo), 0, 0)
    every_call(g, "set_shard", n=30)
    g.close()
    os.environ["CELLECTOR_COMM_SELFTEST"] = "1"
    try:
        g = mods["Cellector"](0)
        g.comm_init_rank(ffi.comm_unique_id(), 1, 0)
    finally:
        os.environ.pop("CELLECTOR_COMM_SELFTEST", None)
    g.load_coo(L, N, *S._u32(coo), 0, 0)
    every_call(g, "without a communicator")
    g.close()
