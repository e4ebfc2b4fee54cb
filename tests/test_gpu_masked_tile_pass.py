"""GPU, engine 2: cellector_cell_log_likelihoods runs the tile pass whatever the mask.

Until now a caller's mask — or ANY call on a ctx whose loop had filtered a locus, or on which cellector_set_loci_mask was used —
sent that call to the CSR kernel, because the tile pass' finalize took the used-locus counts from the ctx's own per-cell counts of
entries at masked loci.  The call now forms the counts of ITS mask in scratch and hands them to the finalize; the ctx's own counts,
mask and masked-locus count stay.

Asserted with option timing 2 (only the tile kernel is timed): kernel_time(CELLECTOR_K_TILE_LL)'s launch count grows by one per call
in every routing case; the results are within tile_reference.cell_bound of tile_reference.cell_reference under the CALL's mask and
loci_used is exact; a ctx that had such calls between its iterations produces the bits of one that had not.

Matrix: tests/test_gpu_cell_pmfs.py's 1400 loci x 1500 cells (three chunks, two cell blocks; without its total-65535 entry, whose
reference is O(n^2)), tile_sb 2 and 4.
"""
import numpy as np
import pytest

import test_gpu_cell_pmfs as P
import test_gpu_tile_sweep as S
import tile_reference as tr

pytestmark = pytest.mark.gpu

L, N = P.L1, P.N1


@pytest.fixture(scope="module")
def mods(oracle_lib, hip_lib_path):
    from cellector_amd import Cellector, ffi
    return dict(Cellector=Cellector, ffi=ffi)


@pytest.fixture(scope="module")
def case():
    coo = P._case1_coo(huge=False)
    alpha, beta = S._alpha_beta(L, 99)
    rng = np.random.default_rng(23)
    chunk = np.ones(L, np.uint8)
    chunk[639:1278] = 0
    masks = {"none": None, "random 30 %": (rng.random(L) >= 0.3).astype(np.uint8), "chunk 1": chunk,
             "other 20 %": (rng.random(L) >= 0.2).astype(np.uint8)}
    refs = {k: tr.cell_reference(N, *coo, alpha, beta, mask=m) for k, m in masks.items()}
    return dict(coo=coo, alpha=alpha, beta=beta, masks=masks, refs=refs)


def _load(mods, coo, sb):
    g = mods["Cellector"](0)
    g.set_option("engine", 2)
    g.set_option("timing", 2)
    g.load_coo(L, N, *S._u32(coo), 0, 0)
    g.set_option("tile_sb", sb)
    assert g.dims().loci_used == L and g.engine_info().engine == 2
    return g


def _tile_launches(g, ffi):
    return g.kernel_time(ffi.K_TILE_LL)[1]


def _call(mods, g, c, name, tag):
    """one cell_log_likelihoods under masks[name]: exactly one more launch of the tile kernel, results within the bound"""
    before = _tile_launches(g, mods["ffi"])
    got = g.cell_log_likelihoods(c["alpha"], c["beta"], c["masks"][name])
    after = _tile_launches(g, mods["ffi"])
    assert after == before + 1, f"{tag}: the tile kernel ran {after - before} times in a call under mask '{name}'"
    G = S._n_partials(g.engine_info().chunk_groups, L, ())
    S._check(f"{tag}, mask '{name}'", got, c["refs"][name], G)
    return got


@pytest.mark.parametrize("sb", [2, 4])
def test_every_call_runs_the_tile_kernel(mods, case, sb):
    c = case
    g = _load(mods, c["coo"], sb)
    tag = f"tile_sb {sb}"
    base = _call(mods, g, c, "none", tag + " fresh ctx")
    # a caller's mask
    _call(mods, g, c, "random 30 %", tag + " fresh ctx")
    _call(mods, g, c, "chunk 1", tag + " fresh ctx")
    # a NULL mask on a ctx whose own mask has masked loci: the call's mask is "all used"
    g.set_loci_mask(c["masks"]["random 30 %"])
    S._same(base, _call(mods, g, c, "none", tag + " after set_loci_mask"), "NULL mask after set_loci_mask")
    # a caller's mask that differs from the ctx's, and the ctx's own
    _call(mods, g, c, "other 20 %", tag + " after set_loci_mask")
    _call(mods, g, c, "chunk 1", tag + " after set_loci_mask")
    _call(mods, g, c, "random 30 %", tag + " after set_loci_mask")
    assert np.array_equal(g.loci_mask(), c["masks"]["random 30 %"])  # the ctx's mask is its own still
    g.close()


def _summary(s):
    return (s.any_change, s.n_new_excluded, s.n_rescued, s.n_excluded, s.n_loci_filtered, s.median, s.iqr, s.threshold, s.n_near_threshold)


@pytest.mark.parametrize("sb", [2, 4])
def test_calls_between_iterations_leave_the_loop_alone(mods, case, sb):
    """both ctxs start from a placed mask (their own per-cell counts of masked entries are not zero); one gets calls under other
    masks between its iterations.  Its iterations' loci_used come from ITS counts: they must be the other ctx's, like every bit."""
    c = case
    ga, gb = _load(mods, c["coo"], sb), _load(mods, c["coo"], sb)
    for g in (ga, gb):
        g.set_loci_mask(c["masks"]["random 30 %"])
    want_used = c["refs"]["random 30 %"]["loci_used"]
    for it in range(4):
        for name in ("chunk 1", "none", "other 20 %"):
            _call(mods, gb, c, name, f"tile_sb {sb} before iteration {it}")
        sa, sb_ = ga.em_iteration(5.0), gb.em_iteration(5.0)
        assert _summary(sa) == _summary(sb_), it
        ca, cb = ga.cell_outputs(), gb.cell_outputs()
        for k in ca:
            assert np.array_equal(ca[k], cb[k]), (it, k)
        if it == 0:
            assert np.array_equal(cb["loci_used"], want_used)
        assert np.array_equal(ga.excluded(), gb.excluded()) and np.array_equal(ga.loci_mask(), gb.loci_mask())
    pa, pb = ga.posteriors(), gb.posteriors()
    for k in pa:
        assert np.array_equal(pa[k], pb[k]), k
    ga.close(); gb.close()
