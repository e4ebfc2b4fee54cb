"""GPU: who looks a row's tier-2 entries up must not change a bit (csrc/kernels_tiled.hip, k_t2_cell / launch_overflow_cell).

The tier-2 cell lookups take their 64-row groups from a device counter that the k_t2_tables launch in front of them resets, and
two grids can draw from it: the co-resident one-wave blocks (option t2_waves) and a helper grid of four-wave blocks that ask for
LDS they do not use, so that they are placed on the CUs the tile grid leaves free (option t2_helper; a forced value launches it
even where no CU is free, which is the case at these sizes, and in the posterior phase, where the automatic setting launches none).  A row belongs to one lane, which adds the row's values in the row's
order, so every deal gives the same sums: the outputs are compared with ==, never approx, across

    t2_helper 0 / 1 / 8 (forced)   x   t2_waves 1 / 512      beside the tile kernel (overlap 1), and the defaults

and against overlap 0 (everything on one stream, no helper), at both bank_order values and compute_expected 0 / 1:
cell_outputs() after each of three iterations, the three iteration summaries, and posteriors() (three more lookup passes, one per
table set).  (Non-temporal loads in the lookup kernel were measured, lost and are not in the source: there is no t2_nt to set.)
With compute_expected 0 no pass forms expected_ll (the array keeps what an earlier pass left), so it is compared
where compute_expected is 1.

Shapes: 2 000 synthetic loci at density 0.05, entry totals 1 + Geometric(0.55) (synth_continue_pct 45), every locus used
(min_alt = min_ref = 0: a single cell would pass no locus through the default filter).  1 cell; 63, 64, 65 cells (one group, ragged
/ full / two groups); 130 cells (three groups, the last with two rows); 5 000 cells (79 groups: more than the co-resident blocks
at t2_waves 1, fewer than the 256 helper blocks of t2_helper 8 on a 256-CU device).
At that coverage 4.1 % of the entries have totals above 4, more than the 3 % beyond which the ingest chooses the deep layouts
(which have no lookup kernel), so the shallow layouts are asked for with ovf_deep 0 before the ingest; engine_info() has no flag
for the choice, so what is asserted through it is that overflow entries exist and are a small share of the matrix.
"""
import itertools

import numpy as np
import pytest

N_LOCI, DENSITY = 2000, 0.05
SHAPES = [1, 63, 64, 65, 130, 5000]
SETTINGS = [dict(t2_helper=h, t2_waves=w) for h, w in itertools.product((0, 1, 8), (1, 512))] + [dict(t2_helper=-1, t2_waves=0)]


@pytest.fixture(scope="module")
def mods(hip_lib_path):
    from cellector_amd import Cellector
    return dict(Cellector=Cellector)


def _load(mods, n_cells, bank_order, seed=11):
    """the shape with overflow entries on the shallow path; a shape without any gets a higher density"""
    density = DENSITY
    while True:
        g = mods["Cellector"](0)
        g.set_option("synth_continue_pct", 45)
        g.set_option("ovf_deep", 0)
        g.set_option("bank_order", bank_order)
        g.load_synthetic(N_LOCI, n_cells, density, seed=seed, min_alt=0, min_ref=0)
        info = g.engine_info()
        if info.nnz_overflow or density >= 1.0:
            break
        g.close()
        density = min(1.0, density * 2)
    print(f"  {n_cells} cells, bank_order {bank_order}, density {density}: {info.nnz_regular} regular + {info.nnz_overflow} overflow entries")
    assert info.engine == 2 and info.nnz_overflow > 0
    assert info.nnz_overflow * 5 < info.nnz_regular  # a small share: the side-chain arrangement, not a deep matrix
    return g


def _run(g, compute_expected, opts):
    """three iterations from the ingest's state and the posterior phase: everything a caller can read, as a flat list of arrays"""
    for k, v in opts.items():
        g.set_option(k, v)
    g.set_option("compute_expected", compute_expected)
    g.em_reset()
    out = []
    for _ in range(3):
        s = g.em_iteration(5.0)
        out.append(("summary", np.array([float(getattr(s, f)) for f, _ in s._fields_])))
        for k, v in g.cell_outputs().items():
            if k != "expected_ll" or compute_expected:
                out.append((k, v))
    out += list(g.posteriors().items())
    return out


def _same(a, b):
    """== per element; a NaN (a cell without a used locus has no normalized value) only against a NaN"""
    return (a == b) | (np.isnan(a) & np.isnan(b))


def _assert_same(got, want, what):
    assert [k for k, _ in got] == [k for k, _ in want]
    for i, ((k, a), (_, b)) in enumerate(zip(got, want)):
        assert a.shape == b.shape and _same(a, b).all(), f"{what}: output {i} ({k}) differs in {int((~_same(a, b)).sum())} places"


@pytest.mark.gpu
@pytest.mark.parametrize("n_cells", SHAPES)
def test_deal_changes_no_bit(mods, n_cells):
    for bank_order in (1, 0):
        g = _load(mods, n_cells, bank_order)
        for ce in (1, 0):
            want = _run(g, ce, dict(overlap=0, t2_helper=0, t2_waves=512))
            for st in SETTINGS:
                _assert_same(_run(g, ce, dict(overlap=1, **st)), want, f"{n_cells} cells, bank_order {bank_order}, compute_expected {ce}, {st}")
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_cells", [130, 5000])
def test_counter_reset_outside_em(mods, n_cells):
    """cellector_cell_log_likelihoods under a caller's alpha/beta, twice in a row: a pass that does not go through the EM path
    resets the counter too (a counter left at its end value would leave every row of the second call without its lookups)"""
    g = _load(mods, n_cells, 1)
    L = g.dims().loci_used
    rng = np.random.default_rng(5)
    alpha, beta = 0.5 + 3.0 * rng.random(L), 0.5 + 3.0 * rng.random(L)
    g.set_option("compute_expected", 1)
    g.set_option("overlap", 0)
    want = g.cell_log_likelihoods(alpha, beta)
    assert np.abs(want[0]).sum() > 0
    for st in (dict(t2_helper=0, t2_waves=1), dict(t2_helper=8, t2_waves=1), dict(t2_helper=1, t2_waves=512)):
        g.set_option("overlap", 1)
        for k, v in st.items():
            g.set_option(k, v)
        for call in range(2):
            got = g.cell_log_likelihoods(alpha, beta)
            for a, b, name in zip(got, want, ("ll", "expected_ll", "loci_used")):
                assert _same(a, b).all(), f"{n_cells} cells, {st}, call {call}: {name} differs in {int((~_same(a, b)).sum())} places"
    g.close()
