"""GPU: the ingest build (ingest_pass1 / ingest_build, csrc/kernels_ingest.hip) swept over its geometry against an exact restatement.

Every number the library produces is computed on the two layouts this step makes from the staged COO, the by-locus CSC and the by-cell
CSR; the other GPU files meet it on matrices the generator happens to draw, behind other features, or at full size.  Here every case is
a matrix built by hand for one edge of the step (tests/ingest_reference.py: the builders, their geometry assertions and the plain-numpy
restatement, all held to the oracle on the CPU by tests/test_ingest_reference.py):

  the pass-1 tallies (k_pass1<SORTED>: a locus' run reduced inside a wave), the filter (k_used_flag, k_compact), the exclusive scans
  (k_scan_block / k_scan_add at one, two and three levels), the locus sort of an unsorted file and the by-cell sort (end_bit at n = 2^k
  and 2^k + 1), k_count / k_fill (runs across wave and block edges), k_row_ptr_from_keys (empty rows, the grid cut from nnz + 1), the
  packing of the counts at bits 32..63, and the same per shard (local cell indices, `sorted` decided after the cut, PASS1 summed).

  test_structure        every case, engine 2, one ctx holding all cells: the five PASS1 planes after ingest_coo; after ingest_finish
                        dims, locus_ids, locus_counts, entries_per_cell and csr_rows(0, N), entry order included.
  test_by_locus         every case with N >= 16, engines 1 (k_locus_stats streams the packed CSC) and 2 (its compact CSC is built from
                        it): the six integer columns of locus_outputs() for two placed sets of N / 8 < |B| < N / 4 cells.  Exempt, for
                        having fewer than 16 cells (ingest_reference.SMALL_N): row-edges-one-cell (N = 1), sort-bits-N-1, sort-bits-N-2,
                        sort-bits-N-3, empty-nnz0 and empty-L0 (N = 4).  No other case is left out.
  test_logical_shards, test_shard_without_cells, test_cell_range_ctx, test_inversions_in_the_other_shard
                        Cellector(devices=[0] * k) against the single-ctx reference; a set_shard ctx for a middle and an empty range, its
                        own PASS1 planes, then the global planes written at the exchange point.
  test_refusals         a count of 65536, a locus and a cell out of range: CELLECTOR_EINVAL naming the entry.

Empty matrices (empty-nnz0: no lines, L = 5 at mins 0; empty-L0: no locus passes): ingest_build -> cellector_ingest_finish ->
tiled_build HANDLE them, they do not refuse: every allocation is of at least one element (dev_alloc), every launch whose grid would be
zero is skipped or cut from n + 1 (g1, gcap), every kernel's loop is bounded by a pointer array that is all zeros, and tiled_build /
the passes return early at L == 0 or nloc == 0.  The two cases hold that: a READY ctx with L, nnz and every row as the restatement says.

All comparisons are of whole numbers and exact.
"""
import ctypes as C

import numpy as np
import pytest

import ingest_reference as ir
from test_gpu_tally_capacity import _place

pytestmark = pytest.mark.gpu

EXTREME = ("counts", "filter-edges-drop", "filter-edges-keep", "filter-edges-mins0", "unsorted-filter-perm", "unsorted-filter-reversed",
           "unsorted-filter-swapped")  # counts near 65535: the -80 filter may take loci (it acts on the NEXT mask: the columns stay)
H2D, D2H = 1, 2


@pytest.fixture(scope="module")
def mods(oracle_lib, hip_lib_path):
    from cellector_amd import Cellector, ffi
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpy.restype = C.c_int
    return dict(Cellector=Cellector, ffi=ffi, hip=hip)


_refs = {}


def _ref(name, cell_range=None):
    """the restatement of a case (of a cell range of it), computed once and left unchanged"""
    key = (name, cell_range)
    if key not in _refs:
        _refs[key] = ir.ref_of(ir.case(name), cell_range)
    return _refs[key]


def _first(bad):
    return int(np.nonzero(bad)[0][0])


def _check_pass1(mods, g, tag, want):
    """the PASS1 exchange buffer against [5][TL] whole numbers"""
    TL = want.shape[1]
    ptr, n = g.exchange_buffer(mods["ffi"].XCHG_PASS1)
    assert n == 5 * TL, (tag, n)
    got = np.empty(5 * TL, np.float64)
    assert mods["hip"].hipMemcpy(got.ctypes.data, ptr, got.nbytes, D2H) == 0
    got = got.reshape(5, TL)
    for k, plane in enumerate(ir.P1_PLANES):
        bad = got[k] != want[k].astype(np.float64)
        assert not bad.any(), f"{tag}: PASS1 plane {plane} differs at {int(bad.sum())} loci, first {_first(bad)}: device {got[k][_first(bad)]}, " \
                              f"restatement {want[k][_first(bad)]}"


def _write_pass1(mods, g, planes):
    ptr, n = g.exchange_buffer(mods["ffi"].XCHG_PASS1)
    buf = np.ascontiguousarray(planes, np.float64).ravel()
    assert n == buf.size
    assert mods["hip"].hipMemcpy(ptr, buf.ctypes.data, buf.nbytes, H2D) == 0


def _check_built(g, tag, ref):
    """a READY ctx against the restatement: dims, the filter's outputs, the by-cell rows with their entry order"""
    cb, ce = ref["cell_range"]
    d = g.dims()
    assert (d.total_loci, d.total_cells, d.cell_begin, d.cell_end) == (ref["TL"], ref["N"], cb, ce), tag
    assert (d.loci_used, d.nnz_used) == (ref["L"], ref["nnz_used"]), (tag, d.loci_used, d.nnz_used, ref["L"], ref["nnz_used"])
    ids = g.locus_ids()
    bad = ids != ref["locus_ids"]
    assert not bad.any(), f"{tag}: locus_ids differ first at used locus {_first(bad)}: device {ids[_first(bad)]}, restatement {ref['locus_ids'][_first(bad)]}"
    lc = g.locus_counts()
    bad = (lc != ref["locus_counts"]).any(axis=1)
    assert not bad.any(), f"{tag}: locus_counts differ first at used locus {_first(bad)} (locus {ids[_first(bad)]}): device {lc[_first(bad)]}, " \
                          f"restatement {ref['locus_counts'][_first(bad)]}"
    want_n = np.diff(ref["row_ptr"].astype(np.int64))
    epc = g.entries_per_cell()
    bad = epc.astype(np.int64) != want_n
    assert not bad.any(), f"{tag}: entries_per_cell differs first at row {_first(bad)}: device {epc[_first(bad)]}, restatement {want_n[_first(bad)]}"
    rp, ent = g.csr_rows(0, ce - cb)
    bad = rp != ref["row_ptr"]
    assert not bad.any(), f"{tag}: row_ptr differs first at row {_first(bad)}: device {rp[_first(bad)]}, restatement {ref['row_ptr'][_first(bad)]}"
    bad = ent != ref["entries"]
    if bad.any():
        i = _first(bad)
        row = int(np.searchsorted(ref["row_ptr"], i, side="right")) - 1
        raise AssertionError(f"{tag}: {int(bad.sum())} entries differ, first in row {row} at position {i - int(ref['row_ptr'][row])}: device "
                             f"(locus index, alt, ref) {[int(x[0]) for x in ir.unpack(ent[i:i + 1])]}, restatement "
                             f"{[int(x[0]) for x in ir.unpack(ref['entries'][i:i + 1])]}")


# ---- structure ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ir.CASES)
def test_structure(mods, name):
    case, ref = ir.case(name), _ref(name)
    g = mods["Cellector"](0)
    assert g.engine_info().engine == 2
    g.ingest_coo(case["TL"], case["N"], *case["coo"])
    _check_pass1(mods, g, name, ref["pass1"])
    g.ingest_finish(case["min_alt"], case["min_ref"])
    _check_built(g, name, ref)
    g.close()


# ---- the by-locus side ---------------------------------------------------------------------------------------------------------------
def _sets(N):
    """two exclusion sets of N / 8 < |B| < N / 4 cells: odd cells only, and a seeded draw.  (Below N / 4 so that an iteration can place
    the set, test_gpu_tally_capacity._place; above N / 8 so that engine 2 counts it locus-driven, csrc/tiled.h LM_NUM / LM_DEN.)"""
    k = (3 * N) // 16
    rng = np.random.default_rng(N)
    odd, drawn = np.zeros(N, bool), np.zeros(N, bool)
    odd[rng.choice(np.arange(1, N, 2), k, replace=False)] = True
    drawn[rng.choice(N, k, replace=False)] = True
    for B in (odd, drawn):
        assert N / 8 < B.sum() < N / 4
    assert not odd[0::2].any()
    return (("odd cells", odd), ("seeded cells", drawn))


@pytest.mark.parametrize("engine", [2, 1])
@pytest.mark.parametrize("name", [n for n in ir.CASES if n not in ir.SMALL_N])
def test_by_locus(mods, name, engine):
    case, ref = ir.case(name), _ref(name)
    N = case["N"]
    assert N >= 16
    g = mods["Cellector"](0)
    g.set_option("engine", engine)       # before the ingest: engine 1 keeps the packed CSC
    if engine == 1 and name in EXTREME:
        # engine 1's cell pass forms the expected term of a total above DM_CHUNK like the reference, a fold over all n + 1 pmfs of n
        # factors each (dm_expected_log_pmf, stats.rs:8-22): at n = 131070 that is 1.7e10 steps in one thread, minutes per entry.  The
        # column is a diagnostic, the placed keys replace what it feeds, and the locus pass (k_locus_stats) does not read it.
        g.set_option("compute_expected", 0)
    g.load_coo(case["TL"], N, *case["coo"], case["min_alt"], case["min_ref"])
    assert g.engine_info().engine == engine and g.dims().loci_used == ref["L"]
    for what, B in _sets(N):
        g.em_reset()
        _place(mods, g, B, N, quiet_filter=name not in EXTREME)
        got, want = g.locus_outputs(), ir.tallies(ref, B)
        for k in ir.KEYS:
            bad = got[k] != want[k]
            assert not bad.any(), (f"{name}, engine {engine}, {what}: {k} differs at {int(bad.sum())} used loci, first {_first(bad)} (locus "
                                   f"{ref['locus_ids'][_first(bad)]}): device {got[k][_first(bad)]}, restatement {want[k][_first(bad)]}")
    g.close()


# ---- shards ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("name", ir.SHARD_CASES)
def test_logical_shards(mods, name, k):
    """k shards of the cells on one GPU (the partition balanced by entries: on row-edges one cell of 300 lines skews it): what the ctx
    shows of the whole matrix is the single-ctx restatement"""
    case, ref = ir.case(name), _ref(name)
    N = case["N"]
    g = mods["Cellector"](devices=[0] * k)
    g.load_coo(case["TL"], N, *case["coo"], case["min_alt"], case["min_ref"])
    bounds = g.partition().astype(np.int64)
    assert len(bounds) == k + 1 and bounds[0] == 0 and bounds[-1] == N and (np.diff(bounds) >= 0).all()
    if name == "row-edges":
        assert not np.array_equal(bounds, [N * r // k for r in range(k + 1)])
    _check_built(g, f"{name}, {k} shards (bounds {bounds.tolist()})", ref)
    g.close()


def test_shard_without_cells(mods):
    """three shards over two cells: one of them holds no cell and no entry"""
    lo, ce = [0, 0, 2, 3, 3, 5], [0, 1, 1, 0, 1, 0]
    al, re = [1, 2, 0, 3, 1, 1], [1, 0, 2, 1, 1, 0]
    ref = ir.build(6, 2, (lo, ce, al, re), 1, 1)
    assert ref["locus_ids"].tolist() == [0, 3] and ref["row_ptr"].tolist() == [0, 2, 4]
    g = mods["Cellector"](devices=[0] * 3)
    g.load_coo(6, 2, lo, ce, al, re, 1, 1)
    assert (np.diff(g.partition().astype(np.int64)) == 0).any()
    _check_built(g, "two cells, three shards", ref)
    g.close()


def _range_ctx(mods, name, cb, ce):
    """a ctx of the cells [cb, ce): its own PASS1 planes after ingest_coo; the global planes written at the exchange point; the global
    filter and the range's rows, local cell indices, after ingest_finish"""
    case, ref = ir.case(name), _ref(name, (cb, ce))
    tag = f"{name}, cells [{cb}, {ce})"
    g = mods["Cellector"](0)
    g.set_shard(cb, ce)
    g.ingest_coo(case["TL"], case["N"], *case["coo"])
    _check_pass1(mods, g, tag, ref["pass1"])
    _write_pass1(mods, g, ref["pass1_global"])
    g.ingest_finish(case["min_alt"], case["min_ref"])
    whole = _ref(name)
    assert np.array_equal(ref["locus_ids"], whole["locus_ids"]) and np.array_equal(ref["locus_counts"], whole["locus_counts"])
    _check_built(g, tag, ref)
    g.close()


@pytest.mark.parametrize("name", ir.SHARD_CASES)
def test_cell_range_ctx(mods, name):
    N = ir.case(name)["N"]
    _range_ctx(mods, name, N // 3, (2 * N) // 3)
    _range_ctx(mods, name, N // 2, N // 2)     # no cells: no entries, no rows, the global filter


def test_inversions_in_the_other_shard(mods):
    """`sorted` is decided per shard after the cell-range cut: the file is out of order only among the cells >= 160, so the shard
    [0, 160) stages an ascending file (asserted by the builder) and takes the sorted kernels; the other shard sorts; so does a ctx of
    all cells (test_structure)"""
    case = ir.case("unsorted-other-shard")
    cb, ce = case["own"]
    _range_ctx(mods, "unsorted-other-shard", cb, ce)
    _range_ctx(mods, "unsorted-other-shard", ce, case["N"])


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(mods):
    """a count above CELLECTOR_MAX_COUNT, a locus and a cell out of range: CELLECTOR_EINVAL naming the (0-based) entry; the value at the
    limit is taken (case `counts`)"""
    case = ir.case("counts")
    TL, N = case["TL"], case["N"]
    EINVAL = 1
    assert mods["ffi"].STATUS_NAMES[EINVAL] == "EINVAL"
    for col, i, value, words in ((2, 7, ir.MAX_COUNT + 1, "count above 65535"), (3, 11, ir.MAX_COUNT + 1, "count above 65535"),
                                 (0, 4, TL, f"locus {TL + 1} out of range"), (1, 19, N, f"cell {N + 1} out of range")):
        coo = [x.copy() for x in case["coo"]]
        coo[col][i] = value
        g = mods["Cellector"](0)
        with pytest.raises(mods["ffi"].CellectorError) as ei:
            g.ingest_coo(TL, N, *coo)
        assert ei.value.status == EINVAL and f"entry {i}:" in str(ei.value) and words in str(ei.value), str(ei.value)
        with pytest.raises(mods["ffi"].CellectorError):
            g.ingest_finish(case["min_alt"], case["min_ref"])     # nothing was staged
        g.close()
