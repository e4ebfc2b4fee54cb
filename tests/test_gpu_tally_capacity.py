"""GPU: the per-locus counts of the exclusion set (get_locus_log_likelihoods, main.rs:368-420) at the edges of the kernels
that form them — the 4096-locus ranges and the 16-bit LDS counters of k_minority_ranges, the signed update of the kept
counts, the growth of the transposed offsets — against exact integers from numpy.

The reference is np.bincount over the entries of the excluded cells: cells_min (entries), alt_min, ref_min per locus, the
majority side being the complement.  It is formed twice, from the COO arrays that were loaded and from what csr_rows()
returns, and the two must agree.

The exclusion set is PLACED, not grown: between em_begin and em_threshold the NORM exchange buffer is overwritten (as
test_gpu_parity.test_order_statistics_on_adversarial_keys does) with -100 for the chosen cells and -1 for the others.  Fewer
than a quarter are chosen, so both quartiles are -1, the iqr is 0, the threshold -1 and exactly the chosen cells lie below it.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ("cells_min", "cells_maj", "alt_min", "ref_min", "alt_maj", "ref_maj")


@pytest.fixture(scope="module")
def mods(oracle_lib, hip_lib_path):
    from cellector_amd import Cellector, ffi
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpy.restype = C.c_int
    return dict(Cellector=Cellector, ffi=ffi, hip=hip)


def _place(mods, g, chosen, n_cells, quiet_filter=True):
    """one EM iteration whose exclusion set is `chosen` (a boolean array); returns the summary.  quiet_filter False: the caller's
    matrix has loci the -80 filter takes (tests/test_gpu_locus_sweep.py) and it checks the filter's outcome itself."""
    assert 0 < chosen.sum() < n_cells / 4
    g.em_begin()
    ptr, m = g.exchange_buffer(mods["ffi"].XCHG_NORM)
    assert m >= n_cells
    keys = np.where(chosen, -100.0, -1.0).astype(np.float64)
    assert mods["hip"].hipMemcpy(ptr, keys.ctypes.data, n_cells * 8, 1) == 0
    g.em_threshold(5.0)
    s = g.em_finish()
    assert (s.iqr, s.threshold) == (0.0, -1.0)
    assert s.n_excluded == int(chosen.sum())
    assert np.array_equal(g.excluded(), chosen.astype(np.uint8))
    if quiet_filter:
        assert s.n_loci_filtered == 0 and g.loci_mask().all()  # (single reads: no locus comes near the -80 filter)
    return s


def _counts(L, lo, ce, al, re, chosen):
    m = chosen[ce]
    out = {}
    for tag, sel in (("min", m), ("maj", ~m)):
        out["cells_" + tag] = np.bincount(lo[sel], minlength=L).astype(np.uint64)
        out["alt_" + tag] = np.bincount(lo[sel], weights=al[sel].astype(np.float64), minlength=L).astype(np.uint64)
        out["ref_" + tag] = np.bincount(lo[sel], weights=re[sel].astype(np.float64), minlength=L).astype(np.uint64)
    return out


def _check_counts(g, L, N, coo, chosen, tag):
    lo, ce, al, re = (np.asarray(x, np.int64) for x in coo)
    assert g.dims().loci_used == L and np.array_equal(g.locus_ids(), np.arange(L, dtype=np.uint64))
    want = _counts(L, lo, ce, al, re, chosen)
    # the same from the device's own by-cell rows: entry = locus | alt << 32 | ref << 48
    rp, ent = g.csr_rows(0, N)
    assert int(rp[-1]) == len(lo)
    row = np.repeat(np.arange(N), np.diff(rp).astype(np.int64))
    e_lo = (ent & np.uint64(0xFFFFFFFF)).astype(np.int64)
    e_al = ((ent >> np.uint64(32)) & np.uint64(0xFFFF)).astype(np.int64)
    e_re = (ent >> np.uint64(48)).astype(np.int64)
    from_rows = _counts(L, e_lo, row, e_al, e_re, chosen)
    got = g.locus_outputs()
    for k in KEYS:
        assert np.array_equal(want[k], from_rows[k]), (tag, k)
        bad = np.nonzero(got[k] != want[k])[0]
        assert bad.size == 0, (f"{tag}: {k} differs at {bad.size} loci, first {bad[:5]}: device {got[k][bad[:5]]}, "
                               f"numpy {want[k][bad[:5]]}")
    return got


def _edge_matrix(L, N, seed):
    """sparse random entries (singles, some totals 5..8, a few 0 and above 8: the tier-2 and overflow paths count too) plus
    entries of many cells on the loci either side of every 4096-locus range edge, the first and the last locus"""
    rng = np.random.default_rng(seed)
    nnz = 12 * N
    lo = rng.integers(0, L, nnz)
    ce = rng.integers(0, N, nnz)
    tot = rng.choice([1, 1, 1, 1, 2, 3, 4, 5, 6, 8, 0, 11], nnz)
    al = (rng.random(nnz) * (tot + 1)).astype(np.int64)
    re = tot - al
    edges = [l for l in (0, 1, 4094, 4095, 4096, 4097, 8190, 8191, 8192, L - 2, L - 1) if 0 <= l < L]
    for l in sorted(set(edges)):
        cells = np.nonzero(rng.random(N) < 0.6)[0]
        a = rng.integers(0, 3, len(cells))
        r = rng.integers(0, 3, len(cells))
        lo = np.concatenate([lo, np.full(len(cells), l)])
        ce = np.concatenate([ce, cells])
        al = np.concatenate([al, a])
        re = np.concatenate([re, r])
    return tuple(x.astype(np.uint32) for x in (lo, ce, al, re))


@pytest.mark.parametrize("L", [4095, 4096, 4097, 8193])
def test_range_edges_all_forms_agree_with_numpy(mods, L):
    """L on either side of one and two 4096-locus ranges (LR_LOCI), entries planted on the loci around every edge.  700 of 3000
    cells are placed in the set — more than nloc / 8, so that locus_mode 2 also has to grow the transposed offsets past what the
    ingest sized them for (tiled_locus_pass), set before the ingest in one ctx and after it in another.  locus_mode 1, 2 and 0:
    every locus output equal to the bit, the six integer ones equal to numpy."""
    N = 3000
    coo = _edge_matrix(L, N, seed=L)
    rng = np.random.default_rng(5)
    chosen = np.zeros(N, bool)
    chosen[rng.choice(N, 700, replace=False)] = True
    assert chosen.sum() > N // 8 + 64
    outs = []
    for mode, before in ((1, True), (2, True), (2, False), (0, True)):
        g = mods["Cellector"](0)
        if before:
            g.set_option("locus_mode", mode)
        g.load_coo(L, N, *coo, 0, 0)
        if not before:
            g.set_option("locus_mode", mode)
        _place(mods, g, chosen, N)
        outs.append(_check_counts(g, L, N, coo, chosen, f"L={L} mode {mode}"))
        g.close()
    for o in outs[1:]:
        for k in o:
            assert np.array_equal(o[k], outs[0][k]), k


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_signed_update_of_the_kept_counts(mods, mode):
    """Both signs of the delta path: a second iteration whose placed set drops 100 cells of the first and adds 150 others (a
    change of 250 against a set of 650: the kept counts are updated, tally_plan).  tally_delta 1 against 0 to the bit, both against
    numpy; a third iteration that only rescues, a fourth without change."""
    L, N = 8193, 3000
    coo = _edge_matrix(L, N, seed=77)
    rng = np.random.default_rng(11)
    order = rng.permutation(N)
    sets = [order[:600], np.concatenate([order[100:600], order[600:750]]), order[150:750], order[150:750]]
    pair = []
    for delta in (1, 0):
        g = mods["Cellector"](0)
        g.set_option("tally_delta", delta)
        g.set_option("locus_mode", mode)
        g.load_coo(L, N, *coo, 0, 0)
        pair.append(g)
    for it, ids in enumerate(sets):
        chosen = np.zeros(N, bool)
        chosen[ids] = True
        got = []
        for g in pair:
            s = _place(mods, g, chosen, N)
            got.append(_check_counts(g, L, N, coo, chosen, f"iteration {it} mode {mode}"))
        if it == 1:
            assert (s.n_new_excluded, s.n_rescued) == (150, 100)
        for k in got[0]:
            assert np.array_equal(got[0][k], got[1][k]), (it, k)
    for g in pair:
        g.close()


def _repeated_pair_matrix(N, L, repeats, seed):
    """every cell: the line (locus 0, cell, alt = 1, ref = 0) `repeats` times, and four single reads at random other loci"""
    rng = np.random.default_rng(seed)
    ce = np.repeat(np.arange(N), repeats + 4)
    lo = np.concatenate([np.zeros((N, repeats), np.int64), rng.integers(1, L, (N, 4))], axis=1).ravel()
    al = np.concatenate([np.ones((N, repeats), np.int64), rng.integers(0, 2, (N, 4))], axis=1).ravel()
    re = np.where(lo == 0, 0, 1 - al)
    return tuple(x.astype(np.uint32) for x in (lo, ce, al, re))


def _capacity_case(mods, N, L, repeats, n_chosen, modes):
    """one ctx, one placed set per entry of n_chosen (an int or a list), every locus_mode on each"""
    coo = _repeated_pair_matrix(N, L, repeats, seed=repeats)
    g = mods["Cellector"](0)
    g.set_option("tally_delta", 0)  # every iteration recounts the whole set: one ctx serves every locus_mode and every set
    g.load_coo(L, N, *coo, 0, 0)
    info = g.engine_info()
    print(f"  {N} cells x {L} loci: {info.cell_blocks} x {info.locus_chunks} tiles, {info.tile_bytes / 2**20:.0f} MiB of tiles")
    try:
        for n in ([n_chosen] if isinstance(n_chosen, int) else n_chosen):
            chosen = np.zeros(N, bool)
            chosen[np.random.default_rng(3).choice(N, n, replace=False)] = True
            for mode in modes:
                g.set_option("locus_mode", mode)
                _place(mods, g, chosen, N)
                got = _check_counts(g, L, N, coo, chosen, f"{repeats} lines per pair, {n} cells, mode {mode}")
                assert got["cells_min"][0] == repeats * n and got["alt_min"][0] == repeats * n
    finally:
        g.close()


def test_counter_carry_three_lines_per_pair(mods):
    """A (locus, cell) pair may be listed any number of times and every line is an entry (load_data.rs:165-173,
    test_gpu_deep.test_repeated_locus_cell_lines_are_separate_entries).  200 000 cells x 530 000 loci: 130 ranges of 4096 loci, more
    than half the CUs, so the exclusion set is ONE subset (lr_sub = 1, tiled_build); every cell lists (locus 0, alt 1) three
    times; 25 000 cells (nloc / 8: what the automatic mode still hands to the minority-driven form) are placed in the set: 75 000
    counts on the u16 LDS counter of (locus 0, code 0) in k_minority_ranges.  Without a bound that knows the matrix, 75 000 wraps to
    9 464 and carries one into the counter beside it (locus 1).  locus_mode 0 and 2.  (With the bound a subset of this matrix holds
    65535 / 3 = 21 845 cells, so this set is counted by the streamed form: the next test sits on that edge.)

    Device memory, under 2 GB: 196 cell blocks x 830 chunks = 162 680 tiles of at least 4 KiB (64 rows x 16 slices x one
    padding entry + the cell id) = 0.67 GB with 42 MB of headers; the builder's offsets toff = 200 000 x 831 x 4 B = 0.66 GB
    (released after the build, its block then serves the 4 x 830 chunk tables of 92 KB = 0.31 GB); roff = 200 000 x 131 x 4 B =
    0.10 GB and as much again for the transposed offsets of locus_mode 2; the count planes 3 x 530 000 x 64 B = 0.10 GB."""
    _capacity_case(mods, 200_000, 530_000, 3, 25_000, (0, 2))


def test_counter_edge_three_lines_per_pair(mods):
    """Either side of the divisor: three lines per pair and ONE subset (530 000 loci) of 21 845 cells put 65 535 on a u16 counter,
    its largest value, in the minority-driven form (locus_mode 2); 21 846 cells would wrap to 2 and must go to the streamed form
    instead.  Both against numpy.  90 000 cells (21 846 is less than a quarter).

    Device memory, under 2 GB: 88 x 830 tiles = 0.30 GB, toff 0.30 GB, chunk tables 0.31 GB, roff and the transposed offsets
    2 x 90 000 x 131 x 4 B = 0.09 GB, count planes 0.10 GB."""
    _capacity_case(mods, 90_000, 530_000, 3, [21_845, 21_846], (2,))


def test_counter_boundary_two_lines_per_pair(mods):
    """The boundary that must keep working in the minority-driven form: two lines per pair and a subset of 32 767 cells put
    65 534 on one u16 counter.  140 000 cells (32 767 is less than a quarter), locus_mode 2.

    Device memory, under 2 GB: 137 x 830 = 113 710 tiles = 0.47 GB, toff = 140 000 x 831 x 4 B = 0.47 GB, chunk tables 0.31 GB,
    roff and the transposed offsets 2 x 140 000 x 131 x 4 B = 0.15 GB, count planes 0.10 GB."""
    _capacity_case(mods, 140_000, 530_000, 2, 32_767, (2, 1))


def test_subsets_of_a_matrix_with_many_lines_per_pair(mods):
    """Several subsets (4097 loci: two ranges, lr_sub = 16) and a pair listed 70 times: a subset of this matrix may hold
    65535 / 70 = 936 cells, less than the 1024 a subset otherwise takes at least (TALLY_SUB_CELLS).  Sets of 1 000 cells (one subset of
    1 000 would put 70 000 on a counter), 2 040 (two of 1 020: 71 400) and 936 (65 520: fits) are placed; a set of 15 000 (more than
    16 x 936) goes to the streamed form.  locus_mode 2 and 0 (17 000 cells: 2 040 is nloc / 8 and less), then the signed update of the kept
    counts with changes of that size."""
    N, L, repeats = 17_000, 4097, 70
    _capacity_case(mods, N, L, repeats, [1_000, 2_040, 936], (2, 0))
    _capacity_case(mods, 64_000, L, repeats, [15_000], (2,))
    # the delta path: 1 000 cells added to a set of 1 100, then 1 000 others rescued
    coo = _repeated_pair_matrix(N, L, repeats, seed=repeats)
    order = np.random.default_rng(8).permutation(N)
    pair = []
    for delta in (1, 0):
        g = mods["Cellector"](0)
        g.set_option("tally_delta", delta)
        g.set_option("locus_mode", 2)
        g.load_coo(L, N, *coo, 0, 0)
        pair.append(g)
    for it, ids in enumerate((order[:1100], order[:2100], order[1000:2100])):
        chosen = np.zeros(N, bool)
        chosen[ids] = True
        got = [(_place(mods, g, chosen, N), _check_counts(g, L, N, coo, chosen, f"70 lines per pair, delta iteration {it}"))[1] for g in pair]
        for k in got[0]:
            assert np.array_equal(got[0][k], got[1][k]), (it, k)
    for g in pair:
        g.close()
