"""GPU: the tiled cell pass (k_tile_ll, csrc/kernels_tiled.hip) swept over its dispatch space against an exact sum.

The small parity tests reach one corner of that kernel's twelve instances (EXPECTED x columns of 2 or 4 cell blocks x three
tile geometries) and compare at 1e-7, the ORACLE's ln_gamma cancellation noise.  Here every case forces its geometry (options
tile_sb, tile_groups, t2_tiles, ovf_deep; min_alt = min_ref = 0 so that every locus is used), asserts that it got it
(dims().loci_used, engine_info()'s blocks / chunks / groups, and for the persistent loop's second trip columns x groups > CUs),
calls cell_log_likelihoods(alpha, beta) with alpha, beta log-uniform in [1, 1e4] and not whole — all table values distinct,
none negligible — and compares EVERY cell with tests/tile_reference.py (80-bit products, exact ln C) within a bound derived
from the device's operation count.  A dropped, duplicated or misrouted lookup moves a cell by about ln(alpha + beta) ~ 1..9;
the bound is ~1e-13.

The device's bound (u = 2^-53, the largest relative error of one rounded double operation; nothing here is fitted to observed errors)

  Per term, B_term(n, a, t), csrc/device_math.h dm_log_bb_pmf = ln C + dm_log_beta_ratio:
    * (2 n + 2 + ceil(n / 8)) roundings of u on the ratio(s) — the products of the n factors above and below, the sum alpha + beta
      and one division per chunk of eight factors — relative on a ratio, hence absolute on its log;
    * one ulp of each of the ceil(n / 8) log results (the device's f64 log is documented as 1 ulp: ROCm device-libs, ocml
      "log: 1 ulp" for double precision), at that log's magnitude, which the reference knows because it splits the product the same way;
    * ln C(n, a) = lf[n] - lf[a] - lf[n - a]: half an ulp of ln(n!) for each of the three table values, 1.5 ulp in all
      (tests/test_tile_reference.py measures this part against the table arithmetic itself, which is host arithmetic); a value
      beyond the table (x > 170: statrs' Lanczos ln_gamma, dm_ln_gamma) instead carries that formula's own count,
      tile_reference.lanczos_bound — about 1e3 u, all of it the cancellation of its alternating series.
  Per cell: sum of B_term + (m + G) u sum |term|, m the cell's entry count (the additions inside the partial sums, in whatever
    order), G the partial sums added at the end: the chunk groups, the tier-2 tile set's groups (at most min(64, its chunks)) and
    the overflow sum.  Plus half an ulp of the reference's own rounding to double.
  Expected terms: tile_reference.expected_bound (the ratio recurrence's count), summed the same way.
  A single-entry probe cell's ll IS the term (adding zeros is exact): held to B_term alone.

The 1e-7 of the other GPU files stays what comparisons with the oracle use (the EM / posterior runs below).

A caller-given mask sends cell_log_likelihoods to the CSR kernel (cellector_cell_log_likelihoods: the tiled pass takes the used-locus
counts from the ctx's own mask), so the mask cases below check that entry point, not k_tile_ll; masked loci reach the tile kernel
through the EM runs' own locus filter (test_em_and_posteriors: a planted locus, and in one case a whole chunk, that the -80
filter masks, the EM pass at the fixed point held to the tight bound).  A pass with every locus masked never runs through k_tile_ll.

Worst observed / bound ratios are printed per case (pytest -s).
"""
import numpy as np
import pytest

import tile_reference as tr

pytestmark = pytest.mark.gpu

BLU = 639  # loci per chunk of the regular tiles (T_BL - 1); the tier-2 tile sets: 338 (totals 5..8) and 767 (5..6)
T2_BLU = {8: 338, 6: 767}
T_GROUPS_MAX, T_GROUPS = 64, 8


@pytest.fixture(scope="module")
def mods(oracle_lib, hip_lib_path):
    import torch
    from cellector_amd import Cellector, ffi
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    return dict(Cellector=Cellector, ffi=ffi, ob=oracle_lib, ncu=ncu)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def _alpha_beta(L, seed):
    rng = np.random.default_rng(1000 + seed)
    return 10.0 ** rng.uniform(0, 4, L), 10.0 ** rng.uniform(0, 4, L)


SHALLOW = [1] * 12 + [2] * 5 + [3, 3, 4, 4] + [0, 5, 6, 8, 9, 13, 17, 18, 25]   # ~70 % singles, 30 % of the kinds beyond the tables
DEEP = [1] * 6 + [2] * 3 + [3, 3, 4, 4] + [5, 5, 6, 6, 7, 8] + [0, 9, 12, 17, 21]  # totals 5..8: a quarter of the entries


def _random_coo(seed, L, N, nnz, totals=SHALLOW):
    """nnz entries at random (locus, cell) pairs (a pair drawn twice is two entries), totals drawn from `totals`, alt uniform"""
    rng = np.random.default_rng(seed)
    lo = rng.integers(0, L, nnz)
    ce = rng.integers(0, N, nnz)
    tot = rng.choice(totals, nnz)
    al = (rng.random(nnz) * (tot + 1)).astype(np.int64)
    return [lo, ce, al, tot - al]


def _plant(coo, loci, N, seed, frac=0.3, totals=(1, 1, 2, 3, 4)):
    """entries of a share of the cells on each of `loci` (the loci either side of a chunk edge)"""
    rng = np.random.default_rng(seed)
    for l in sorted(set(int(x) for x in loci)):
        cells = np.nonzero(rng.random(N) < frac)[0]
        if len(cells) == 0:
            cells = np.array([0])
        tot = rng.choice(totals, len(cells))
        al = (rng.random(len(cells)) * (tot + 1)).astype(np.int64)
        for i, v in enumerate((np.full(len(cells), l), cells, al, tot - al)):
            coo[i] = np.concatenate([coo[i], v])
    return coo


def _u32(coo):
    return tuple(np.ascontiguousarray(x, dtype=np.uint32) for x in coo)


def _edge_loci(L, blu):
    out = [0, L - 1]
    for e in range(blu, L + 2, blu):
        out += [e - 2, e - 1, e, e + 1]
    return [l for l in out if 0 <= l < L]


# ---- geometry ----------------------------------------------------------------------------------------------------------------
def _groups_for(nb, nj, ncu, opt):
    """tile_groups_for + the rounding of tiled_build: (groups, chunks per group)"""
    cols = (nb + 3) // 4
    groups, best = 1, 1e300
    for g in range(1, min(T_GROUPS_MAX, nj) + 1):
        per = min(max(ncu // g, 1), cols)
        rounds, chunks = -(-cols // per), -(-nj // g)
        cost = rounds * (chunks + 3) * (1.0 + 0.03 * ((g - T_GROUPS) / T_GROUPS if g > T_GROUPS else 0.0))
        if cost < best:
            best, groups = cost, g
    if opt > 0:
        groups = opt
    groups = min(groups, nj)
    cpg = -(-nj // groups)
    return -(-nj // cpg), cpg


def _load(mods, L, N, coo, opts=()):
    g = mods["Cellector"](0)
    for k, v in opts:
        g.set_option(k, v)
    g.load_coo(L, N, *_u32(coo), 0, 0)
    return g


def _assert_geometry(mods, g, L, N, coo, opts):
    """the case is the one intended: every locus used, blocks / chunks / groups as computed here, regular / overflow split"""
    o = dict(opts)
    d, info = g.dims(), g.engine_info()
    assert (d.loci_used, d.total_cells, d.nnz_used) == (L, N, len(coo[0]))
    nb, nj = max(1, -(-N // 1024)), max(1, -(-L // BLU))
    groups, cpg = _groups_for(nb, nj, mods["ncu"], o.get("tile_groups", 0))
    assert (info.engine, info.cell_blocks, info.locus_chunks, info.chunk_groups) == (2, nb, nj, groups), \
        (info.cell_blocks, info.locus_chunks, info.chunk_groups, nb, nj, groups)
    tot = np.asarray(coo[2]) + np.asarray(coo[3])
    n_reg = int(((tot >= 1) & (tot <= 4)).sum())
    assert (info.nnz_regular, info.nnz_overflow) == (n_reg, len(tot) - n_reg)
    # the 1.5 ulp figure of ln C is measured to hold for totals up to 64 and is exceeded once above (C(125, 40),
    # tests/test_tile_reference.py): no case may draw a total it is not established for
    assert not ((tot > 64) & (tot <= 170)).any()
    # which tier-2 tile set the ingest built: engine_info does not say, but once a matrix is loaded option t2_tiles accepts the
    # value that was built and refuses the others (cellector_set_option: "set it before the ingest")
    if "t2_tiles" in o:
        for v in (0, 6, 8):
            if v == o["t2_tiles"]:
                g.set_option("t2_tiles", v)
            else:
                with pytest.raises(mods["ffi"].CellectorError):
                    g.set_option("t2_tiles", v)
    return nb, nj, groups, cpg


def _n_partials(groups, L, opts):
    t2 = dict(opts).get("t2_tiles", 0)
    g2 = min(T_GROUPS_MAX, -(-L // T2_BLU[t2])) if t2 in T2_BLU else 0
    return groups + g2 + 1


# ---- comparison --------------------------------------------------------------------------------------------------------------
def _ratio(diff, bound):
    """largest diff / bound; a zero bound wants a zero difference"""
    assert (diff[bound == 0] == 0).all(), "a cell whose bound is zero (no entries, or only zero-total ones) must be exact"
    nz = bound > 0
    return float((diff[nz] / bound[nz]).max()) if nz.any() else 0.0


def _check(tag, got, ref, n_partials, expected=True, probes=False):
    """every cell: ll and expected_ll within the per-cell bound, loci_used exactly; returns the worst observed / bound"""
    ll, ell, nl = got
    assert np.isfinite(ll).all() and np.isfinite(ell).all(), tag
    assert np.array_equal(nl, ref["loci_used"]), (tag, np.nonzero(nl != ref["loci_used"])[0][:8])
    if probes:  # one entry per cell: the term itself
        b_ll, b_ell = ref["b_ll"].copy(), ref["b_ell"].copy()
    else:
        b_ll, b_ell = tr.cell_bound(ref, n_partials)
    b_ll = b_ll + np.where(b_ll > 0, 0.5 * np.spacing(np.abs(ref["ll"])), 0.0)
    b_ell = b_ell + np.where(b_ell > 0, 0.5 * np.spacing(np.abs(ref["expected_ll"])), 0.0)
    d_ll, d_ell = np.abs(ll - ref["ll"]), np.abs(ell - ref["expected_ll"])
    r_ll = _ratio(d_ll, b_ll)
    r_ell = _ratio(d_ell, b_ell) if expected else 0.0
    print(f"  {tag}: worst |ll - ref| / bound = {r_ll:.3f} (largest bound {b_ll.max():.2e})"
          + (f", expected_ll {r_ell:.3f} ({b_ell.max():.2e})" if expected else ""))
    bad = np.nonzero(d_ll > b_ll)[0]
    assert bad.size == 0, (f"{tag}: ll beyond its bound at {bad.size} of {len(ll)} cells, first {bad[:6]}: device {ll[bad[:6]]}, "
                           f"reference {ref['ll'][bad[:6]]}, bound {b_ll[bad[:6]]}, entries {ref['count'][bad[:6]]}")
    if expected:
        bad = np.nonzero(d_ell > b_ell)[0]
        assert bad.size == 0, (f"{tag}: expected_ll beyond its bound at {bad.size} cells, first {bad[:6]}: device {ell[bad[:6]]}, "
                               f"reference {ref['expected_ll'][bad[:6]]}, bound {b_ell[bad[:6]]}")
    return max(r_ll, r_ell)


def _same(a, b, tag, cols=(0, 1, 2)):
    for i in cols:
        assert np.array_equal(a[i], b[i]), f"{tag}: output {i} differs at {np.nonzero(a[i] != b[i])[0][:8]}"


def _sweep(mods, tag, L, N, coo, opts=(), sbs=(2, 4, 0), orders=(1, 0), seed=0, second_trip=False, probes=False):
    """One matrix: reference once; for bank_order 1 and 0 a ctx each; every column width; widths agree to the bit."""
    alpha, beta = _alpha_beta(L, seed)
    ref = tr.cell_reference(N, *coo, alpha, beta)
    worst = 0.0
    for order in orders:
        o = tuple(opts) + (("bank_order", order),)
        g = _load(mods, L, N, coo, o)
        nb, nj, groups, cpg = _assert_geometry(mods, g, L, N, coo, o)
        runs = {}
        for sb in sbs:
            g.set_option("tile_sb", sb)
            if second_trip:
                assert sb in (2, 4) and -(-nb // sb) * groups > mods["ncu"], (nb, sb, groups, mods["ncu"])
            runs[sb] = g.cell_log_likelihoods(alpha, beta)
            worst = max(worst, _check(f"{tag} bank_order {order} tile_sb {sb}", runs[sb], ref, _n_partials(groups, L, o),
                                      probes=probes))
        for sb in sbs[1:]:  # the summation order of a cell does not depend on the column width
            _same(runs[sbs[0]], runs[sb], f"{tag} bank_order {order}: tile_sb {sbs[0]} against {sb}")
        g.close()
    return worst


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def test_option_tile_sb_values(mods):
    g = mods["Cellector"](0)
    for v in (0, 2, 4):
        g.set_option("tile_sb", v)
    for v in (1, 3, 8, -1):
        with pytest.raises(mods["ffi"].CellectorError) as e:
            g.set_option("tile_sb", v)
        assert e.value.status == 1  # CELLECTOR_EINVAL
    g.close()


@pytest.mark.parametrize("N", [1, 1023, 1024, 1025, 3 * 1024 + 1, 5 * 1024, 7 * 1024 + 3])
def test_ragged_blocks_and_columns(mods, N):
    """Cell counts around a block and around columns of 2 and 4 blocks (nb = 1, 1, 1, 2, 4, 5, 8: nb % 4 in {1, 2, 0}, a last
    block of 1, 3 and 1023 cells), three chunks; tile_sb 2, 4 and the automatic rule."""
    L = 3 * BLU - 17
    coo = _plant(_random_coo(N, L, N, 25 * N + 40), _edge_loci(L, BLU), N, seed=N)
    _sweep(mods, f"ragged N={N}", L, N, coo, seed=N)


@pytest.mark.parametrize("L", [1, 638, 639, 640, 1278, 1279, 7 * 639 + 1])
def test_chunk_edges(mods, L):
    """Locus counts around one, two and seven chunks of 639 (the last chunk full, one short, one locus long), entries of a third of
    the cells planted on the loci either side of every chunk edge.  2100 cells: three blocks, the last ragged."""
    N = 2100
    coo = _plant(_random_coo(L, L, N, 8 * N), _edge_loci(L, BLU), N, seed=L)
    _sweep(mods, f"chunks L={L}", L, N, coo, seed=L)


@pytest.mark.parametrize("nj,N", [(7, 2100), (64, 1025)])
@pytest.mark.parametrize("groups", [0, 1, 2, 3, 5, 64])
def test_chunk_groups(mods, nj, N, groups):
    """tile_groups forced on 7 chunks (3 and 5 do not divide it: groups of 3, 3, 1 and of 2, 2, 2, 1 chunks; 64 is clamped to 7
    groups of one chunk) and on 64 chunks (64: one chunk per group, 5: groups of 13 and one of 12).  Every count agrees with the
    reference within the bound — hence with tile_groups 1 within twice the bound, not to the bit (include/cellector_ffi.h)."""
    L = nj * BLU
    coo = _plant(_random_coo(nj + groups, L, N, 30 * N), _edge_loci(L, BLU), N, seed=nj, frac=0.1)
    _sweep(mods, f"groups nj={nj} tile_groups={groups}", L, N, coo, opts=(("tile_groups", groups),), seed=nj)


def _second_trip_coo(seed=3):
    """17 400 cells (nb = 18: ragged for columns of 4) x 40 300 loci (64 chunks, the last of 43 loci), 2.8 M entries (density 0.004),
    totals 1 + Geometric(0.7) like vartrix counts (2 % beyond the tables)"""
    N, L, nnz = 17_400, 40_300, 2_800_000
    rng = np.random.default_rng(seed)
    lo = rng.integers(0, L, nnz)
    ce = rng.integers(0, N, nnz)
    tot = rng.geometric(0.7, nnz)
    al = (rng.random(nnz) * (tot + 1)).astype(np.int64)
    return N, L, [lo, ce, al, tot - al]


def test_second_trip_of_the_persistent_loop(mods):
    """tile_groups 64 on 64 chunks leaves each group ncu / 64 workgroups (4 on 256 CUs) for 9 columns of two blocks or 5 of four:
    every workgroup fetches a second column and clears its accumulators again behind the barrier at the top of the loop.  Asserted:
    columns x groups > CUs.  Device memory: 18 x 64 tiles, 6 MB of entries; nothing of note."""
    N, L, coo = _second_trip_coo()
    _sweep(mods, "second trip", L, N, coo, opts=(("tile_groups", 64),), sbs=(2, 4), seed=5, second_trip=True)


def _row_length_coo(seed=9):
    """Cells with exactly k entries in chunk 1 of three chunks.
    block 0: 60 cells of each k in 0, 1, 2, 6, 7, 8, 9, 14, 15, 16, 17, 31, 62, 63, 64, 200, 639 (the builder sorts a tile's rows by
             length: slices of mixed lengths, the long ones on the loop beyond T_NE = 15 entries; a tile above TB_STAGE);
    block 1: k in {0, 1}: every slice of one lookup;
    block 2: 128 cells each of k = 1, 2, {6, 7}, {8, 9}, {14, 15}, {16, 17}, 31, {62, 63}: slices whose K is 1, 3, 7 (the second 16-byte
             load repeats the first), 9, 15 (all registers), 17 (first trip of the loop), 31, 63; 19 712 u16: below TB_STAGE;
    block 3: empty cells only;
    block 4: every row full, 639 entries (written directly, K = 639);
    block 5: 300 cells (ragged), k random in 0..20.
    Chunks 0 and 2 hold a few entries of every third cell."""
    rng = np.random.default_rng(seed)
    L = 3 * BLU
    ks = []
    ks += [k for k in (0, 1, 2, 6, 7, 8, 9, 14, 15, 16, 17, 31, 62, 63, 64, 200, 639) for _ in range(60)] + [0] * 4
    ks += list(rng.integers(0, 2, 1024))
    for pair in ((1, 1), (2, 2), (6, 7), (8, 9), (14, 15), (16, 17), (31, 31), (62, 63)):
        ks += [pair[i % 2] for i in range(128)]
    ks += [0] * 1024
    ks += [639] * 1024
    ks += list(rng.integers(0, 21, 300))
    ks = np.array(ks)
    N = len(ks)
    assert N == 5 * 1024 + 300
    perm = np.arange(1024)
    rng.shuffle(perm)
    ks[:1024] = ks[:1024][perm]  # (block 0 in mixed order)
    lo, ce = [], []
    for c in np.nonzero(ks)[0]:
        k = int(ks[c])
        lo.append(BLU + (np.arange(BLU) if k == BLU else rng.choice(BLU, k, replace=False)))
        ce.append(np.full(k, c))
    for c in range(0, N, 3):
        if 3 * 1024 <= c < 4 * 1024:
            continue
        k = int(rng.integers(1, 5))
        lo.append(np.concatenate([rng.integers(0, BLU, k), rng.integers(2 * BLU, 3 * BLU, k)]))
        ce.append(np.full(2 * k, c))
    lo, ce = np.concatenate(lo), np.concatenate(ce)
    tot = rng.choice([1, 1, 1, 2, 2, 3, 4], len(lo))
    al = (rng.random(len(lo)) * (tot + 1)).astype(np.int64)
    coo = [lo, ce, al, tot - al]
    per_cell_chunk1 = np.bincount(ce[(lo >= BLU) & (lo < 2 * BLU)], minlength=N)
    assert np.array_equal(per_cell_chunk1, ks)
    assert np.bincount(ce, minlength=N)[3 * 1024:4 * 1024].sum() == 0
    return N, L, coo


def test_row_lengths(mods):
    N, L, coo = _row_length_coo()
    _sweep(mods, "row lengths", L, N, coo, seed=2)
    # the same rows with one overflow entry among them (the builder puts a padding entry in its place) and a zero-total one
    rng = np.random.default_rng(4)
    pick = rng.random(len(coo[0])) < 0.02
    coo2 = [x.copy() for x in coo]
    coo2[2][pick] = rng.choice([0, 3, 9], int(pick.sum()))
    coo2[3][pick] = rng.choice([0, 4, 11], int(pick.sum()))
    _sweep(mods, "row lengths with overflow entries", L, N, coo2, sbs=(4, 2), seed=2)


PROBES = ([(1, 0), (0, 1), (2, 0), (1, 1), (0, 2), (3, 0), (2, 1), (1, 2), (0, 3), (4, 0), (3, 1), (2, 2), (1, 3), (0, 4)]
          + [(0, 0)] + [(n - r, r) for n in (5, 6, 7, 8) for r in (0, n // 2, n)] + [(4, 5), (9, 0), (8, 9), (0, 17), (9, 9), (18, 0)]
          + [(20, 20), (3, 37), (100, 71), (171, 0), (1, 170), (120, 120), (200, 40), (0, 240)])


@pytest.mark.parametrize("opts", [(), (("t2", 0),), (("ovf_deep", 1), ("t2_tiles", 8)), (("ovf_deep", 1), ("t2_tiles", 6)),
                                  (("ovf_deep", 1), ("t2_tiles", 0))], ids=["default", "t2=0", "deep-t8", "deep-t6", "deep-t0"])
def test_single_entry_probes(mods, opts):
    """A cell whose only entry is (alt, ref) at a first, a middle and a last slot of a chunk: each of the 14 regular codes, and totals
    0, 5..8, 9, 17, 18, 40, 171 and 240 (beyond 170: the ln_gamma branch of ln n!).  Its ll is that term, held to B_term; its
    expected_ll the expected term.  Under every layout the totals 5..8 and above can take."""
    slots = [0, 319, 638, 639, 639 + 337, 639 + 338, 2 * 639 - 1, 2 * 639 + 100]
    L = 2 * BLU + 128
    lo, ce, al, re = [], [], [], []
    for a, r in PROBES:
        for s in slots:
            ce.append(len(ce)); lo.append(s); al.append(a); re.append(r)
    N = len(ce)
    coo = [np.array(x, dtype=np.int64) for x in (lo, ce, al, re)]
    _sweep(mods, "probes " + (",".join(f"{k}={v}" for k, v in opts) or "default"), L, N, coo, opts=opts, seed=11, probes=True)


def test_masks(mods):
    """none; a random 30 %; one whole chunk; all masked.  (A caller's mask takes cellector_cell_log_likelihoods to the CSR kernel:
    module docstring.)"""
    L, N = 4 * BLU + 5, 2100
    # (totals up to 8: beyond, the CSR kernel folds the expected term in log space, which expected_bound does not count)
    coo = _plant(_random_coo(21, L, N, 20 * N, totals=[1] * 12 + [2] * 5 + [3, 3, 4, 4, 0, 5, 6, 8]), _edge_loci(L, BLU), N, seed=21)
    alpha, beta = _alpha_beta(L, 21)
    rng = np.random.default_rng(21)
    chunk = np.ones(L, np.uint8)
    chunk[BLU:2 * BLU] = 0
    masks = {"none": None, "random 30 %": (rng.random(L) >= 0.3).astype(np.uint8), "chunk 1": chunk, "all": np.zeros(L, np.uint8)}
    g = _load(mods, L, N, coo)
    _, _, groups, _ = _assert_geometry(mods, g, L, N, coo, ())
    for name, m in masks.items():
        ref = tr.cell_reference(N, *coo, alpha, beta, mask=m)
        _check(f"mask {name}", g.cell_log_likelihoods(alpha, beta, m), ref, _n_partials(groups, L, ()))
        if name == "all":
            assert not ref["ll"].any() and not ref["loci_used"].any()
    g.close()


def _t2_coo(L, N, seed):
    """counts widened: totals 5..8 are a quarter of the entries; block 1 (cells 1024..2047) holds totals 1..4 only, so that all its
    tier-2 slices are empty (SKIP_EMPTY); entries planted either side of every chunk edge of all three geometries"""
    coo = _random_coo(seed, L, N, 14 * N, totals=DEEP)
    edges = _edge_loci(L, BLU) + _edge_loci(L, 338) + _edge_loci(L, 767)
    coo = _plant(coo, edges, N, seed=seed, frac=0.2, totals=(1, 2, 5, 5, 6, 7, 8, 8, 4))
    lo, ce, al, re = coo
    blk1 = (ce >= 1024) & (ce < 2048) & (al + re > 4)
    al[blk1] = np.minimum(al[blk1], 1)
    re[blk1] = 1 - al[blk1]
    tot = al + re
    assert ((tot >= 5) & (tot <= 8)).mean() >= 0.10
    assert not (tot[(ce >= 1024) & (ce < 2048)] > 4).any()
    return [lo, ce, al, re]


@pytest.mark.parametrize("L", [337, 338, 339, 677, 766, 767, 768, 3 * 767 + 2])
@pytest.mark.parametrize("t2_tiles", [8, 6, 0])
def test_tier2_tile_sets(mods, L, t2_tiles):
    """ovf_deep 1 with the second tile set over the totals 5..8 (geo_t2<8>: chunks of 338 loci), 5..6 (geo_t2<6>: 767) or none; L on
    the chunk edges of both; columns of 2 and 4 blocks (the width is shared by both tile kernels of a pass).  2500 cells: three
    blocks, the last ragged, the second without any tier-2 entry."""
    N = 2500
    coo = _t2_coo(L, N, seed=L)
    _sweep(mods, f"tier-2 tiles {t2_tiles} L={L}", L, N, coo, opts=(("ovf_deep", 1), ("t2_tiles", t2_tiles)), sbs=(2, 4), seed=L)


# ---- bit identity ------------------------------------------------------------------------------------------------------------
def _identity_cases():
    N, L, coo = _second_trip_coo()
    yield "second trip", L, N, coo, (("tile_groups", 64),)
    L2, N2 = 3 * 767 + 2, 7 * 1024 + 3
    yield "tier-2 tiles 8", L2, N2, _t2_coo(L2, N2, seed=8), (("ovf_deep", 1), ("t2_tiles", 8))
    yield "shallow ragged", 3 * BLU - 17, 5 * 1024 + 1, _random_coo(77, 3 * BLU - 17, 5 * 1024 + 1, 130_000), ()


def test_bit_identity_of_options_repeats_and_reloads(mods):
    """Claims the code makes (include/cellector_ffi.h) or implies, each against the case's default run, np.array_equal on the doubles:
    tile_sb 2 / 4 / 0; compute_expected 0 against 1 (ll and loci_used); timing 0 / 1 / 2 / 3 (the same kernel through
    hipExtLaunchKernelGGL; 3 times every fourth launch: five calls); overlap 0 / 1 / 2; the same call twice on one ctx (work stealing
    must not show); a fresh ctx against one that held another matrix before."""
    other = _random_coo(1, 900, 3000, 40_000)
    for tag, L, N, coo, opts in _identity_cases():
        alpha, beta = _alpha_beta(L, 31)
        ref = tr.cell_reference(N, *coo, alpha, beta)
        g = _load(mods, L, N, coo, opts)
        _, _, groups, _ = _assert_geometry(mods, g, L, N, coo, opts)
        base = g.cell_log_likelihoods(alpha, beta)
        _check(f"identity base, {tag}", base, ref, _n_partials(groups, L, opts))
        _same(base, g.cell_log_likelihoods(alpha, beta), f"{tag}: second call")
        for sb in (2, 4, 0):
            g.set_option("tile_sb", sb)
            _same(base, g.cell_log_likelihoods(alpha, beta), f"{tag}: tile_sb {sb}")
            g.set_option("compute_expected", 0)
            _same(base, g.cell_log_likelihoods(alpha, beta), f"{tag}: tile_sb {sb} compute_expected 0", cols=(0, 2))
            g.set_option("compute_expected", 1)
        for timing in (1, 2, 3, 0):
            g.set_option("timing", timing)
            for rep in range(5 if timing == 3 else 1):
                _same(base, g.cell_log_likelihoods(alpha, beta), f"{tag}: timing {timing} call {rep}")
        for overlap in (0, 2, 1):
            g.set_option("overlap", overlap)
            _same(base, g.cell_log_likelihoods(alpha, beta), f"{tag}: overlap {overlap}")
        g.close()
        h = mods["Cellector"](0)
        for k, v in opts:
            h.set_option(k, v)
        h.load_coo(900, 3000, *_u32(other), 0, 0)
        h.cell_log_likelihoods(*_alpha_beta(900, 1))
        h.load_coo(L, N, *_u32(coo), 0, 0)
        _same(base, h.cell_log_likelihoods(alpha, beta), f"{tag}: a ctx that held another matrix")
        h.close()


# ---- the EM and posterior passes on three of the geometries ----------------------------------------------------------------
def _em_cases():
    N, L, coo = _second_trip_coo()
    yield "second trip", L, N, _two_populations(coo, N, L, seed=3), (("tile_groups", 64),)
    yield ("row lengths",) + _em_row_lengths() + ((),)
    yield ("tier-2 tiles 8",) + _em_tier2() + ((("ovf_deep", 1), ("t2_tiles", 8)),)
    yield ("masked chunk",) + _em_masked_chunk() + ((),)


def _two_populations(coo, N, L, seed):
    """alt counts redrawn from two populations' genotypes (the shapes keep their loci, cells and totals).  Locus 5 also gets an
    entry of a third of the cells, fixed for opposite alleles in the two populations at depth 60: the -80 filter masks it after the first
    iteration (main.rs:444-447), so the later passes and the posterior phase run the tile kernel over a masked locus."""
    rng = np.random.default_rng(seed)
    lo, ce, al, re = coo
    minority = rng.random(N) < 0.07
    af = rng.choice([0.02, 0.5, 0.98], (2, L), p=[0.5, 0.3, 0.2])
    tot = al + re
    al = rng.binomial(tot, af[minority[ce].astype(np.int64), lo])
    # (every third cell with at least five entries: a depth of 20 N keeps the ORACLE's ln_gamma cancellation at this locus far
    #  below the 1e-9 its normalised values are compared at, also for the cells with few entries)
    cells = np.nonzero((np.bincount(ce, minlength=N) >= 5) & (np.arange(N) % 3 == 0))[0]
    m = minority[cells]
    return [np.concatenate([lo, np.full(len(cells), 5)]), np.concatenate([ce, cells]),
            np.concatenate([al, np.where(m, 0, 60)]), np.concatenate([tot - al, np.where(m, 60, 0)])]


def _em_row_lengths():
    N, L, coo = _row_length_coo()
    return L, N, _two_populations(coo, N, L, seed=6)


def _em_masked_chunk():
    """three chunks, 2500 cells; EVERY locus of chunk 1 is fixed for opposite alleles in the two populations at depth 60 in a
    sixth of the cells, so the -80 filter masks the whole chunk after the first iteration: from then on the tile kernel stages an
    all-zero table for it (and loci_used drops the chunk's entries)"""
    L, N = 3 * BLU, 2500
    lo, ce, al, re = _two_populations(_random_coo(41, L, N, 40 * N, totals=[1] * 12 + [2] * 5 + [3, 3, 4, 4, 5, 7, 0]), N, L, seed=41)
    minority = np.random.default_rng(41).random(N) < 0.07  # (_two_populations' first draw with this seed: the same cells)
    # (locus l in the cells with (cell + l) % 6 == 0: about 106 such entries a cell and a depth of 10 N per locus keep the ORACLE's
    #  ln_gamma cancellation, ~5e-11 an entry there, far inside the 1e-7 its sums are compared at)
    add = [[], [], [], []]
    for l in range(BLU, 2 * BLU):
        cells = np.nonzero((np.arange(N) + l) % 6 == 0)[0]
        m = minority[cells]
        for i, v in enumerate((np.full(len(cells), l), cells, np.where(m, 0, 60), np.where(m, 60, 0))):
            add[i].append(v)
    lo, ce, al, re = (np.concatenate([x] + y) for x, y in zip((lo, ce, al, re), add))
    return L, N, [lo, ce, al, re]


def _em_tier2():
    L, N = 3 * 767 + 2, 2500
    return L, N, _two_populations(_t2_coo(L, N, seed=12), N, L, seed=12)


@pytest.mark.parametrize("case", [0, 1, 2, 3], ids=["second-trip", "row-lengths", "tier2-tiles-8", "masked-chunk"])
def test_em_and_posteriors(mods, case):
    """The whole loop and the posterior phase (three more launches of the tile kernel, the partial sums of the three table sets
    strided by groups x padded cells) with columns of 2 and of 4 blocks, against the oracle at the existing tolerances
    (test_gpu_parity._run_both / _check_posteriors: no cell within 1e-9 of the threshold — a condition these inputs meet, checked
    with the oracle alone).  Against the reference within the tight bound:
      * ll, expected_ll and loci_used of one more iteration at the fixed point — the EM pass (EXPECTED = true) under the mask
        the locus filter left (locus 5 is masked: its table rows are zero and its entries leave loci_used);
      * ll_minority and ll_majority of the posterior phase, which runs over ALL loci (quirk Q1: get_loci_used_for_posterior_calc,
        main.rs:282-306, returns all-true) with alpha / beta from the exclusion set's tallies over all loci, formed as
        posterior_reference.posterior_alpha_betas does (posterior_alpha_betas(0 / 1 / 2) must return those bits);
      * posterior and doublet_posterior of every cell within the relative bound of tests/posterior_reference.py, which is how the
        doublet set's sum — table set 2 of the phase, not returned by the ABI — is seen."""
    import posterior_reference as pr
    import test_gpu_parity as T
    tag, L, N, coo, opts = list(_em_cases())[case]
    post = None
    lo, ce, al, re = coo
    ob = mods["ob"]
    ob.set_threads(ob.host_threads())
    try:
        for sb in (2, 4):
            g = _load(mods, L, N, coo, opts)
            _, _, groups, _ = _assert_geometry(mods, g, L, N, coo, opts)
            G = _n_partials(groups, L, opts)
            g.set_option("tile_sb", sb)
            o = ob.Oracle.from_coo(L, N, *_u32(coo), 0, 0)
            iters = T._run_both(g, o)
            assert iters >= 2 and o.excluded().sum() > 0 and not o.loci_mask()[5]
            # one more iteration at the fixed point: the set does not move and no locus is filtered, so its cell pass ran with
            # alpha_betas() (init_alpha_betas of the set, on every locus) under the mask loci_mask() returns
            sg, so = g.em_iteration(5.0), o.em_iteration(5.0)
            T._check_iteration(g, o, sg, so)
            assert not sg.any_change and sg.n_loci_filtered == 0
            a_em, b_em = g.alpha_betas()
            used = g.loci_mask()
            assert not used[5]
            if tag == "masked chunk":
                assert not used[BLU:2 * BLU].any() and used[:5].all() and used[2 * BLU:].all()
            co = g.cell_outputs()
            ref = tr.cell_reference(N, *coo, a_em, b_em, mask=used)
            worst = _check(f"{tag} tile_sb {sb}: last EM pass", (co["ll"], co["expected_ll"], co["loci_used"]), ref, G)
            pg, _ = T._check_posteriors(dict(mods, engine=2), g, o)
            exc = g.excluded() != 0
            if post is None:  # (the reference of the posterior phase: once per case, the set is the same under both widths)
                post = pr.reference(L, N, coo, exc)
            assert np.array_equal(exc, post["excluded"]) and np.array_equal(g.locus_counts(), post["locus_counts"])
            for which in (0, 1, 2):
                a, b = g.posterior_alpha_betas(which)
                assert np.array_equal(a, post["ab"][which][0]) and np.array_equal(b, post["ab"][which][1]), (tag, which)
            for name, ref in (("ll_minority", post["sums"][0]), ("ll_majority", post["sums"][1])):
                bound = tr.cell_bound(ref, G)[0] + 0.5 * np.spacing(np.abs(ref["ll"]))
                d = np.abs(pg[name] - ref["ll"])
                worst = max(worst, _ratio(d, bound))
                bad = np.nonzero(d > bound)[0]
                assert bad.size == 0, (tag, sb, name, bad[:6], pg[name][bad[:6]], ref["ll"][bad[:6]], bound[bad[:6]])
            # posterior and doublet_posterior by the relative rule of tests/posterior_reference.py: the only outputs the doublet
            # set's sum reaches
            res = pr.compare(post, pg, G)
            assert all(bad.size == 0 for _, bad in res.values()), f"{tag} tile_sb {sb}: " + pr.describe(post, pg, res, G)
            print(f"  {tag} tile_sb {sb}: posterior phase worst / bound " + ", ".join(f"{k} {res[k][0]:.3f}" for k in pr.OUTPUTS))
            print(f"  {tag} tile_sb {sb}: {iters} iterations, {int(exc.sum())} excluded, {int((used == 0).sum())} loci masked; "
                  f"EM pass and posterior sums worst / bound = {worst:.3f}")
            g.close(); o.close()
    finally:
        ob.set_threads(1)
