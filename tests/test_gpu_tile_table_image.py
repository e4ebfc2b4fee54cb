"""GPU: every word of a chunk's table image is where the tile kernel's lookup reads it (k_tile_ll, csrc/kernels_tiled.hip).

The chunk tables are written by one kernel (k_build_tables, k_t2c_tables), copied into LDS by another (the tile kernel's staging:
16-byte units, the last row of them written by part of the workgroup only) and read there by an address function of (slot, code) that the
geometry owns (csrc/tiled.h: tab_pmf / tab_exp; code-major for the regular entries).  A word that lands one plane, one slot or one
unit off moves a single-entry cell by a whole term, so the matrices here give EVERY (locus, code) of three chunks a cell of its
own whose only entry it is: its ll is that table word, its expected_ll the expected-term word of the entry's total.

Bounds: those of tests/test_gpu_tile_sweep.py for a single-entry probe (tile_reference.term_bound / expected_bound alone: adding
zeros is exact); everything else here is bit equality.
"""
import functools

import numpy as np
import pytest

import test_gpu_tile_sweep as S
import tile_reference as tr

pytestmark = pytest.mark.gpu

BLU = S.BLU
CODES = [(1, 0), (0, 1), (2, 0), (1, 1), (0, 2), (3, 0), (2, 1), (1, 2), (0, 3), (4, 0), (3, 1), (2, 2), (1, 3), (0, 4)]
assert [(a, r) for n in range(1, 5) for r in range(n + 1) for a in [n - r]] == CODES  # code = n (n + 1) / 2 - 1 + ref


@pytest.fixture(scope="module")
def mods(oracle_lib, hip_lib_path):
    import torch
    from cellector_amd import Cellector, ffi
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    return dict(Cellector=Cellector, ffi=ffi, ob=oracle_lib, ncu=ncu)


def _sub(d, sel):
    """the per-cell arrays of a cell_reference result, for the cells `sel`"""
    return {k: d[k][sel] for k in ("ll", "expected_ll", "loci_used", "count", "abs_ll", "abs_ell", "b_ll", "b_ell")}


def _singles(L, pairs):
    """one cell per (locus, pair), locus-major, then a second copy of all of them: the copy of cell c is cell c + L * len(pairs)"""
    P = len(pairs)
    lo = np.repeat(np.arange(L), P)
    al = np.tile(np.array([p[0] for p in pairs]), L)
    re = np.tile(np.array([p[1] for p in pairs]), L)
    n1 = L * P
    return n1, [np.concatenate([lo, lo]), np.arange(2 * n1), np.concatenate([al, al]), np.concatenate([re, re])]


@functools.lru_cache(maxsize=None)
def _regular_case():
    """L = 2 * 639 + 1: three chunks, the last with one locus (its image is all zero slot but one).  Cells [0, n1): the singles;
    [n1, 2 n1): their copies (17 906 cells further: other blocks, other lanes); then the two-entry cells of the zero-slot test:
    per chunk, pairs of loci (first, last and random slots; chunk 2: the same locus twice) with random codes, ascending locus."""
    L = 2 * BLU + 1
    n1, coo = _singles(L, CODES)
    rng = np.random.default_rng(7)
    pairs = []  # (locus a, code a, locus b, code b), locus a <= locus b, same chunk
    for j in (0, 1):
        slots = [(0, 638), (0, 1), (637, 638), (31, 32), (319, 320)] + [tuple(sorted(rng.choice(BLU, 2, replace=False))) for _ in range(59)]
        pairs += [(j * BLU + s, int(rng.integers(14)), j * BLU + t, int(rng.integers(14))) for s, t in slots]
    pairs += [(2 * BLU, ca, 2 * BLU, cb) for ca in range(14) for cb in (0, 5, 13) if ca != cb]
    n2 = len(pairs)
    lo2 = np.array([[p[0], p[2]] for p in pairs]).ravel()
    cd2 = np.array([[p[1], p[3]] for p in pairs]).ravel()
    ce2 = np.repeat(2 * n1 + np.arange(n2), 2)
    codes = np.array(CODES)
    coo = [np.concatenate([coo[0], lo2]), np.concatenate([coo[1], ce2]), np.concatenate([coo[2], codes[cd2, 0]]),
           np.concatenate([coo[3], codes[cd2, 1]])]
    N = 2 * n1 + n2
    alpha, beta = S._alpha_beta(L, 71)  # (log-uniform, not whole: all table words distinct)
    return dict(L=L, N=N, n1=n1, coo=coo, pairs=pairs, alpha=alpha, beta=beta, ref=tr.cell_reference(N, *coo, alpha, beta))


def _single_checks(tag, got, ref, n1, expected):
    """the singles against the reference within the single-entry bound; the copies to the bit"""
    sel = np.arange(2 * n1)
    ll, ell, nl = (x[sel] for x in got)
    if not expected:  # (compute_expected 0 leaves expected_ll unspecified)
        ell = np.zeros_like(ll)
    S._check(tag, (ll, ell, nl), _sub(ref, sel), 0, expected=expected, probes=True)
    for i in ((0, 1, 2) if expected else (0, 2)):
        a, b = got[i][:n1], got[i][n1:2 * n1]
        assert np.array_equal(a, b), f"{tag}: output {i} of a cell and of its copy differ at {np.nonzero(a != b)[0][:8]}"


@pytest.mark.parametrize("compute_expected", [1, 0])
@pytest.mark.parametrize("bank_order", [0, 1])
def test_every_table_word_and_the_zero_slot(mods, bank_order, compute_expected):
    """Cases 1 and 2.  Every (locus, code) of three chunks, twice; columns of 2 and 4 blocks agree to the bit.  The two-entry cells
    (K = 3: one padding lookup, which must read 0.0 out of the zero slot of whatever plane its code 0 / n - 1 = 0 selects): ll is
    the rounded sum of the two single-entry cells' values in ascending-locus order — zeros added to it change nothing."""
    c = _regular_case()
    L, N, n1, ref = c["L"], c["N"], c["n1"], c["ref"]
    opts = (("bank_order", bank_order),)
    g = S._load(mods, L, N, c["coo"], opts)
    S._assert_geometry(mods, g, L, N, c["coo"], opts)
    g.set_option("compute_expected", compute_expected)
    runs = {}
    for sb in (2, 4):
        g.set_option("tile_sb", sb)
        got = runs[sb] = g.cell_log_likelihoods(c["alpha"], c["beta"])
        tag = f"table image: bank_order {bank_order} compute_expected {compute_expected} tile_sb {sb}"
        _single_checks(tag, got, ref, n1, bool(compute_expected))
        ll = got[0]
        for k, (la, ca, lb, cb) in enumerate(c["pairs"]):
            want = ll[la * 14 + ca] + ll[lb * 14 + cb]
            assert ll[2 * n1 + k] == want, (tag, "two-entry cell", k, (la, ca, lb, cb), ll[2 * n1 + k], want)
            if compute_expected:
                want = got[1][la * 14 + ca] + got[1][lb * 14 + cb]  # (the expected terms of the two entries' totals)
                assert got[1][2 * n1 + k] == want, (tag, "two-entry cell, expected", k, (la, ca, lb, cb), got[1][2 * n1 + k], want)
        assert np.array_equal(got[2][2 * n1:], np.full(len(c["pairs"]), 2.0))
    S._same(runs[2], runs[4], "table image: tile_sb 2 against 4", cols=(0, 1, 2) if compute_expected else (0, 2))
    g.close()


def test_no_stale_words_across_passes(mods):
    """Case 3.  Two passes on one ctx.  The second alpha / beta differ at the loci of chunk 1 and at the masked loci only; its mask
    drops loci of chunks 0 and 1 (their first and last and every seventh locus): a masked locus' words are all zero, the words of chunks 0 and 2 are the
    first pass' bits, chunk 1's are the new ones."""
    c = _regular_case()
    L, N, n1 = c["L"], c["N"], c["n1"]
    g = S._load(mods, L, N, c["coo"])
    first = g.cell_log_likelihoods(c["alpha"], c["beta"])
    _single_checks("two passes: first", first, c["ref"], n1, True)
    a2, b2 = c["alpha"].copy(), c["beta"].copy()
    an, bn = S._alpha_beta(L, 72)
    a2[BLU:2 * BLU], b2[BLU:2 * BLU] = an[BLU:2 * BLU], bn[BLU:2 * BLU]
    mask = np.ones(L, np.uint8)
    mask[[0, BLU - 1, BLU, 2 * BLU - 1]] = 0
    mask[3::7] = 0
    assert mask[2 * BLU]  # (chunk 2's only locus stays)
    a2[mask == 0], b2[mask == 0] = an[mask == 0], bn[mask == 0]
    second = g.cell_log_likelihoods(a2, b2, mask)
    ref2 = tr.cell_reference(N, *c["coo"], a2, b2, mask=mask)
    lo = c["coo"][0][:2 * n1]  # the singles' loci
    dead = mask[lo] == 0
    for i in (0, 1, 2):
        assert not second[i][:2 * n1][dead].any(), f"output {i}: a cell at a masked locus is not zero"
    same = ~dead & ((lo < BLU) | (lo >= 2 * BLU))
    for i in (0, 1, 2):
        a, b = first[i][:2 * n1][same], second[i][:2 * n1][same]
        assert np.array_equal(a, b), f"output {i}: chunks 0 / 2 moved between the passes at {np.nonzero(a != b)[0][:8]}"
    assert (first[0][:2 * n1][~same & ~dead] != second[0][:2 * n1][~same & ~dead]).all()  # (chunk 1 did change)
    _single_checks("two passes: second", second, ref2, n1, True)
    g.close()


@functools.lru_cache(maxsize=None)
def _tier2_case(t2_tiles):
    blu, hi = S.T2_BLU[t2_tiles], t2_tiles
    L = 2 * blu + 1
    pairs = [(n - r, r) for n in range(5, hi + 1) for r in range(n + 1)]
    assert len(pairs) == {8: 30, 6: 13}[t2_tiles]
    n1, coo = _singles(L, pairs)
    alpha, beta = S._alpha_beta(L, 73 + t2_tiles)
    return dict(L=L, N=2 * n1, n1=n1, coo=coo, alpha=alpha, beta=beta, ref=tr.cell_reference(2 * n1, *coo, alpha, beta))


@pytest.mark.parametrize("compute_expected", [1, 0])
@pytest.mark.parametrize("bank_order", [0, 1])
@pytest.mark.parametrize("t2_tiles", [8, 6])
def test_tier2_table_words(mods, t2_tiles, bank_order, compute_expected):
    """Case 4.  The tier-2 tile sets of a deep matrix: every (locus, (alt, ref)) of totals 5..8 (chunks of 338 loci; the table is
    11 526 doubles: the staging's last row of units ends inside a wave) resp. 5..6 (767 loci), three chunks, the last with one locus."""
    c = _tier2_case(t2_tiles)
    L, N, n1 = c["L"], c["N"], c["n1"]
    opts = (("ovf_deep", 1), ("t2_tiles", t2_tiles), ("bank_order", bank_order))
    g = S._load(mods, L, N, c["coo"], opts)
    info = g.engine_info()
    assert (info.nnz_regular, info.nnz_overflow) == (0, N)
    for v in (0, 6, 8):  # (the tile set that was built: test_gpu_tile_sweep._assert_geometry)
        if v == t2_tiles:
            g.set_option("t2_tiles", v)
        else:
            with pytest.raises(mods["ffi"].CellectorError):
                g.set_option("t2_tiles", v)
    g.set_option("compute_expected", compute_expected)
    runs = {}
    for sb in (2, 4):
        g.set_option("tile_sb", sb)
        runs[sb] = g.cell_log_likelihoods(c["alpha"], c["beta"])
        _single_checks(f"tier-2 table image {t2_tiles}: bank_order {bank_order} compute_expected {compute_expected} tile_sb {sb}",
                       runs[sb], c["ref"], n1, bool(compute_expected))
    S._same(runs[2], runs[4], f"tier-2 table image {t2_tiles}: tile_sb 2 against 4", cols=(0, 1, 2) if compute_expected else (0, 2))
    g.close()
