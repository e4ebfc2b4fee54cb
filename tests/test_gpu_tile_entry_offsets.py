"""GPU: the tile entries' encoding (csrc/tiled.h: tile_entry and its decoders; offset entries for the regular geometry) seen through
the tiled cell pass — every code at every position of a row, and the padding entries behind a short row.

A regular tile entry carries where its two table values sit (the expected term's element, and how many planes behind it the
log-pmf lies) instead of slot, code and total; the builders make it, the bank model and the tile kernel take it apart, all through
the helpers of tiled.h, whose exhaustive compile-time round trip over every (slot, code) is the first half of this check: a
library that was built cannot address outside a chunk's table image.  The second half is here: a lookup that lands one plane or one slot
off moves a cell by a whole term (alpha, beta log-uniform in [1, 1e4]: all table values distinct, |term| ~ 1..9), and every cell is
held to the per-cell bound of tests/test_gpu_tile_sweep.py (~1e-13; module docstring there — nothing of it is fitted to observed
errors), loci_used exactly.

Which half of which dword of a row an entry sits in decides the instructions that decode it (the low half: shift and mask of the
dword as it is; the high half: a shift by 16 more), and a row's length decides the path: both parities of K, the second 16-byte row
load from 9 u16 on, the loop beyond the registers from 17 u16 on.  Hence rows of every length 1..18, and at every position every one
of the 14 codes, with the slots 0 and 638 at both ends of a row.
"""
import numpy as np
import pytest

import test_gpu_tile_sweep as S
import tile_reference as tr

pytestmark = pytest.mark.gpu

BLU = S.BLU
# code = n (n + 1) / 2 - 1 + ref (csrc/tiled.h ent_code): its (alt, ref)
CODES = [(1, 0), (0, 1), (2, 0), (1, 1), (0, 2), (3, 0), (2, 1), (1, 2), (0, 3), (4, 0), (3, 1), (2, 2), (1, 3), (0, 4)]
assert all(a + r and (a + r) * (a + r + 1) // 2 - 1 + r == c for c, (a, r) in enumerate(CODES))


@pytest.fixture(scope="module")
def mods(oracle_lib, hip_lib_path):
    import torch
    from cellector_amd import Cellector, ffi
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    return dict(Cellector=Cellector, ffi=ffi, ob=oracle_lib, ncu=ncu)


def _coo_of(rows):
    """rows: (cell, ascending loci, codes by position) -> COO arrays"""
    lo = np.concatenate([l for _, l, _ in rows])
    ce = np.concatenate([np.full(len(l), c) for c, l, _ in rows])
    code = np.concatenate([k for _, _, k in rows])
    ar = np.array(CODES, dtype=np.int64)[code]
    return [lo.astype(np.int64), ce.astype(np.int64), ar[:, 0], ar[:, 1]]


def _every_code_rows():
    """1024 + 70 cells x 639 + 5 loci: two chunks, a full block and a ragged one.
    Block 0, chunk 0: cell i has 1 + (i // 14) % 18 entries (14 consecutive cells share a length: with the code of position p being
    (p + i) mod 14, every position of every length meets all 14 codes), at ascending loci, so that with bank_order 0 position p
    of the row is the p-th of them; by i % 4 the row starts at slot 0, ends at slot 638, does both, or neither (a row of
    one entry: slot 0, slot 638, slot 0, a random one — the two slots at the first and at the last position of a row).
    Block 0, chunk 1 (5 loci): every third cell, one or two entries.  Block 1 (70 cells): 0..20 entries anywhere."""
    rng = np.random.default_rng(20)
    L, N = BLU + 5, 1024 + 70
    rows = []
    for i in range(1024):
        k, kind = 1 + (i // 14) % 18, i % 4
        if k == 1:
            loci = np.array([[0], [BLU - 1], [0], [int(rng.integers(1, BLU - 1))]][kind])
        else:
            ends = [[0], [BLU - 1], [0, BLU - 1], []][kind]
            loci = np.sort(np.concatenate([ends, 1 + rng.choice(BLU - 2, k - len(ends), replace=False)]).astype(np.int64))
        assert len(loci) == k and (np.diff(loci) > 0).all()
        rows.append((i, loci, (np.arange(k) + i) % 14))
        if i % 3 == 0:
            m = 1 + i % 2
            rows.append((i, BLU + np.sort(rng.choice(5, m, replace=False)), rng.integers(0, 14, m)))
    for i in range(1024, N):
        k = int(rng.integers(0, 21))
        if k:
            rows.append((i, np.sort(rng.choice(L, k, replace=False)), rng.integers(0, 14, k)))
    # what the construction claims: per length 1..18 and position, all 14 codes; the two end slots at both ends of a row
    seen = np.zeros((19, 18, 14), bool)
    first, last = set(), set()
    for c, loci, codes in rows:
        if c < 1024 and loci[0] < BLU:
            seen[len(loci), np.arange(len(loci)), codes] = True
            first.add(int(loci[0])); last.add(int(loci[-1]))
    assert all(seen[k, :k].all() for k in range(1, 19))
    assert {0, BLU - 1} <= first and {0, BLU - 1} <= last
    return L, N, rows


@pytest.fixture(scope="module")
def every_code():
    L, N, rows = _every_code_rows()
    coo = _coo_of(rows)
    alpha, beta = S._alpha_beta(L, 20)
    return dict(L=L, N=N, coo=coo, alpha=alpha, beta=beta, ref=tr.cell_reference(N, *coo, alpha, beta))


def _run_options(mods, tag, case, order, probes=False):
    """one ctx under bank_order `order`: tile_sb 2, 4 and 0, each with compute_expected 1 and 0; every run within the bound, the
    column widths bit-identical to each other, compute_expected 0 bit-identical in ll and loci_used.  Returns the default run."""
    L, N, coo, alpha, beta, ref = (case[k] for k in ("L", "N", "coo", "alpha", "beta", "ref"))
    opts = (("bank_order", order),)
    g = S._load(mods, L, N, coo, opts)
    _, _, groups, _ = S._assert_geometry(mods, g, L, N, coo, opts)
    G = S._n_partials(groups, L, opts)
    runs = {}
    for sb in (2, 4, 0):
        g.set_option("tile_sb", sb)
        runs[sb] = g.cell_log_likelihoods(alpha, beta)
        S._check(f"{tag} bank_order {order} tile_sb {sb}", runs[sb], ref, G, probes=probes)
        g.set_option("compute_expected", 0)
        plain = g.cell_log_likelihoods(alpha, beta)
        g.set_option("compute_expected", 1)
        S._check(f"{tag} bank_order {order} tile_sb {sb} compute_expected 0", plain, ref, G, expected=False, probes=probes)
        S._same(runs[sb], plain, f"{tag} bank_order {order} tile_sb {sb}: compute_expected 0 against 1", cols=(0, 2))
    for sb in (4, 0):
        S._same(runs[2], runs[sb], f"{tag} bank_order {order}: tile_sb 2 against {sb}")
    g.close()
    return runs[0]


@pytest.mark.parametrize("order", [0, 1])
def test_every_code_at_every_position(mods, every_code, order):
    _run_options(mods, "every code", every_code, order)


# ---- padding -----------------------------------------------------------------------------------------------------------------
PAD_K = (3, 4, 8, 9, 17)              # lengths of the rows that share a slice with the single-entry cells
PAD_SLOTS = (0, 31, 320, BLU - 1)     # x 14 codes = 56 single-entry cells a block: they and 8 longer rows make the tile's first slice


def _padding_rows():
    """Block b < 5: cells 0..55 hold ONE entry — (slot, code) over PAD_SLOTS x the 14 codes — and the other 968 hold PAD_K[b]; the
    builder sorts a tile's rows by length and cuts slices of 64, so the 56 short rows sit in a slice of K = PAD_K[b] with K - 1
    padding entries behind their own: in both halves of a dword, behind the second row load (9), on the loop beyond the registers (17).
    Block 5: every cell holds one entry (slices of K = 1: no padding), cell q < 56 the same entry as cell q of the other blocks."""
    rng = np.random.default_rng(23)
    L, N = BLU, 6 * 1024
    single = [(s, c) for s in PAD_SLOTS for c in range(14)]
    rows = []
    for b in range(6):
        for q in range(1024):
            if q < len(single):
                loci, codes = np.array([single[q][0]]), np.array([single[q][1]])
            else:
                k = PAD_K[b] if b < 5 else 1
                loci, codes = np.sort(rng.choice(BLU, k, replace=False)), rng.integers(0, 14, k)
            rows.append((b * 1024 + q, loci, codes))
    return L, N, rows, len(single)


@pytest.fixture(scope="module")
def padding():
    L, N, rows, n_single = _padding_rows()
    coo = _coo_of(rows)
    alpha, beta = S._alpha_beta(L, 23)
    return dict(L=L, N=N, coo=coo, alpha=alpha, beta=beta, ref=tr.cell_reference(N, *coo, alpha, beta), n_single=n_single)


@pytest.mark.parametrize("order", [0, 1])
def test_padding_behind_a_single_entry(mods, padding, order):
    """A padding entry's two lookups read 0.0 (code 0 of the chunk's all-zero slot), and adding 0.0 is exact: a cell whose one
    entry is followed by padding returns the bits of the same entry in a row of its own length."""
    ll, ell, nl = _run_options(mods, "padding", padding, order)
    q = np.arange(padding["n_single"])
    assert (padding["ref"]["count"][q] == 1).all()
    for b, k in enumerate(PAD_K):
        for name, v in (("ll", ll), ("expected_ll", ell), ("loci_used", nl)):
            bad = np.nonzero(v[b * 1024 + q] != v[5 * 1024 + q])[0]
            assert bad.size == 0, (f"bank_order {order}, beside rows of {k}: {name} of single-entry cells {bad[:8]} is "
                                   f"{v[b * 1024 + bad[:8]]}, in a row of one {v[5 * 1024 + bad[:8]]}")
    # and that value is the term itself
    one = padding["ref"]
    assert (np.abs(ll[q] - one["ll"][q]) <= one["b_ll"][q] + 0.5 * np.spacing(np.abs(one["ll"][q]))).all()
    assert (np.abs(ell[q] - one["expected_ll"][q]) <= one["b_ell"][q] + 0.5 * np.spacing(np.abs(one["expected_ll"][q]))).all()
