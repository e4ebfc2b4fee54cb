"""GPU: the two row formats of a tile slice (csrc/tiled.h) — K, a slice's longest row, of either parity — through k_tile_ll.

A slice of the tiled cell-pass layout is 64 x (K + 1) u16 with K = the entries of its longest row, at least 1.  K odd: 64 rows of
[cell id, K entries]; K even: the 64 cell ids first, then 64 rows of K entries.  The tile kernel holds the first 16 u16 of a row in
registers (15 entries behind the cell id, or 16), needs its second 16-byte load beyond 8 u16, and walks longer rows in a loop.

The matrix here: 1024 + 70 cells (a full block and a ragged one) x 2 * 639 + 5 loci (three chunks, the last nearly empty).  In the
full block the row lengths are constructed so that the sixteen slices of the tile of chunk 0 have longest rows 0, 1, ..., 15 and
those of chunk 1 have 2, 3, ..., 17 (a slice holds 24 rows one entry shorter than its longest, so padding occurs too): both
parities, the 7/8/9 edge of the second row load, the 14/15/16/17 edge of the registers against the loop, and an empty slice.
Totals 1..4 with 1.5 % of the entries turned into overflow entries (totals 0, 5, 9), which keep their place in the builder's sort
key (kernels_tiled_build.hip: the row length is the segment's length including them) and get a padding entry in the row.

Checked as tests/test_gpu_tile_sweep.py checks (its helpers, tests/tile_reference.py): every cell within the per-cell bound, loci_used
exactly, bank_order 0 and 1, tile_sb 2, 4 and 0, the widths bit-identical to each other; the same for a tier-2 tile set (ovf_deep 1,
t2_tiles 8 and 6) on a small deep matrix whose tier-2 rows have 0, 1 and 2 entries.

The layout pin: from the COO, in numpy, every tile's sorted row lengths give K of slice s = max(length at rank 64 s + 63, 1);
engine_info().tile_lookups must be 64 * sum K and tile_bytes 2 * (64 * sum (K + 1) + 128 per tile) — 128 (K + 1) bytes per slice in
either format plus the tile's 256-byte header.  Rounding K up to odd again fails both.
"""
import numpy as np
import pytest

import test_gpu_tile_sweep as S

BLU = S.BLU
N_CELLS, N_LOCI = 1024 + 70, 2 * BLU + 5


@pytest.fixture(scope="module")
def mods(oracle_lib, hip_lib_path):
    import torch
    from cellector_amd import Cellector, ffi
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    return dict(Cellector=Cellector, ffi=ffi, ob=oracle_lib, ncu=ncu)


def _slice_lengths(longest):
    """1024 row lengths whose sorted slices of 64 have the given longest rows (ascending): 24 rows one shorter, 40 rows full"""
    out = []
    for k in longest:
        out += [max(k - 1, 0)] * 24 + [k] * 40
    assert len(out) == 1024 and out == sorted(out)
    return np.array(out)


def _parity_coo(seed=17):
    rng = np.random.default_rng(seed)
    lens = np.zeros((N_CELLS, 3), np.int64)
    lens[:1024, 0] = rng.permutation(_slice_lengths(range(0, 16)))
    lens[:1024, 1] = rng.permutation(_slice_lengths(range(2, 18)))
    lens[:1024, 2] = rng.integers(0, 6, 1024)
    lens[1024:, 0] = rng.integers(0, 18, 70)
    lens[1024:, 1] = rng.integers(0, 18, 70)
    lens[1024:, 2] = rng.integers(0, 3, 70)
    width = [BLU, BLU, 5]
    lo, ce = [], []
    for c in range(N_CELLS):
        for j in range(3):
            k = int(lens[c, j])
            if k:
                lo.append(j * BLU + rng.choice(width[j], k, replace=False))
                ce.append(np.full(k, c))
    lo, ce = np.concatenate(lo), np.concatenate(ce)
    tot = rng.choice([1, 1, 1, 2, 2, 3, 4], len(lo))
    ovf = rng.random(len(lo)) < 0.015
    tot[ovf] = rng.choice([0, 5, 9], int(ovf.sum()))
    al = (rng.random(len(lo)) * (tot + 1)).astype(np.int64)
    return [lo, ce, al, tot - al], lens


def _slice_ks(coo, n_cells, n_loci, blu):
    """K of every slice, [block][chunk][16], from the COO: the builder's sort key is a row's number of entries in the chunk"""
    lo, ce = np.asarray(coo[0]), np.asarray(coo[1])
    nb, nj = max(1, -(-n_cells // 1024)), max(1, -(-n_loci // blu))
    lens = np.zeros((nb * 1024, nj), np.int64)
    np.add.at(lens, (ce, lo // blu), 1)
    srt = np.sort(lens.reshape(nb, 1024, nj), axis=1)
    return np.maximum(srt[:, 63::64, :], 1).transpose(0, 2, 1)


def test_constructed_row_lengths():
    """the construction is what the docstring says (no GPU)"""
    coo, lens = _parity_coo()
    ks = _slice_ks(coo, N_CELLS, N_LOCI, BLU)
    assert ks.shape == (2, 3, 16)
    assert list(ks[0, 0]) == [1] + list(range(1, 16))      # longest rows 0..15, the empty slice kept at one padding entry
    assert list(ks[0, 1]) == list(range(2, 18))
    got = np.zeros_like(lens)
    np.add.at(got, (coo[1], coo[0] // BLU), 1)
    assert np.array_equal(got, lens)
    tot = coo[2] + coo[3]
    assert ((tot == 0) | (tot > 4)).sum() > 20 and set(np.unique(tot)) == {0, 1, 2, 3, 4, 5, 9}


@pytest.mark.gpu
def test_layout_pin(mods):
    coo, _ = _parity_coo()
    ks = _slice_ks(coo, N_CELLS, N_LOCI, BLU)
    n_tiles = ks.shape[0] * ks.shape[1]
    for order in (1, 0):
        g = S._load(mods, N_LOCI, N_CELLS, coo, (("bank_order", order),))
        info = g.engine_info()
        print(f"  bank_order {order}: tile_lookups {info.tile_lookups} (64 sum K = {64 * int(ks.sum())}), tile_bytes {info.tile_bytes} "
              f"(layout: {2 * (64 * int((ks + 1).sum()) + 128 * n_tiles)}); K rounded up to odd would give {64 * int((ks | 1).sum())} lookups")
        assert (info.cell_blocks, info.locus_chunks) == ks.shape[:2]
        assert info.tile_lookups == 64 * int(ks.sum())
        assert info.tile_bytes == 2 * (64 * int((ks + 1).sum()) + 128 * n_tiles)
        g.close()


@pytest.mark.gpu
def test_both_row_formats(mods):
    coo, _ = _parity_coo()
    S._sweep(mods, "row parity", N_LOCI, N_CELLS, coo, sbs=(2, 4, 0), orders=(1, 0), seed=17)


@pytest.mark.gpu
@pytest.mark.parametrize("t2_tiles", [8, 6])
def test_tier2_row_formats(mods, t2_tiles):
    """A small deep matrix: the tier-2 rows (totals 5..8 or 5..6 per chunk of 338 or 767 loci) have 0, 1, 2 and a few more entries;
    block 1 has none (every slice empty: skipped by the header's flag)."""
    N, L = N_CELLS, 2 * 338 + 3
    coo = S._t2_coo(L, N, seed=29)
    tot = np.asarray(coo[2]) + np.asarray(coo[3])
    take = (tot >= 5) & (tot <= t2_tiles)
    ks = _slice_ks([np.asarray(coo[0])[take], np.asarray(coo[1])[take]], N, L, S.T2_BLU[t2_tiles])
    longest = set(ks[0].ravel().tolist())
    print(f"  tier-2 tiles {t2_tiles}: K of block 0's slices {sorted(longest)}")
    assert {1, 2} <= longest and (ks[1] == 1).all()
    S._sweep(mods, f"row parity, tier-2 tiles {t2_tiles}", L, N, coo, opts=(("ovf_deep", 1), ("t2_tiles", t2_tiles)), sbs=(2, 4, 0),
             orders=(1, 0), seed=29)
