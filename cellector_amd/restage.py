"""Host twin of cellector_restage (csrc/kernels_restage.hip): a cell subset, renumbered, and per-read downsampling of a COO.

All-integer like synth.py, so the numpy result is bit-identical to the device's.  The draw, for the entry at position i of the
arrays passed in, allele a (0 = ref, 1 = alt) and read r = 0..count-1:

    x = mix64(mix64((seed * GOLD) ^ ((i + 1) * GOLD)) + (2 r + a + 1) * GOLD);   removed iff (x >> 11) < T
    T = int(downsample_rate * 2**53)

It is keyed by the position BEFORE the cell selection, so it does not depend on `keep`.
"""
import numpy as np

from .synth import GOLD, mix64

TILE = 4096  # RESTAGE_TILE of csrc/kernels_restage.hip: entries per tile of its count and write passes


def threshold(downsample_rate):
    """T of the draw: a read is removed iff its 53-bit draw is below it"""
    r = float(downsample_rate)
    if not 0.0 <= r <= 1.0:  # (NaN fails both comparisons)
        raise ValueError(f"downsample_rate {downsample_rate} is not in [0, 1]")
    return int(r * 9007199254740992.0)


def thin_counts(alt, ref, downsample_rate, seed=4):
    """(alt, ref) after the draw; entry i of the arrays is position i of the stream"""
    alt = np.ascontiguousarray(alt, dtype=np.uint32)
    ref = np.ascontiguousarray(ref, dtype=np.uint32)
    t = threshold(downsample_rate)
    if t == 0 or alt.size == 0:
        return alt.copy(), ref.copy()
    t = np.uint64(t)
    with np.errstate(over="ignore"):
        pos = np.arange(1, alt.size + 1, dtype=np.uint64)
        h = mix64((np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) * GOLD) ^ (pos * GOLD))
        out = []
        for allele, counts in ((1, alt), (0, ref)):
            kept = np.zeros(counts.size, np.uint32)
            live = np.nonzero(counts)[0]
            r = 0
            while live.size:
                x = mix64(h[live] + np.uint64(2 * r + allele + 1) * GOLD)
                kept[live] += ((x >> np.uint64(11)) >= t).astype(np.uint32)
                r += 1
                live = live[counts[live] > r]
            out.append(kept)
    return out[0], out[1]


def restage_coo(locus0, cell0, alt, ref, total_cells, keep=None, downsample_rate=0.0, seed=4):
    """What cellector_restage leaves staged: (locus0, cell0, alt, ref, n_cells, origin).  Kept cells are renumbered in ascending
    order of their old index, the surviving entries keep their order, an entry whose two counts reach 0 stays; origin[j] = the
    old index of new cell j."""
    locus0 = np.ascontiguousarray(locus0, dtype=np.uint32)
    cell0 = np.ascontiguousarray(cell0, dtype=np.uint32)
    alt, ref = thin_counts(alt, ref, downsample_rate, seed)
    if keep is None:
        return locus0.copy(), cell0.copy(), alt, ref, int(total_cells), np.arange(total_cells, dtype=np.uint32)
    keep = np.asarray(keep) != 0
    if keep.shape != (total_cells,):
        raise ValueError(f"{total_cells} keep flags expected, got shape {keep.shape}")
    if not keep.any():
        raise ValueError("the selection keeps no cell")
    origin = np.nonzero(keep)[0].astype(np.uint32)
    rank = np.cumsum(keep, dtype=np.int64) - 1  # exclusive scan at the kept cells
    sel = keep[cell0]
    return locus0[sel], rank[cell0[sel]].astype(np.uint32), alt[sel], ref[sel], int(origin.size), origin
