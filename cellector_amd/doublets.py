"""Host twin of cellector_add_doublets (csrc/kernels_doublets.hip): synthetic doublets made of cells of a COO.

For j = 0..n_pairs-1 a cell n_cells + j joins the matrix; at every locus at which cell_a[j] or cell_b[j] has an entry it holds
one entry with the sums of the two parents' (thinned) counts over ALL their entries at that locus.  All-integer like restage.py,
so the numpy result is bit-identical to the device's.  The draw, for the parent entry at position i of the arrays passed in,
pair j, side s (0 = cell_a, 1 = cell_b), allele a (0 = ref, 1 = alt) and read r = 0..count-1:

    h = mix64(mix64((seed * GOLD) ^ ((i + 1) * GOLD)) ^ ((2 j + s + 1) * GOLD))
    x = mix64(h + (2 r + a + 1) * GOLD);   removed iff (x >> 11) < T,   T = int(downsample_rate * 2**53)

The inner hash is restage's entry hash: the draw is independent per (pair, side) and does not depend on which other pairs exist.
Everything then ascends by (locus, cell, ref, alt), as after combine.combine_coo.
"""
import numpy as np

from . import restage
from .synth import GOLD, mix64

TILE = 2048  # DOUBLETS_TILE of csrc/kernels_doublets.hip: staged entries per tile of its count and emit passes
BLOCK = 256  # DB_BLOCK: records one round of a block's emit loop places
MAX_COUNT = 65535  # CELLECTOR_MAX_COUNT


def _thin(h, counts, allele, t):
    """reads of counts[] that survive the draw under the record hashes h[]"""
    kept = np.zeros(counts.size, np.uint32)
    live = np.nonzero(counts)[0]
    r = 0
    with np.errstate(over="ignore"):
        while live.size:
            x = mix64(h[live] + np.uint64(2 * r + allele + 1) * GOLD)
            kept[live] += ((x >> np.uint64(11)) >= t).astype(np.uint32)
            r += 1
            live = live[counts[live] > r]
    return kept


def pair_lists(cell_a, cell_b, n_cells):
    """the two lists as uint32 arrays, refused where cellector_add_doublets refuses them"""
    out = []
    for name, v in (("cell_a", cell_a), ("cell_b", cell_b)):
        if v is None:
            raise ValueError(f"{name} is None")
        v = np.asarray(v)
        if v.ndim != 1 or (v.size and v.dtype.kind not in "iu"):
            raise ValueError(f"{name} is not a list of cell indices")
        out.append(v.astype(np.int64) if v.dtype != np.uint64 else v)
    a, b = out
    if a.size != b.size:
        raise ValueError(f"{a.size} cells a, {b.size} cells b")
    if a.size == 0:
        raise ValueError("no pairs")
    if int(n_cells) + a.size > 0xFFFFFFFF:
        raise ValueError(f"{n_cells} + {a.size} cells exceed 32-bit indices")
    bad = np.nonzero((a < 0) | (a >= n_cells) | (b < 0) | (b >= n_cells))[0]
    same = np.nonzero(a == b)[0]
    first_bad = int(bad[0]) if bad.size else a.size
    first_same = int(same[0]) if same.size else a.size
    if first_bad < a.size and first_bad <= first_same:
        raise ValueError(f"pair {first_bad} ({int(a[first_bad])}, {int(b[first_bad])}) names a cell that is not below total_cells {n_cells}")
    if first_same < a.size:
        raise ValueError(f"pair {first_same} names cell {int(a[first_same])} twice")
    return a.astype(np.uint32), b.astype(np.uint32)


def doublet_side(coo, n_cells, cell_a, cell_b, rate=0.0, seed=4):
    """(locus, cell, alt, ref) of the new cells alone, strictly ascending by (locus, cell); the lists as pair_lists returns them.
    Raises ValueError for a sum above 65535: the first such entry in that order, ref before alt inside it."""
    locus, cell, alt, ref = [np.ascontiguousarray(a, dtype=np.uint32) for a in coo]
    t = np.uint64(restage.threshold(rate))
    # the entries of every cell: positions in ascending order behind row_ptr
    order = np.argsort(cell, kind="stable")
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(cell, minlength=n_cells), dtype=np.int64)])
    ent, pair, side = [], [], []
    for s, parents in enumerate((cell_a, cell_b)):
        cnt = row_ptr[parents.astype(np.int64) + 1] - row_ptr[parents]
        tot = int(cnt.sum())
        start = np.repeat(row_ptr[parents], cnt)
        within = np.arange(tot, dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        ent.append(order[start + within])
        pair.append(np.repeat(np.arange(parents.size, dtype=np.int64), cnt))
        side.append(np.full(tot, s, np.int64))
    ent, pair, side = np.concatenate(ent), np.concatenate(pair), np.concatenate(side)
    r_alt, r_ref = alt[ent], ref[ent]
    if int(t) and ent.size:
        with np.errstate(over="ignore"):
            inner = mix64((np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) * GOLD) ^ ((ent.astype(np.uint64) + np.uint64(1)) * GOLD))
            h = mix64(inner ^ ((2 * pair + side + 1).astype(np.uint64) * GOLD))
        r_ref = _thin(h, r_ref, 0, t)
        r_alt = _thin(h, r_alt, 1, t)
    key = locus[ent].astype(np.uint64) << np.uint64(32) | (pair + int(n_cells)).astype(np.uint64)
    uniq, inv = np.unique(key, return_inverse=True)
    s_alt = np.zeros(uniq.size, np.uint64)
    s_ref = np.zeros(uniq.size, np.uint64)
    np.add.at(s_alt, inv, r_alt.astype(np.uint64))
    np.add.at(s_ref, inv, r_ref.astype(np.uint64))
    over = np.nonzero((s_ref > MAX_COUNT) | (s_alt > MAX_COUNT))[0]
    if over.size:
        d = int(over[0])
        j = int(uniq[d] & np.uint64(0xFFFFFFFF)) - int(n_cells)
        allele = "ref" if int(s_ref[d]) > MAX_COUNT else "alt"
        raise ValueError(f"pair {j} ({int(cell_a[j])}, {int(cell_b[j])}): the summed {allele} count at locus "
                         f"{int(uniq[d] >> np.uint64(32))} exceeds {MAX_COUNT}")
    return ((uniq >> np.uint64(32)).astype(np.uint32), (uniq & np.uint64(0xFFFFFFFF)).astype(np.uint32), s_alt.astype(np.uint32),
            s_ref.astype(np.uint32))


def add_doublets_coo(coo, n_cells, cell_a, cell_b, rate=0.0, seed=4, origin=None, source=None, k=1):
    """What cellector_add_doublets leaves staged: (locus, cell, alt, ref, total_cells, origin, source).

    coo: (locus0, cell0, alt, ref) as staged_coo() returns them, n_cells its cell count.  origin / source: what cell_origin() /
    cell_source() return before the call (None: identity / 0); k: the number this call gets as a combine, n_combines + 1.
    Raises ValueError where the device call returns CELLECTOR_EINVAL."""
    n_cells = int(n_cells)
    restage.threshold(rate)  # (raises for a rate outside [0, 1] or NaN)
    if not 1 <= int(k) <= 255:
        raise ValueError("255 combines since the last ingest from outside (cell_source is a byte)")
    a, b = pair_lists(cell_a, cell_b, n_cells)
    d = [np.ascontiguousarray(x, dtype=np.uint32) for x in coo]
    n_locus, n_cell, n_alt, n_ref = doublet_side(d, n_cells, a, b, rate, seed)
    locus = np.concatenate([d[0], n_locus])
    cell = np.concatenate([d[1], n_cell])
    alt = np.concatenate([d[2], n_alt])
    ref = np.concatenate([d[3], n_ref])
    order = np.lexsort((alt, ref, cell, locus))  # (the last key is the primary one)
    own = np.arange(n_cells, dtype=np.uint32) if origin is None else np.asarray(origin, dtype=np.uint32)
    own_source = np.zeros(n_cells, np.uint8) if source is None else np.asarray(source, dtype=np.uint8)
    return (locus[order], cell[order], alt[order], ref[order], n_cells + a.size, np.concatenate([own, own[a]]),
            np.concatenate([own_source, np.full(a.size, k, np.uint8)]))
