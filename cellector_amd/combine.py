"""Host twin of cellector_combine (csrc/kernels_combine.hip): a second COO merged into a first one, the way the reference's
`combiner` writes two datasets into one (combiner/src/main.rs).

The src side is restage.restage_coo on src's arrays (the selection, the renumbering and the position-keyed draw are
cellector_restage's); its loci then go through the map and its cells behind dst's.  The result ascends by the tuple
(locus, cell, ref, alt) — lines.sort() of main.rs:111 — which is unique, so the numpy result is bit-identical to the device's
whatever order either side came in.
"""
import gzip

import numpy as np

from . import restage

TILE = 2048  # COMBINE_TILE of csrc/kernels_combine.hip: output entries per tile of its merge


def combine_coo(dst_coo, n_dst, src_coo, n_src, keep=None, locus_map=None, total_loci_out=None, rate=0.0, seed=4,
                dst_origin=None, dst_source=None, src_origin=None, k=1):
    """What cellector_combine leaves staged: (locus, cell, alt, ref, total_cells, origin, source).

    dst_coo / src_coo: (locus0, cell0, alt, ref) of the two sides, n_dst / n_src their cell counts.  keep [n_src] (None: all),
    rate and seed act on src only, keyed by the position in src_coo.  locus_map [src total_loci] (None: identity).
    dst_origin / dst_source / src_origin: what cell_origin() / cell_source() of the two ctxs return (None: identity / 0 /
    identity); k: the number of this combine since dst's last ingest from outside."""
    s_locus, s_cell, s_alt, s_ref, n_kept, origin = restage.restage_coo(*src_coo, n_src, keep, rate, seed)
    if locus_map is not None:
        locus_map = np.ascontiguousarray(locus_map, dtype=np.uint32)
        s_locus = locus_map[s_locus]
    total_cells = int(n_dst) + int(n_kept)
    if total_cells > 0xFFFFFFFF:
        raise ValueError(f"{n_dst} + {n_kept} cells exceed 32-bit indices")
    d = [np.ascontiguousarray(a, dtype=np.uint32) for a in dst_coo]
    locus = np.concatenate([d[0], s_locus.astype(np.uint32)])
    cell = np.concatenate([d[1], (s_cell.astype(np.uint64) + np.uint64(n_dst)).astype(np.uint32)])
    alt = np.concatenate([d[2], s_alt])
    ref = np.concatenate([d[3], s_ref])
    if total_loci_out is not None and locus.size and int(locus.max()) >= int(total_loci_out):
        raise ValueError(f"locus {int(locus.max())} is not below total_loci_out {total_loci_out}")
    order = np.lexsort((alt, ref, cell, locus))  # (the last key is the primary one)
    if src_origin is not None:
        origin = np.asarray(src_origin, dtype=np.uint32)[origin]
    own = np.arange(n_dst, dtype=np.uint32) if dst_origin is None else np.asarray(dst_origin, dtype=np.uint32)
    own_source = np.zeros(n_dst, np.uint8) if dst_source is None else np.asarray(dst_source, dtype=np.uint8)
    return (locus[order], cell[order], alt[order], ref[order], total_cells, np.concatenate([own, origin]),
            np.concatenate([own_source, np.full(n_kept, k, np.uint8)]))


def _vcf_records(path, columns=False):
    """(chrom, pos) of every record line, in file order; columns: (chrom, pos, all the line's columns) instead"""
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "rt") as f:
        for line in f:
            if line.startswith("#"):
                continue
            line = line.rstrip("\n")
            if not line:
                continue
            toks = line.split("\t")
            yield (toks[0], int(toks[1]), toks) if columns else (toks[0], int(toks[1]))


def locus_map_from_vcfs(vcf1, vcf2):
    """(locus_map, total_loci_out) of get_locus_mapping (combiner/src/main.rs:197-231), 0-based: record j of vcf2 maps to the
    record of vcf1 at the same (chrom, pos) — the last one, if vcf1 repeats a position — and otherwise to the next number
    behind vcf1's records, in vcf2's order.  Header lines (#) are skipped."""
    seen = {}
    n1 = 0
    for rec in _vcf_records(vcf1):
        seen[rec] = n1
        n1 += 1
    out = []
    nxt = n1
    for rec in _vcf_records(vcf2):
        at = seen.get(rec)
        if at is None:  # (not remembered: a position vcf2 repeats gets a new number each time, as in the reference)
            at = nxt
            nxt += 1
        out.append(at)
    return np.array(out, dtype=np.uint32), nxt
