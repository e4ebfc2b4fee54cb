"""cellector_amd/combine.py, the numpy twin of cellector_combine, against the reference's own definition (no GPU needed):
combine_coo against a plain-Python sorted() of the tuple list (locus, cell, ref, alt) the combiner pushes (combiner/src/main.rs:72-111),
locus_map_from_vcfs against get_locus_mapping (main.rs:197-231) on a hand-written VCF pair."""
import gzip

import numpy as np
import pytest

from cellector_amd import combine, restage


def _random_side(rng, n, tl, nc, repeats):
    locus = rng.integers(0, tl, n).astype(np.uint32)
    cell = rng.integers(0, nc, n).astype(np.uint32)
    if repeats and n > 6:  # repeated (locus, cell) lines with other counts
        locus[n // 2:n // 2 + 3] = locus[0]
        cell[n // 2:n // 2 + 3] = cell[0]
    return [locus, cell, rng.integers(0, 6, n).astype(np.uint32), rng.integers(0, 6, n).astype(np.uint32)]


def _plain(dst, n_dst, src, n_src, keep, lmap, rate, seed):
    """the combiner's loop in plain Python on the thinned counts"""
    s_alt, s_ref = restage.thin_counts(src[2], src[3], rate, seed)  # keyed by the position in src
    keep = np.ones(n_src, bool) if keep is None else np.asarray(keep) != 0
    new_id = {}
    for c in range(n_src):
        if keep[c]:
            new_id[c] = n_dst + len(new_id)
    lines = [(int(l), int(c), int(r), int(a)) for l, c, a, r in zip(*dst)]
    for i in range(len(src[0])):
        c = int(src[1][i])
        if c in new_id:
            l = int(src[0][i])
            lines.append((int(lmap[l]) if lmap is not None else l, new_id[c], int(s_ref[i]), int(s_alt[i])))
    lines.sort()
    return lines, n_dst + len(new_id), sorted(new_id)


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("rate", [0.0, 0.37])
def test_combine_coo_is_the_sorted_tuple_list(seed, rate):
    rng = np.random.default_rng(seed)
    tl_d, tl_s, n_dst, n_src = 17, 23, 9, 11
    dst = _random_side(rng, 150, tl_d, n_dst, True)  # unsorted, with repeated pairs
    assert (np.diff(dst[0].astype(np.int64)) < 0).any()
    src = _random_side(rng, 120, tl_s, n_src, True)
    lmap = rng.permutation(tl_s + 4)[:tl_s].astype(np.uint32)
    lmap[5] = lmap[2]  # two src loci fold into one
    keep = None if seed == 0 else rng.random(n_src) < 0.6
    if keep is not None:
        keep[3] = True
    tlo = max(tl_d, int(lmap.max()) + 1)
    got = combine.combine_coo(dst, n_dst, src, n_src, keep, lmap, tlo, rate, 4)
    lines, total_cells, kept = _plain(dst, n_dst, src, n_src, keep, lmap, rate, 4)
    assert got[4] == total_cells
    assert [tuple(int(x) for x in t) for t in zip(got[0], got[1], got[3], got[2])] == lines
    assert all(a.dtype == np.uint32 for a in got[:4])
    assert np.array_equal(got[5], np.concatenate([np.arange(n_dst), kept]))
    assert np.array_equal(got[6], np.concatenate([np.zeros(n_dst), np.ones(len(kept))]))
    assert got[5].dtype == np.uint32 and got[6].dtype == np.uint8


def test_identity_map_and_composition_arguments():
    rng = np.random.default_rng(9)
    dst, src = _random_side(rng, 40, 8, 5, False), _random_side(rng, 30, 8, 4, False)
    got = combine.combine_coo(dst, 5, src, 4, keep=[1, 0, 1, 1], dst_origin=[7, 8, 9, 10, 11], dst_source=[0, 0, 1, 1, 0],
                              src_origin=[20, 21, 22, 23], k=2)
    lines, total_cells, _ = _plain(dst, 5, src, 4, [1, 0, 1, 1], None, 0.0, 4)
    assert total_cells == 8 and [tuple(int(x) for x in t) for t in zip(got[0], got[1], got[3], got[2])] == lines
    assert got[5].tolist() == [7, 8, 9, 10, 11, 20, 22, 23] and got[6].tolist() == [0, 0, 1, 1, 0, 2, 2, 2]
    with pytest.raises(ValueError):
        combine.combine_coo(dst, 5, src, 4, total_loci_out=3)
    with pytest.raises(ValueError):
        combine.combine_coo(dst, 5, src, 4, keep=[0, 0, 0, 0])


VCF1 = """##fileformat=VCFv4.2
#CHROM\tPOS\tID\tREF\tALT
chr1\t100\t.\tA\tC
chr1\t250\t.\tG\tT
chr2\t100\t.\tA\tG
chr2\t900\t.\tC\tT
"""
VCF2 = """##fileformat=VCFv4.2
##source=hand
#CHROM\tPOS\tID\tREF\tALT
chr1\t50\t.\tA\tC
chr1\t250\t.\tG\tT
chr2\t100\t.\tA\tG
chr2\t500\t.\tT\tG
chr3\t100\t.\tC\tA
chr2\t900\t.\tC\tT
"""


@pytest.mark.parametrize("gz", [False, True])
def test_locus_map_from_vcfs(tmp_path, gz):
    paths = []
    for name, text in (("a.vcf", VCF1), ("b.vcf", VCF2)):
        p = tmp_path / (name + (".gz" if gz else ""))
        (gzip.open(p, "wt") if gz else open(p, "w")).write(text)
        paths.append(str(p))
    lmap, total = combine.locus_map_from_vcfs(*paths)
    # shared positions take vcf1's number (chrom AND pos: chr2:100 is not chr1:100), new ones are appended in vcf2's order
    assert lmap.tolist() == [4, 1, 2, 5, 6, 3] and total == 7 and lmap.dtype == np.uint32
    same, total = combine.locus_map_from_vcfs(paths[0], paths[0])
    assert same.tolist() == [0, 1, 2, 3] and total == 4
