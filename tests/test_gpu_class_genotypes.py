"""GPU: cellector_class_genotypes (csrc/kernels_genotypes.hip + csrc/genotype_host.h) against the numpy twin
cellector_amd/genotypes.py on the ctx's own staged_coo(), the class tallies, the two-class final tallies and the oracle's genotype
call.  Every claim is exact: integers with ==, gt / gp / gp3 with == (NaN equal to NaN; the rule runs on the host in the library,
on the same C library the twin calls).  Every matrix has at most about 1e5 entries.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 16)


@pytest.fixture(scope="module")
def mods(oracle_lib, hip_lib_path):
    from cellector_amd import Cellector, ffi, genotypes, synth
    return dict(Cellector=Cellector, ffi=ffi, gn=genotypes, synth=synth, ob=oracle_lib)


def _u32(coo):
    return [np.ascontiguousarray(x, np.uint32) for x in coo]


def _load(mods, TL, N, coo, min_alt=0, min_ref=0):
    g = mods["Cellector"](0)
    g.load_coo(TL, N, *_u32(coo), min_alt, min_ref)
    return g


def _labels(N, K, seed):
    """a draw over the K classes with 255s; for K >= 2 the last class has no cell"""
    rng = np.random.default_rng(1000 * K + seed)
    lab = rng.integers(0, max(K - 1, 1), N).astype(np.uint8)
    lab[rng.random(N) < 0.15] = 255
    lab[0] = 0
    return lab


def _same(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y, equal_nan=x.dtype.kind == "f")


def _check(mods, g, TL, N, seed=0, ks=KS, genotypes=True):
    """class_genotypes == the twin on the ctx's staged entries, for every K; returns {K: the library's dict}"""
    gn = mods["gn"]
    coo = g.staged_coo()
    out = {}
    for K in ks:
        lab = _labels(N, K, seed)
        got = g.class_genotypes(lab, K, genotypes=genotypes)
        cells, alt, ref = gn.class_genotype_tallies(TL, coo, lab, K)
        assert _same(got["cells"], cells) and _same(got["alt"], alt) and _same(got["ref"], ref), K
        if K >= 2:
            assert not got["alt"][K - 1].any() and not got["ref"][K - 1].any() and got["cells"][K - 1] == 0
        if genotypes:
            gt, gp, gp3 = gn.genotype_posteriors(alt, ref)
            assert _same(got["gt"], gt) and _same(got["gp"], gp) and _same(got["gp3"], gp3), K
            if K >= 2:
                assert (got["gp"][K - 1] == 1.0 / 3.0).all() and not got["gt"][K - 1].any()
        else:
            assert set(got) == {"cells", "alt", "ref"}
        out[K] = got
    return out


def _random_coo(n, TL, N, seed, max_count=6):
    rng = np.random.default_rng(seed)
    lo = np.sort(rng.integers(0, TL, n))
    return lo, rng.integers(0, N, n), rng.integers(0, max_count, n), rng.integers(0, max_count, n)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 5000])
def test_entry_counts_and_any_order(mods, n):
    """locus-major entries (repeated pairs and alt = ref = 0 lines among them), then the same entries in a random permutation
    through ingest_coo: identical integers"""
    TL, N = 37, 50
    coo = _random_coo(n, TL, N, seed=n)
    g = _load(mods, TL, N, coo)
    a = _check(mods, g, TL, N, genotypes=n in (65, 5000))
    g.close()
    perm = np.random.default_rng(n + 1).permutation(n)
    g = _load(mods, TL, N, [x[perm] for x in coo])
    b = _check(mods, g, TL, N, genotypes=False)
    g.close()
    for K in KS:
        for k in ("cells", "alt", "ref"):
            assert np.array_equal(a[K][k], b[K][k]), (K, k)


def test_locus_runs_against_wave_and_block_edges(mods):
    """runs of one locus that end inside a wave (10, 300), on a wave edge (64) and on a block edge (256, 512)"""
    ends = [10, 64, 200, 256, 300, 512, 513, 700]
    N, TL = 260, len(ends) + 2  # (locus 0 and the last one have no read)
    lo = np.concatenate([np.full(e - b, 1 + i) for i, (b, e) in enumerate(zip([0] + ends[:-1], ends))])
    ce = np.concatenate([np.arange(e - b) for b, e in zip([0] + ends[:-1], ends)])
    rng = np.random.default_rng(3)
    coo = (lo, ce, rng.integers(0, 9, len(lo)), rng.integers(0, 9, len(lo)))
    g = _load(mods, TL, N, coo)
    out = _check(mods, g, TL, N)
    assert not out[3]["alt"][:, 0].any() and not out[3]["alt"][:, -1].any() and out[3]["alt"][:, 1:-1].sum(axis=0).all()
    g.close()


def test_64_distinct_keys_and_two_alternating_keys(mods):
    """wave 0: 64 entries at 64 loci; wave 1: two loci alternating lane by lane; wave 2: one locus, two classes alternating; wave 3:
    64 distinct (locus, slot) keys over 4 loci x 16 classes"""
    N, TL = 64, 80
    i = np.arange(64)
    lo = np.concatenate([i, 70 + i % 2, np.full(64, 75), 76 + i // 16])
    ce = np.concatenate([i, i, i, i])
    coo = (lo, ce, 1 + np.arange(256) % 5, 2 + np.arange(256) % 3)
    g = _load(mods, TL, N, coo)
    gn = mods["gn"]
    for K, lab in ((1, np.zeros(N, np.uint8)), (2, (i % 2).astype(np.uint8)), (16, (i % 16).astype(np.uint8)),
                   (16, np.where(i % 5 == 0, 255, i % 16).astype(np.uint8))):
        got = g.class_genotypes(lab, K)
        cells, alt, ref = gn.class_genotype_tallies(TL, g.staged_coo(), lab, K)
        assert _same(got["cells"], cells) and _same(got["alt"], alt) and _same(got["ref"], ref), K
    g.close()


def test_a_sum_beyond_32_bits_and_zero_entries(mods):
    """one locus with 70 000 cells at alt = ref = 65535 (4.6e9 in all, 4.46e9 > 2^32 in one class), a locus of alt = ref = 0 lines, and a repeated
    (locus, cell) line"""
    n_big, N = 70_000, 70_000
    lo = np.concatenate([np.zeros(n_big, np.int64), np.full(100, 1), [2, 2, 2]])
    ce = np.concatenate([np.arange(n_big), np.arange(100), [5, 5, 6]])
    al = np.concatenate([np.full(n_big, 65535), np.zeros(100, np.int64), [3, 3, 1]])
    re = np.concatenate([np.full(n_big, 65535), np.zeros(100, np.int64), [1, 1, 0]])
    g = _load(mods, 3, N, (lo, ce, al, re))
    lab = np.zeros(N, np.uint8)
    lab[::35] = 1  # (68 000 cells stay in class 0: 4.46e9)
    lab[5] = 0
    got = g.class_genotypes(lab, 2)
    n1 = int((lab == 1).sum())
    assert got["alt"][:, 0].tolist() == [65535 * (N - n1), 65535 * n1, 0] and got["alt"][0, 0] > 2 ** 32
    assert np.array_equal(got["alt"][:, 0], got["ref"][:, 0]) and not got["alt"][:, 1].any() and not got["ref"][:, 1].any()
    assert got["alt"][:, 2].tolist() == [7, 0, 0] and got["ref"][:, 2].tolist() == [2, 0, 0]  # (the repeated line counts twice)
    cells, alt, ref = mods["gn"].class_genotype_tallies(3, g.staged_coo(), lab, 2)
    assert _same(got["alt"], alt) and _same(got["ref"], ref) and _same(got["cells"], cells)
    # the deep locus is the reference's quirk or a call, whatever the header says: the twin decides
    gt, gp, gp3 = mods["gn"].genotype_posteriors(alt, ref)
    assert _same(got["gt"], gt) and _same(got["gp"], gp) and _same(got["gp3"], gp3)
    g.close()


@pytest.fixture(scope="module")
def mixture(mods):
    """1500 loci x 700 cells, about 1e5 entries, loaded with min_alt = min_ref = 4 and run to the end of its EM loop"""
    TL, N = 1500, 700
    coo = mods["synth"].generate_coo(TL, N, 0.10, seed=4, minority_fraction=0.08)
    g = _load(mods, TL, N, coo, 4, 4)
    g.run(5.0, 40)
    yield dict(g=g, TL=TL, N=N, coo=coo)
    g.close()


def test_cross_checks_on_a_filtered_matrix(mods, mixture):
    g, TL, N = mixture["g"], mixture["TL"], mixture["N"]
    d = g.dims()
    ids = g.locus_ids().astype(np.int64)
    assert d.total_loci == TL and 0 < d.loci_used < TL
    failed = np.setdiff1d(np.arange(TL), ids)
    fin = g.final_allele_tallies()
    tot_a, tot_r = fin["alt_min"] + fin["alt_maj"], fin["ref_min"] + fin["ref_maj"]
    assert (tot_a[failed] + tot_r[failed]).any()
    out = _check(mods, g, TL, N, seed=7)
    for K in KS:
        lab = _labels(N, K, 7)
        got = out[K]
        # the loci that failed the filter carry their reads
        assert (got["alt"][:, failed].sum(axis=0) == tot_a[failed]).all() and got["alt"][:, failed].any()
        # at the used loci: cellector_class_tallies
        cells, alt, ref = g.class_tallies(lab, K)
        assert np.array_equal(got["alt"][:K][:, ids], alt) and np.array_equal(got["ref"][:K][:, ids], ref)
        assert np.array_equal(got["cells"][:K], cells)
        # the K + 1 slots add up to the locus totals
        assert np.array_equal(got["alt"].sum(axis=0), tot_a) and np.array_equal(got["ref"].sum(axis=0), tot_r)
    # K = 2 by the exclusion set: load_mtx_final and the two sample columns of cellector.vcf
    excl = g.excluded()
    assert 0 < excl.sum() < N
    got = g.class_genotypes(excl == 0, 2)
    assert np.array_equal(got["alt"][0], fin["alt_min"]) and np.array_equal(got["ref"][0], fin["ref_min"])
    assert np.array_equal(got["alt"][1], fin["alt_maj"]) and np.array_equal(got["ref"][1], fin["ref_maj"])
    assert not got["alt"][2].any() and got["cells"].tolist() == [int(excl.sum()), int(N - excl.sum()), 0]
    for t in range(TL):
        gmaj, pmaj, gmin, pmin = mods["ob"].vcf_genotype(fin["alt_min"][t], fin["ref_min"][t], fin["alt_maj"][t], fin["ref_maj"][t])
        assert (got["gt"][0, t], got["gt"][1, t]) == (gmin, gmaj), t
        assert got["gp"][0, t] == pmin or (pmin != pmin and got["gp"][0, t] != got["gp"][0, t]), t
        assert got["gp"][1, t] == pmaj or (pmaj != pmaj and got["gp"][1, t] != got["gp"][1, t]), t
    assert set(np.unique(got["gt"]).tolist()) >= {0, 3}
    # other settings reach the rule
    g5 = g.class_genotypes(excl == 0, 2, ambient=0.0, gt_threshold=0.5)
    gt, gp, gp3 = mods["gn"].genotype_posteriors(got["alt"], got["ref"], 0.0, 0.5)
    assert _same(g5["gt"], gt) and _same(g5["gp"], gp) and _same(g5["gp3"], gp3) and not _same(g5["gt"], got["gt"])


def test_after_combine_and_add_doublets(mods):
    TL, N = 300, 120
    a = _load(mods, TL, N, mods["synth"].generate_coo(TL, N, 0.15, seed=4), 4, 4)
    b = _load(mods, TL, 40, mods["synth"].generate_coo(TL, 40, 0.15, seed=9), 4, 4)
    a.combine(b)
    a.add_doublets(np.arange(10), 120 + np.arange(10))
    a.ingest_finish(4, 4)
    src = a.cell_source()
    assert a.dims().total_cells == 170 and np.bincount(src).tolist() == [120, 40, 10]
    got = a.class_genotypes(src, 3)
    cells, alt, ref = mods["gn"].class_genotype_tallies(TL, a.staged_coo(), src, 3)
    assert _same(got["cells"], cells) and _same(got["alt"], alt) and _same(got["ref"], ref) and alt[2].any()
    # the doublets held out, as a caller of the doublet refine passes them
    held = np.where(src == 2, 255, src).astype(np.uint8)
    got = a.class_genotypes(held, 2)
    assert np.array_equal(got["alt"][2], alt[2]) and np.array_equal(got["alt"][:2], alt[:2]) and got["cells"].tolist() == [120, 40, 10]
    a.close(); b.close()


def test_the_loop_continues_with_the_same_bits(mods, mixture):
    TL, N, coo = mixture["TL"], mixture["N"], mixture["coo"]
    x, y = _load(mods, TL, N, coo, 4, 4), _load(mods, TL, N, coo, 4, 4)
    want = x.run(5.0, 40)
    assert len(want) >= 2 and not want[-1].any_change
    want.append(x.em_iteration(5.0))  # (one more at the fixed point: an iteration follows the interruption)
    got = []
    for it in range(len(want)):
        got.append(y.em_iteration(5.0))
        if it == 1:
            state = (y.excluded(), y.loci_mask())
            y.class_genotypes(_labels(N, 3, 1), 3)
            y.class_genotypes(_labels(N, 16, 1), 16, genotypes=False)
            assert np.array_equal(y.excluded(), state[0]) and np.array_equal(y.loci_mask(), state[1])
    assert [bytes(s) for s in got] == [bytes(s) for s in want]
    assert np.array_equal(x.excluded(), y.excluded()) and np.array_equal(x.loci_mask(), y.loci_mask())
    for k, v in x.cell_outputs().items():
        assert v.tobytes() == y.cell_outputs()[k].tobytes(), k
    x.close(); y.close()


def test_refusals(mods):
    ffi = mods["ffi"]
    TL, N = 37, 50
    coo = _random_coo(300, TL, N, seed=2)
    lab = (np.arange(N) % 3).astype(np.uint8)

    def refused(fn, match):
        with pytest.raises(ffi.CellectorError, match=match) as e:
            fn()
        assert e.value.status == 1

    g = _load(mods, TL, N, coo)
    for K in (0, 17):
        refused(lambda: g.class_genotypes(np.zeros(N, np.uint8), K), "1..16 are supported")
    bad = lab.copy()
    bad[5] = 3
    refused(lambda: g.class_genotypes(bad, 3), "cell 5 has label 3")
    refused(lambda: g.class_genotypes(np.full(N, 255, np.uint8), 3), "every cell is unlabelled")
    for v in (1.5, -0.1, np.nan):
        refused(lambda: g.class_genotypes(lab, 3, ambient=v), "ambient")
        refused(lambda: g.class_genotypes(lab, 3, gt_threshold=v), "gt_threshold")
    lib = ffi.load_library()
    assert lib.cellector_class_genotypes(g.h, None, 3, 0.03, 0.99, *([None] * 6)) == 1 and b"null labels" in lib.cellector_last_error(g.h)
    g.em_begin()
    refused(lambda: g.class_genotypes(lab, 3), "in flight")
    g.em_threshold(5.0)
    g.em_finish()
    # usable afterwards, every output optional
    assert lib.cellector_class_genotypes(g.h, lab.ctypes.data, 3, 0.03, 0.99, *([None] * 6)) == 0
    assert g.class_genotypes(lab, 3, ambient=1.0, gt_threshold=0.0)["cells"].tolist() == [17, 17, 16, 0]
    g.close()
    g = mods["Cellector"](0)
    refused(lambda: g.class_genotypes(lab, 3), "no matrix loaded")
    g.close()
    g = mods["Cellector"](0)
    g.set_option("keep_coo", 0)
    g.load_coo(TL, N, *_u32(coo), 0, 0)
    refused(lambda: g.class_genotypes(lab, 3), r"final tallies need the staged COO \(option keep_coo=1\)")
    g.close()
    m = mods["Cellector"](devices=[0, 0, 0])
    m.load_coo(TL, N, *_u32(coo), 0, 0)
    refused(lambda: m.class_genotypes(lab, 3), "single-device")
    m.close()
    g = mods["Cellector"](0)
    g.set_shard(10, 40)
    g.load_coo(TL, N, *_u32(coo), 0, 0)
    refused(lambda: g.class_genotypes(lab[:30], 3), "set_shard")
    g.close()
