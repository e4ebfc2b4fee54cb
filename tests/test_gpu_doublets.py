"""GPU: cellector_add_doublets — synthetic doublets from resident cells, made on the device.

1. The kernel against its numpy twin (cellector_amd/doublets.py): staged_coo(), dims(), cell_origin() and cell_source() are equal
   exactly, at rates 0, 0.5 and 1 on both engines, on ctxs whose staged entry counts lie around the tile of the count and emit
   passes (doublets.TILE), with emitted-record counts around the block (doublets.BLOCK), with more doublet entries at one locus
   than a merge tile (combine.TILE) holds, with one pair, a hub cell in 130 pairs that carries a count of 65535, every kind of
   parent overlap, and a ctx staged from input that is not locus-major (before and after the finish).
2. Composition with combine and restage.
3. After the finish the ctx equals a fresh load of the twin's arrays, bit for bit, and is held to the CPU oracle with the bounds of
   tests/test_gpu_combine.py::test_combined_ctx_against_the_oracle.
4. Every refusal, with the ctx unchanged.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POST_ATOL = 1e-6  # tests/test_gpu_combine.py
EINVAL = 1
RATES = (0.0, 0.5, 1.0)


@pytest.fixture(scope="module")
def env(oracle_lib, hip_lib_path):
    from cellector_amd import Cellector, combine, doublets, ffi, restage, synth
    return dict(Cellector=Cellector, ffi=ffi, restage=restage, combine=combine, doublets=doublets, synth=synth, ob=oracle_lib)


def _make(env, engine=2, devices=None, **options):
    g = env["Cellector"](devices=devices) if devices else env["Cellector"](0)
    g.set_option("engine", engine)
    for k, v in options.items():
        g.set_option(k, v)
    return g


def _einval(env, fn, *args, **kw):
    with pytest.raises(env["ffi"].CellectorError) as e:
        fn(*args, **kw)
    assert e.value.status == EINVAL and len(str(e.value)) > len("EINVAL: "), str(e.value)
    return str(e.value)


def _same_arrays(got, want, what=""):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), (what, k)


def _tiles():
    from cellector_amd import combine, doublets
    return doublets.TILE, doublets.BLOCK, combine.TILE


TILE, BLOCK, MERGE_TILE = _tiles()


def _add_and_check(env, g, a, b, rate=0.0, seed=4, k=1):
    """one add_doublets on g: everything equal to the twin on what g held staged"""
    before, d0 = g.staged_coo(), g.dims()
    want = env["doublets"].add_doublets_coo(before, d0.total_cells, a, b, rate, seed, g.cell_origin(), g.cell_source(), k)
    g.add_doublets(a, b, rate, seed)
    _same_arrays(g.staged_coo(), want[:4], "staged_coo")
    d = g.dims()
    assert (d.total_cells, d.total_loci, d.cell_begin, d.cell_end) == (want[4], d0.total_loci, 0, want[4])
    assert np.array_equal(g.cell_origin(), want[5]) and np.array_equal(g.cell_source(), want[6])
    key = want[0].astype(np.uint64) << np.uint64(32) | want[1].astype(np.uint64)
    new = key[want[1] >= d0.total_cells]
    assert (np.diff(new.astype(np.int64)) > 0).all()  # exactly one entry per (locus, new cell)
    return want


def _ascending_coo(n, n_loci, n_cells, seed, top=9):
    """n entries with distinct (locus, cell), ascending"""
    rng = np.random.default_rng(seed)
    key = np.sort(rng.choice(n_loci * n_cells, n, replace=False))
    return [(key // n_cells).astype(np.uint32), (key % n_cells).astype(np.uint32), rng.integers(0, top, n).astype(np.uint32),
            rng.integers(0, top, n).astype(np.uint32)]


def _random_pairs(rng, n_cells, n_pairs):
    a = rng.integers(0, n_cells, n_pairs)
    return a, (a + rng.integers(1, n_cells, n_pairs)) % n_cells


# ---- 1. the kernel against the twin -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", [2, 1], ids=["tiled", "csr"])
@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
def test_kernel_equals_the_twin_around_the_tile(env, engine, n):
    n_loci, n_cells = 40, 300
    coo = _ascending_coo(n, n_loci, n_cells, n)
    a, b = _random_pairs(np.random.default_rng(n + 1), n_cells, 70)
    a[-1], b[-1] = coo[1][-1], coo[1][0]  # the last and the first staged entry are parents' entries
    if a[-1] == b[-1]:
        b[-1] = (b[-1] + 1) % n_cells
    g = _make(env, engine)
    for rate in RATES:
        g.ingest_coo(n_loci, n_cells, *coo)
        _add_and_check(env, g, a, b, rate)
    g.close()


@pytest.mark.parametrize("records", [BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK, 2 * BLOCK + 1])
@pytest.mark.parametrize("spread", ["one_entry", "many_entries"])
def test_emitted_records_straddle_the_block(env, records, spread):
    """a round of the emit pass deals its records to the block's threads BLOCK at a time: exactly `records` of them, from one entry
    of a hub cell (one_entry) or from every entry of the round (many_entries); the partners' rows are empty"""
    if spread == "one_entry":
        n_pairs = records
        n_cells = 1 + n_pairs
        coo = [np.array([3], np.uint32), np.zeros(1, np.uint32), np.array([200], np.uint32), np.array([150], np.uint32)]
        a, b = np.zeros(n_pairs, np.int64), 1 + np.arange(n_pairs)
    else:  # ten entries of the hub, ten records per pair it is in; the remainder from cells of one entry, one record a pair
        full, rest = divmod(records, 10)
        n_pairs = full + rest
        n_cells = 1 + 2 * n_pairs  # the hub, the cells 1 .. n_pairs (the first `rest` of them hold an entry), the empty partners
        a = np.concatenate([np.zeros(full, np.int64), 1 + np.arange(rest)])
        b = 1 + n_pairs + np.arange(n_pairs)
        extra = np.arange(rest, dtype=np.uint32)
        coo = [np.concatenate([np.arange(10, dtype=np.uint32), extra % 10]), np.concatenate([np.zeros(10, np.uint32), 1 + extra]),
               np.concatenate([5 + np.arange(10, dtype=np.uint32), extra + 1]), np.concatenate([np.full(10, 7, np.uint32), extra + 2])]
        order = np.lexsort((coo[1], coo[0]))
        coo = [x[order] for x in coo]
    cnt = np.bincount(coo[1], minlength=n_cells)
    assert int(cnt[a].sum() + cnt[b].sum()) == records and len(coo[0]) <= BLOCK  # one round emits them all
    g = _make(env)
    for rate in RATES:
        g.ingest_coo(10, n_cells, *coo)
        _add_and_check(env, g, a, b, rate)
    g.close()


def test_whole_merge_tiles_from_the_doublet_side_alone(env):
    """2100 doublet entries at one locus, behind exactly MERGE_TILE entries of the ctx: output tile 1 holds doublets only"""
    n_par, n_fill = 64, (MERGE_TILE - 64) // 8
    assert n_fill * 8 + n_par == MERGE_TILE
    n_cells = n_fill + n_par
    rng = np.random.default_rng(3)
    locus = np.concatenate([np.repeat(np.arange(8), n_fill), np.full(n_par, 8)]).astype(np.uint32)
    cell = np.concatenate([np.tile(np.arange(n_fill), 8), n_fill + np.arange(n_par)]).astype(np.uint32)
    coo = [locus, cell, rng.integers(0, 9, MERGE_TILE).astype(np.uint32), rng.integers(0, 9, MERGE_TILE).astype(np.uint32)]
    pa, pb = np.divmod(np.arange(2100), 63)
    a, b = n_fill + pa, n_fill + (pa + 1 + pb) % n_par
    g = _make(env)
    for rate in (0.0, 0.5):
        g.ingest_coo(9, n_cells, *coo)
        want = _add_and_check(env, g, a, b, rate)
        assert len(want[0]) == MERGE_TILE + 2100
        assert (want[1][MERGE_TILE:2 * MERGE_TILE] >= n_cells).all() and (want[1][:MERGE_TILE] < n_cells).all()
    g.close()


@pytest.mark.parametrize("engine", [2, 1], ids=["tiled", "csr"])
def test_one_pair(env, engine):
    coo = _ascending_coo(500, 30, 200, 5)
    g = _make(env, engine)
    for rate in RATES:
        g.ingest_coo(30, 200, *coo)
        want = _add_and_check(env, g, [int(coo[1][7])], [int(coo[1][300]) if coo[1][300] != coo[1][7] else int(coo[1][301])], rate)
        assert want[4] == 201
    g.close()


def test_a_hub_cell_in_130_pairs_with_a_count_of_65535(env):
    n_loci, n_cells = 25, 200
    coo = _ascending_coo(1500, n_loci, n_cells, 17)
    hub = int(coo[1][40])
    at = np.flatnonzero(coo[1] == hub)
    assert len(at) >= 2
    coo[2][at[0]] = 65535  # alt of one of the hub's entries ...
    coo[3][at[1]] = 65535  # ... and ref of another
    others = np.array([c for c in range(n_cells) if c != hub][:130])
    a = np.where(np.arange(130) % 3 == 0, others, hub)  # side b in every third pair, side a in the others
    b = np.where(np.arange(130) % 3 == 0, hub, others)
    g = _make(env)
    for rate in (0.5, 1.0):
        g.ingest_coo(n_loci, n_cells, *coo)
        _add_and_check(env, g, a, b, rate, seed=12)
    # at rate 0 a partner with reads at one of those loci makes the sum too large: the twin's refusal, word for word
    g.ingest_coo(n_loci, n_cells, *coo)
    before = g.staged_coo()
    with pytest.raises(ValueError) as e:
        env["doublets"].add_doublets_coo(coo, n_cells, a, b, 0.0, 12)
    assert str(e.value) in _einval(env, g.add_doublets, a, b, 0.0, 12)
    _same_arrays(g.staged_coo(), before)
    g.close()


def test_every_kind_of_parent_overlap(env):
    # cell 0: loci 0, 1, 2.  cell 1: loci 0, 1, 2 (shares every locus with 0).  cell 2: loci 5, 6 (shares none with 0).
    # cell 3: locus 1 three times and locus 6 twice (repeated lines).  cells 4 and 5: empty rows.
    lines = [(0, 0, 3, 4), (0, 1, 1, 0), (1, 0, 0, 0), (1, 1, 9, 9), (1, 3, 2, 5), (1, 3, 7, 1), (1, 3, 2, 5), (2, 0, 8, 2), (2, 1, 6, 6),
             (5, 2, 4, 4), (6, 2, 1, 3), (6, 3, 30, 40), (6, 3, 0, 0)]
    coo = [np.array([x[k] for x in lines], np.uint32) for k in range(4)]
    a = [0, 0, 0, 3, 0, 4, 2, 3]
    b = [2, 1, 3, 2, 4, 5, 3, 0]
    g = _make(env)
    for rate in RATES:
        g.ingest_coo(7, 6, *coo)
        want = _add_and_check(env, g, a, b, rate, seed=3)
        per_cell = np.bincount(want[1], minlength=14)[6:]
        assert per_cell.tolist() == [5, 3, 4, 3, 3, 0, 3, 4]  # loci covered by either parent; two empty parents: an empty row
    assert want[2][want[1] >= 6].sum() == 0 and want[3][want[1] >= 6].sum() == 0  # rate 1: the entries stay, at 0
    g.close()


@pytest.mark.parametrize("n", [257, TILE + 1])
def test_ctx_staged_from_input_that_is_not_locus_major(env, n):
    n_loci, n_cells = 20, 150
    coo = _ascending_coo(n, n_loci, n_cells, n + 2)
    order = np.random.default_rng(n).permutation(n)
    shuffled = [x[order] for x in coo]
    a, b = _random_pairs(np.random.default_rng(n + 3), n_cells, 40)
    g = _make(env)
    for rate in (0.0, 0.5):
        # before the finish: the staged order is the file's, the ctx side goes through the sort
        g.ingest_coo(n_loci, n_cells, *shuffled)
        _same_arrays(g.staged_coo(), shuffled, "file order while STAGED")
        w1 = _add_and_check(env, g, a, b, rate)
        # after the finish: the stable sort by locus of that order; cells inside a locus still do not ascend
        g.ingest_coo(n_loci, n_cells, *shuffled)
        g.ingest_finish(1, 1)
        st = g.staged_coo()
        assert (np.diff(st[0].astype(np.int64)) >= 0).all()
        key = st[0].astype(np.uint64) << np.uint64(32) | st[1].astype(np.uint64)
        assert (np.diff(key.astype(np.int64)) < 0).any()
        w2 = _add_and_check(env, g, a, b, rate)
        # the positions differ, so do the draws: equal at rate 0 only
        same = all(np.array_equal(x, y) for x, y in zip(w1[:4], w2[:4]))
        assert same == (rate == 0.0)
    g.ingest_finish(1, 1)  # the merged COO is locus-major: the finish takes it as it stands
    _same_arrays(g.staged_coo(), w2[:4], "after the finish")
    g.close()


# ---- 2. composition ---------------------------------------------------------------------------------------------------------------
def test_composition_with_combine_and_restage(env):
    n_loci, n_dst, n_src = 60, 200, 90
    dst, src = _ascending_coo(3000, n_loci, n_dst, 31), _ascending_coo(1200, n_loci, n_src, 32)
    g, s = _make(env), _make(env)
    s.ingest_coo(n_loci, n_src, *src)
    g.ingest_coo(n_loci, n_dst, *dst)
    keep = np.arange(n_src) % 3 != 0
    g.combine(s, keep, downsample_rate=0.25)
    mixed = g.staged_coo()
    source, origin = g.cell_source(), g.cell_origin()
    assert set(source.tolist()) == {0, 1}
    rng = np.random.default_rng(6)
    a, b = rng.choice(np.flatnonzero(source == 0), 50), rng.choice(np.flatnonzero(source == 1), 50)
    want = _add_and_check(env, g, a, b, 0.5, k=2)
    assert want[6].tolist() == source.tolist() + [2] * 50 and np.array_equal(want[5][len(source):], origin[a])
    g.ingest_finish()
    g.run(5.0, 30)
    g.restage(keep=g.cell_source() != 2)  # the doublets out again: the mixture as it was staged
    _same_arrays(g.staged_coo(), mixed, "the mixture")
    assert np.array_equal(g.cell_source(), source) and np.array_equal(g.cell_origin(), origin)
    # a second round of doublets is the third combine; a restage composes source and origin
    want = _add_and_check(env, g, b[:5], a[:5], 0.0, k=3)
    assert want[6][-5:].tolist() == [3] * 5 and np.array_equal(want[5][-5:], origin[b[:5]])
    pick = np.arange(want[4]) % 2 == 1
    g.restage(keep=pick)
    assert np.array_equal(g.cell_source(), want[6][pick]) and np.array_equal(g.cell_origin(), want[5][pick])
    _same_arrays(s.staged_coo(), src, "src")
    g.close(); s.close()


# ---- 3. a ctx with doublets, a fresh load of the twin's arrays, the oracle -------------------------------------------------------
L0, N0, NP = 400, 500, 40


@pytest.fixture(scope="module")
def case(env):
    coo = env["synth"].generate_coo(L0, N0, 0.1, seed=11, minority_fraction=0.1)
    cls = env["synth"].cell_classes(N0, seed=11, minority_fraction=0.1)
    rng = np.random.default_rng(4)
    a, b = rng.choice(np.flatnonzero(cls == 0), NP), rng.choice(np.flatnonzero(cls == 1), NP)
    twin = env["doublets"].add_doublets_coo(coo, N0, a, b, 0.5, 4)
    return dict(coo=coo, a=a, b=b, twin=twin)


def _collect(g):
    """everything the equivalence compares, after running to the fixed point (tests/test_gpu_combine.py's)"""
    d = g.dims()
    out = dict(dims=(d.total_cells, d.total_loci, d.loci_used, d.cell_begin, d.cell_end, d.nnz_used), locus_ids=g.locus_ids(),
               locus_counts=g.locus_counts(), entries_per_cell=g.entries_per_cell(), csr=list(g.csr_rows(0, d.total_cells)), iterations=[])
    for _ in range(30):
        s = g.em_iteration(5.0)
        it = dict(summary=tuple(getattr(s, f) for f, _ in s._fields_), excluded=g.excluded(), loci_mask=g.loci_mask())
        it.update({"cell_" + k: v for k, v in g.cell_outputs().items()})
        it.update({"locus_" + k: v for k, v in g.locus_outputs().items()})
        out["iterations"].append(it)
        if not s.any_change:
            break
    else:
        raise AssertionError("no convergence")
    out.update({"assign_" + k: v for k, v in g.assign(0.999, 30).items()})
    return out


def _same_bits(a, b, path=""):
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), path
        for k in a:
            _same_bits(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, list):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same_bits(x, y, f"{path}[{i}]")
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape, path
        assert a.tobytes() == b.tobytes(), f"{path}: {int((a != b).sum())} of {a.size} values differ"
    elif isinstance(a, tuple):
        assert np.array(a, np.float64).tobytes() == np.array(b, np.float64).tobytes(), (path, a, b)
    else:
        assert a == b, path


def _with_doublets(env, case, engine, loaded=True):
    g = _make(env, engine)
    if loaded:
        g.load_coo(L0, N0, *case["coo"])
        g.run(5.0, 30)
    else:
        g.ingest_coo(L0, N0, *case["coo"])
    g.add_doublets(case["a"], case["b"], 0.5, 4)
    g.ingest_finish()
    return g


@pytest.mark.parametrize("engine", [2, 1], ids=["tiled", "csr"])
def test_ctx_with_doublets_equals_a_fresh_load(env, case, engine):
    t = case["twin"]
    f = _make(env, engine)
    f.load_coo(L0, t[4], *t[:4])
    want = _collect(f)
    f.close()
    g = _with_doublets(env, case, engine)  # (from a loaded ctx that has run: nothing of the former matrix may leak)
    got = _collect(g)
    assert got["dims"][:2] == (N0 + NP, L0)
    _same_bits(got, want)
    _same_arrays(g.staged_coo(), t[:4])
    assert np.array_equal(g.cell_origin(), t[5]) and np.array_equal(g.cell_source(), t[6])
    g.close()


@pytest.mark.parametrize("engine", [2, 1], ids=["tiled", "csr"])
def test_ctx_with_doublets_against_the_oracle(env, case, engine):
    t = case["twin"]
    g = _with_doublets(env, case, engine, loaded=False)  # (in state STAGED this time)
    o = env["ob"].Oracle.from_coo(L0, t[4], *t[:4])
    assert np.array_equal(g.locus_ids(), o.locus_ids())
    assert np.array_equal(g.entries_per_cell(), o.entries_per_cell())
    for _ in range(30):
        sg, so = g.em_iteration(5.0), o.em_iteration(5.0)
        assert sg.n_near_threshold == 0
        assert (sg.any_change, sg.n_new_excluded, sg.n_rescued) == (so.any_change, so.n_new_excluded, so.n_rescued)
        assert np.array_equal(g.excluded(), o.excluded()) and np.array_equal(g.loci_mask(), o.loci_mask())
        if not so.any_change:
            break
    else:
        raise AssertionError("no convergence")
    po = o.posteriors()
    pa, aa, _ = o.assignments(po["posterior"], po["doublet_posterior"], 0.999, 30)
    res = g.assign(0.999, 30)
    np.testing.assert_allclose(res["posterior"], po["posterior"], rtol=0, atol=POST_ATOL)
    np.testing.assert_allclose(res["doublet_posterior"], po["doublet_posterior"], rtol=0, atol=POST_ATOL)
    assert np.array_equal(res["posterior_assignment"], pa) and np.array_equal(res["anomaly_assignment"], aa)
    g.close(); o.close()


# ---- 4. refusals: the ctx unchanged ---------------------------------------------------------------------------------------------------
def _state(x):
    d = x.dims()
    return (d.total_cells, d.total_loci, d.loci_used, d.nnz_used), x.staged_coo(), x.cell_origin(), x.cell_source()


def _unchanged(x, before):
    now = _state(x)
    assert now[0] == before[0]
    _same_arrays(now[1], before[1])
    assert np.array_equal(now[2], before[2]) and np.array_equal(now[3], before[3])


def _summary(s):
    return tuple(getattr(s, k) for k, _ in s._fields_)


def test_refusals_leave_the_ctx_unchanged(env, case):
    coo = [x.copy() for x in case["coo"]]
    # two cells whose summed ref at one locus is 40000 + 40000, behind a legal pair
    c0, c1 = int(coo[1][0]), int(coo[1][1])
    l0 = int(coo[0][0])
    assert coo[0][1] == l0 and c0 != c1
    coo[3][0] = coo[3][1] = 40000
    g, f = _make(env), _make(env)
    for x in (g, f):
        x.load_coo(L0, N0, *coo)
    s0 = g.em_iteration(5.0)
    before = _state(g)
    lib, h = g._lib, g.h
    ok = np.array([5, 6], np.uint32)
    p0, p1, p2 = [c for c in range(N0) if c not in (c0, c1)][:3]
    calls = [
        (dict(cell_a=[], cell_b=[]), "no pairs"),
        (dict(cell_a=[1, 2, N0], cell_b=[2, 3, 1]), "pair 2"),
        (dict(cell_a=[1, 2, 3], cell_b=[2, N0 + 7, N0]), "pair 1"),
        (dict(cell_a=[1, 9, 3, 4], cell_b=[2, 9, 3, 5]), "pair 1 names cell 9 twice"),
        (dict(cell_a=[1], cell_b=[2], downsample_rate=1.5), "downsample_rate"),
        (dict(cell_a=[1], cell_b=[2], downsample_rate=-0.25), "downsample_rate"),
        (dict(cell_a=[1], cell_b=[2], downsample_rate=float("nan")), "downsample_rate"),
    ]
    for kw, word in calls:
        assert word in _einval(env, g.add_doublets, **kw), kw
        _unchanged(g, before)
    # a NULL list (the method always passes arrays)
    for pa, pb in ((None, ok.ctypes.data), (ok.ctypes.data, None)):
        assert lib.cellector_add_doublets(h, pa, pb, 2, 0.0, 4) == EINVAL
        assert b"NULL" in lib.cellector_last_error(h)
    # the summed count: known only after the doublet side is built; pair, locus and allele of the first such entry
    pairs_a, pairs_b = [p0, c1, c0, c0], [p1, c0, c1, p2]
    msg = _einval(env, g.add_doublets, pairs_a, pairs_b)
    assert f"pair 1 ({c1}, {c0})" in msg and f"locus {l0}" in msg and " ref " in msg and "65535" in msg
    with pytest.raises(ValueError) as e:
        env["doublets"].add_doublets_coo(coo, N0, pairs_a, pairs_b)
    assert f"pair 1 ({c1}, {c0})" in str(e.value) and f"locus {l0}" in str(e.value) and " ref " in str(e.value)
    _unchanged(g, before)
    # an iteration in flight
    g.em_begin()
    assert "em_begin" in _einval(env, g.add_doublets, [1], [2])
    g.em_threshold(5.0)
    _einval(env, g.add_doublets, [1], [2])
    s1 = g.em_finish()
    _unchanged(g, before)
    # still READY with its built matrix: the run it would have been, to the same fixed point
    for mine in (s0, s1):
        _same_bits(_summary(mine), _summary(f.em_iteration(5.0)))
    for _ in range(30):
        sg, sf = g.em_iteration(5.0), f.em_iteration(5.0)
        _same_bits(_summary(sg), _summary(sf))
        if not sf.any_change:
            break
    assert np.array_equal(g.excluded(), f.excluded())
    _same_bits(g.cell_outputs(), f.cell_outputs())
    # thinned, the same pairs are accepted
    g.add_doublets(pairs_a, pairs_b, 0.5)
    assert g.dims().total_cells == N0 + 4
    g.close(); f.close()


def test_ctxs_that_cannot_take_part_are_refused(env, case):
    coo = case["coo"]
    e = _make(env)  # state EMPTY
    assert "staged" in _einval(env, e.add_doublets, [0], [1])
    e.close()
    m = _make(env, devices=[0, 0])
    m.load_coo(L0, N0, *coo)
    assert "multi-device" in _einval(env, m.add_doublets, [0], [1])
    assert m.dims().total_cells == N0
    m.close()
    h = _make(env)
    h.set_shard(0, 300)
    h.ingest_coo(L0, N0, *coo)
    assert "set_shard" in _einval(env, h.add_doublets, [0], [1])
    h.close()
    k = _make(env, keep_coo=0)
    k.load_coo(L0, N0, *coo)
    assert "keep_coo" in _einval(env, k.add_doublets, [0], [1])
    k.close()


def test_a_ctx_with_a_communicator_is_refused(env, case):
    """a one-rank communicator (the RCCL self-test of tests/test_gpu_em_state.py) makes the ctx one whose ranks stage their own cells"""
    import os
    os.environ["CELLECTOR_COMM_SELFTEST"] = "1"
    try:
        m = _make(env)
        m.comm_init_rank(env["ffi"].comm_unique_id(), 1, 0)
    finally:
        os.environ.pop("CELLECTOR_COMM_SELFTEST", None)
    f = _make(env)
    for x in (m, f):
        x.load_coo(L0, N0, *case["coo"])
    s0 = m.em_iteration(5.0)
    before = _state(m)
    assert "communicator" in _einval(env, m.add_doublets, [0], [1])
    _unchanged(m, before)
    _same_bits(_summary(s0), _summary(f.em_iteration(5.0)))
    _same_bits(_summary(m.em_iteration(5.0)), _summary(f.em_iteration(5.0)))
    m.close(); f.close()


def test_refusals_by_the_counts(env):
    one = [np.zeros(2, np.uint32), np.arange(2, dtype=np.uint32), np.ones(2, np.uint32), np.ones(2, np.uint32)]
    # n_ctx + n_pairs above 2^32 - 1: a ctx of 2^32 - 2 cells without entries costs nothing while STAGED
    g = _make(env)
    none = [np.zeros(0, np.uint32)] * 4
    g.ingest_coo(1, 2 ** 32 - 2, *none)
    assert "cells" in _einval(env, g.add_doublets, [0, 1], [1, 0])
    assert g.dims().total_cells == 2 ** 32 - 2 and len(g.staged_coo()[0]) == 0
    # 255 combines since the last ingest from outside, the next one is refused
    g.ingest_coo(1, 2, *one)
    for k in range(255):
        g.add_doublets([0], [1], 1.0)
    assert g.dims().total_cells == 257 and np.array_equal(g.cell_source(), np.concatenate([[0], np.arange(256)]))
    before = _state(g)
    assert "255" in _einval(env, g.add_doublets, [0], [1])
    _unchanged(g, before)
    g.ingest_coo(1, 2, *one)  # the counter starts again
    g.add_doublets([0], [1])
    assert g.cell_source().tolist() == [0, 0, 1] and g.staged_coo()[2].tolist() == [1, 1, 2]
    g.close()
