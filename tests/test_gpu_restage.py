"""GPU: cellector_restage — a cell subset, renumbered, and per-read downsampling of the resident matrix.

1. The kernel against its numpy twin (cellector_amd/restage.py): staged_coo(), dims().total_cells and cell_origin() are equal
   exactly, on entry counts around the wave (64), the block (256) and the tile (restage.TILE), under keep patterns that make a
   whole wave vote 0 and the next one 1, drop the first and the last entry, and keep a cell without entries.
2. A restaged ctx against a fresh ctx that loads the twin's arrays: both run the same build on the same arrays, so every output is
   equal to the bit, and any difference is state that leaked from the former matrix.  test_two_fresh_loads_agree shows first that
   two fresh loads of the same arrays agree to the bit in everything compared here.
3. Against the CPU oracle on the twin's arrays, with the suite's standing bounds: exclusion flags and labels identical, posteriors
   within 1e-6 (README "Parity").
4. State and errors: the call order, the options that survive, and every refusal with the ctx unchanged.

The equivalence cases are those of the issue: 1500 x 800 at 10 % (120 148 entries, L = 1014, 81 cells excluded at the fixed
point); (a) 569 cells, L = 893; (b) the peel, 719 cells, L = 483, nothing excluded; (c) rate 0.6, 61 634 entries at 0 / 0, L = 731.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POST_ATOL = 1e-6
EINVAL = 1
L0, N0 = 1500, 800


@pytest.fixture(scope="module")
def env(oracle_lib, hip_lib_path):
    from cellector_amd import Cellector, ffi, restage, synth
    return dict(Cellector=Cellector, ffi=ffi, restage=restage, synth=synth, ob=oracle_lib)


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


# ---- 1. the kernel against the twin -------------------------------------------------------------------------------------------
N_CELLS = 41  # cell N_CELLS - 2 never has an entry


def _hand_coo(n, seed=0):
    """locus-major; the entries [64, 128) belong to cell 1, [128, 192) to cell 2, [300, 500) to cell 1: runs that fill whole waves"""
    rng = np.random.default_rng(1000 + n + seed)
    locus = (np.arange(n) // 7).astype(np.uint32)
    cell = rng.integers(3, N_CELLS - 2, n).astype(np.uint32)
    cell[64:128] = 1
    cell[128:192] = 2
    cell[300:500] = 1
    if n:
        cell[0] = 0
    if n > 1:
        cell[-1] = N_CELLS - 1
    alt = rng.integers(0, 6, n).astype(np.uint32)
    ref = rng.integers(0, 8, n).astype(np.uint32)
    return n // 7 + 1, locus, cell, alt, ref


def _patterns(cell):
    rng = np.random.default_rng(5)
    one = lambda i: np.eye(1, N_CELLS, i, dtype=bool)[0]
    run = rng.random(N_CELLS) < 0.5
    run[1], run[2] = False, True  # a whole wave votes 0, the next one 1
    ends = np.ones(N_CELLS, bool)
    if len(cell):
        ends[cell[0]] = ends[cell[-1]] = False  # the first and the last entry leave
    empty = rng.random(N_CELLS) < 0.5
    empty[N_CELLS - 2] = True  # a kept cell without entries
    return {"all": np.ones(N_CELLS, bool), "none_given": None, "first": one(0), "last": one(N_CELLS - 1),
            "alternating": np.arange(N_CELLS) % 2 == 0, "run": run, "ends": ends, "empty_row": empty}


def _nnz_cases():
    from cellector_amd import restage
    t = restage.TILE
    return [0, 1, 63, 64, 65, 255, 256, 257, t - 1, t, t + 1, 2 * t + 65]


def _check_against_twin(env, g, src, n_cells, keep, rate, seed):
    want = env["restage"].restage_coo(*src, n_cells, keep, rate, seed)
    g.restage(keep, rate, seed)
    got = g.staged_coo()
    for k, name in enumerate(("locus", "cell", "alt", "ref")):
        assert np.array_equal(got[k], want[k]), name
    assert g.dims().total_cells == want[4]
    assert np.array_equal(g.cell_origin(), want[5])
    return want


@pytest.mark.parametrize("nnz", _nnz_cases())
def test_kernel_equals_the_twin(env, nnz):
    tl, *src = _hand_coo(nnz)
    g = _make(env)
    for name, keep in _patterns(src[1]).items():
        for rate in (0.0, 0.37, 1.0):
            g.ingest_coo(tl, N_CELLS, *src)
            assert np.array_equal(g.cell_origin(), np.arange(N_CELLS))  # an ingest from outside: identity
            want = _check_against_twin(env, g, src, N_CELLS, keep, rate, 4)
            if rate == 1.0:
                assert not want[2].any() and not want[3].any()
            if keep is not None and rate == 0.0:
                assert len(want[0]) == int(keep[src[1]].sum())
    g.close()


def test_full_counts_at_rate_one_half(env):
    src = [np.array([0], np.uint32), np.array([1], np.uint32), np.array([65535], np.uint32), np.array([65535], np.uint32)]
    g = _make(env)
    for keep in (None, np.array([False, True, True])):
        g.ingest_coo(1, 3, *src)
        want = _check_against_twin(env, g, src, 3, keep, 0.5, 4)
        for k in (2, 3):  # 65535 fair draws: within 6 sigma of the half
            assert abs(int(want[k][0]) - 32767.5) < 6 * 128
    g.close()


def test_input_that_is_not_locus_major(env):
    """staged order is file order before the finish and the ingest's stable locus sort after it: the draw follows it"""
    rng = np.random.default_rng(21)
    n, tl, nc = 700, 60, 50
    src = [rng.integers(0, tl, n).astype(np.uint32), rng.integers(0, nc, n).astype(np.uint32),
           rng.integers(0, 5, n).astype(np.uint32), rng.integers(0, 5, n).astype(np.uint32)]
    assert (np.diff(src[0].astype(np.int64)) < 0).any()
    keep = rng.random(nc) < 0.7
    g = _make(env)
    g.ingest_coo(tl, nc, *src)
    in_file_order = _check_against_twin(env, g, src, nc, keep, 0.37, 4)
    g.ingest_coo(tl, nc, *src)
    g.ingest_finish(1, 1)
    order = np.argsort(src[0], kind="stable")
    for got, s in zip(g.staged_coo(), src):
        assert np.array_equal(got, s[order])
    in_sorted_order = _check_against_twin(env, g, [s[order] for s in src], nc, keep, 0.37, 4)
    # the same multiset of (locus, cell) pairs, other draws
    assert len(in_file_order[0]) == len(in_sorted_order[0])
    o2 = np.argsort(in_file_order[0], kind="stable")
    assert np.array_equal(in_file_order[1][o2], in_sorted_order[1])
    assert not (np.array_equal(in_file_order[2][o2], in_sorted_order[2]) and np.array_equal(in_file_order[3][o2], in_sorted_order[3]))
    g.ingest_finish(1, 1)
    assert g.dims().total_cells == int(keep.sum())
    g.close()


# ---- 2. / 3. a restaged ctx, a fresh load of the twin's arrays, the oracle ------------------------------------------------------
@pytest.fixture(scope="module")
def full(env):
    """the matrix, the oracle's fixed point on it, and the three restages with the twin's arrays"""
    coo = env["synth"].generate_coo(L0, N0, 0.1, seed=11, minority_fraction=0.08, doublet_fraction=0.01)
    assert len(coo[0]) == 120148
    o = env["ob"].Oracle.from_coo(L0, N0, *coo)
    o.run(5.0, 30)
    excluded = o.excluded().copy()
    assert len(o.locus_ids()) == 1014 and int(excluded.sum()) == 81
    o.close()
    keep_a = np.random.default_rng(3).random(N0) < 0.7
    keep_a[0], keep_a[N0 - 1] = False, True
    args = {"a": (keep_a, 0.0, 4), "b": (excluded == 0, 0.0, 4), "c": (None, 0.6, 4)}
    twin = {k: env["restage"].restage_coo(*coo, N0, *a) for k, a in args.items()}
    assert (twin["a"][4], twin["b"][4], twin["c"][4]) == (569, 719, 800)
    assert int(((twin["c"][2] == 0) & (twin["c"][3] == 0)).sum()) == 61634
    return dict(coo=coo, excluded=excluded, args=args, twin=twin)


EXPECT = {"a": dict(L=893), "b": dict(L=483, n_excluded=0), "c": dict(L=731)}


def _collect(g):
    """everything the equivalence compares, after running to the fixed point"""
    d = g.dims()
    out = dict(dims=(d.total_cells, d.total_loci, d.loci_used, d.cell_begin, d.cell_end, d.nnz_used), locus_ids=g.locus_ids(),
               locus_counts=g.locus_counts(), entries_per_cell=g.entries_per_cell(), iterations=[])
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
    out.update({"tally_" + k: v for k, v in g.final_allele_tallies().items()})
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


_fresh_cache = {}


def _fresh(env, full, case, engine):
    if (case, engine) not in _fresh_cache:
        t = full["twin"][case]
        g = _make(env, engine)
        g.load_coo(L0, t[4], *t[:4])
        _fresh_cache[(case, engine)] = _collect(g)
        g.close()
    return _fresh_cache[(case, engine)]


@pytest.mark.parametrize("engine", [2, 1], ids=["tiled", "csr"])
def test_two_fresh_loads_agree(env, full, engine):
    t = full["twin"]["a"]
    g = _make(env, engine)
    g.load_coo(L0, t[4], *t[:4])
    _same_bits(_collect(g), _fresh(env, full, "a", engine))
    g.close()


@pytest.mark.parametrize("case", ["a", "b", "c"])
@pytest.mark.parametrize("engine", [2, 1], ids=["tiled", "csr"])
def test_restaged_ctx_equals_a_fresh_load(env, full, engine, case):
    g = _make(env, engine)
    g.load_coo(L0, N0, *full["coo"])
    assert g.dims().loci_used == 1014
    g.run(5.0, 30)
    assert np.array_equal(g.excluded(), full["excluded"])
    keep, rate, seed = full["args"][case]
    if case == "b":
        keep = g.excluded() == 0  # the peel, from the ctx's own set
    g.restage(keep, rate, seed)
    g.ingest_finish()
    got = _collect(g)
    want = _fresh(env, full, case, engine)
    assert got["dims"][2] == EXPECT[case]["L"] and got["dims"][0] == full["twin"][case][4]
    if "n_excluded" in EXPECT[case]:
        assert int(got["iterations"][-1]["excluded"].sum()) == EXPECT[case]["n_excluded"]
    _same_bits(got, want)
    assert np.array_equal(g.cell_origin(), full["twin"][case][5])
    g.close()


@pytest.mark.parametrize("case", ["a", "b", "c"])
@pytest.mark.parametrize("engine", [2, 1], ids=["tiled", "csr"])
def test_restaged_ctx_against_the_oracle(env, full, engine, case):
    t = full["twin"][case]
    g = _make(env, engine)
    g.ingest_coo(L0, N0, *full["coo"])
    g.restage(*full["args"][case])  # (in state STAGED this time)
    g.ingest_finish()
    o = env["ob"].Oracle.from_coo(L0, t[4], *t[:4])
    assert np.array_equal(g.locus_ids(), o.locus_ids()) and len(o.locus_ids()) == EXPECT[case]["L"]
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


# ---- 4. state and errors ------------------------------------------------------------------------------------------------------
def test_call_order_and_surviving_options(env, full):
    t = full["twin"]["a"]
    keep = full["args"]["a"][0]
    g = _make(env, 2, normalization=1)
    g.load_coo(L0, N0, *full["coo"])
    g.em_iteration(5.0)
    g.restage(keep)
    _einval(env, g.em_iteration, 5.0)  # STAGED: no matrix to iterate on
    g.ingest_finish()
    f = _make(env, 2, normalization=1)
    f.load_coo(L0, t[4], *t[:4])
    _same_bits(_collect(g), _collect(f))  # the z-score keys: the option survived
    g.close(); f.close()
    # resolve_ties with a file-order copy that belongs to the new matrix
    g = _make(env, 2, resolve_ties=1)
    g.load_coo(L0, N0, *full["coo"])
    g.run(5.0, 30)
    g.restage(keep)
    g.ingest_finish()
    f = _make(env, 2, resolve_ties=1)
    f.load_coo(L0, t[4], *t[:4])
    a, b = _collect(g), _collect(f)
    _same_bits(a, b)
    assert g.resolution().mode == 1 and np.array_equal(g.resolved_cells(), f.resolved_cells())
    g.close(); f.close()


def test_two_restages_compose_in_cell_origin(env, full):
    keep1 = full["args"]["a"][0]
    g = _make(env)
    g.load_coo(L0, N0, *full["coo"])
    g.restage(keep1)
    first = np.nonzero(keep1)[0]
    assert np.array_equal(g.cell_origin(), first)
    keep2 = np.arange(len(first)) % 3 != 1
    g.restage(keep2, 0.0)
    assert np.array_equal(g.cell_origin(), first[keep2]) and g.dims().total_cells == int(keep2.sum())
    g.restage()  # all cells, rate 0: the same entries staged again
    assert np.array_equal(g.cell_origin(), first[keep2])
    both = np.zeros(N0, bool)
    both[first[keep2]] = True
    want = env["restage"].restage_coo(*full["coo"], N0, both)
    for got, w in zip(g.staged_coo(), want[:4]):
        assert np.array_equal(got, w)
    g.ingest_finish()
    g.load_coo(L0, N0, *full["coo"])  # an ingest from outside: identity again
    assert np.array_equal(g.cell_origin(), np.arange(N0))
    g.close()


def test_back_from_ready_to_staged_for_another_min_alt(env, full):
    g = _make(env)
    g.load_coo(L0, N0, *full["coo"])
    g.restage()
    g.ingest_finish(8, 8)
    f = _make(env)
    f.load_coo(L0, N0, *full["coo"], min_alt=8, min_ref=8)
    assert g.dims().loci_used == f.dims().loci_used < 1014
    _same_bits(_collect(g), _collect(f))
    g.close(); f.close()


def test_keep_coo_zero_refuses_in_ready_and_the_ctx_still_iterates(env, full):
    g = _make(env, keep_coo=0)
    g.ingest_coo(L0, N0, *full["coo"])
    g.restage(full["args"]["a"][0])  # STAGED is always allowed
    g.ingest_finish()
    assert "keep_coo" in _einval(env, g.restage)
    assert g.dims().total_cells == 569 and g.dims().loci_used == 893
    f = _fresh(env, full, "a", 2)
    s = g.em_iteration(5.0)
    assert tuple(getattr(s, k) for k, _ in s._fields_) == f["iterations"][0]["summary"]
    g.close()


def test_refusals_leave_the_ctx_unchanged(env, full):
    keep = full["args"]["a"][0]
    g = _make(env, devices=[0, 0])
    g.load_coo(L0, N0, *full["coo"])
    assert "single-device" in _einval(env, g.restage, keep)
    assert g.dims().total_cells == N0
    g.close()
    g = _make(env)
    assert "staged" in _einval(env, g.restage)  # state EMPTY
    g.set_shard(0, 400)
    g.ingest_coo(L0, N0, *full["coo"])
    assert "set_shard" in _einval(env, g.restage, None, 0.5)
    g.close()
    g = _make(env)
    g.load_coo(L0, N0, *full["coo"])
    s0 = g.em_iteration(5.0)
    before = g.staged_coo()
    for kw in (dict(downsample_rate=1.5), dict(downsample_rate=float("nan")), dict(downsample_rate=-0.25), dict(keep=np.zeros(N0, bool))):
        _einval(env, g.restage, **kw)
    g.em_begin()
    assert "em_begin" in _einval(env, g.restage, keep)
    g.em_threshold(5.0)
    _einval(env, g.restage, keep)
    s1 = g.em_finish()
    d = g.dims()
    assert (d.total_cells, d.loci_used) == (N0, 1014) and s1.n_excluded > 0 and s0.n_new_excluded > 0
    for a, b in zip(before, g.staged_coo()):
        assert np.array_equal(a, b)
    # ... and it is the run it would have been
    f = _make(env)
    f.load_coo(L0, N0, *full["coo"])
    f.em_iteration(5.0)
    s2 = f.em_iteration(5.0)
    assert tuple(getattr(s1, k) for k, _ in s1._fields_) == tuple(getattr(s2, k) for k, _ in s2._fields_)
    assert np.array_equal(g.excluded(), f.excluded())
    g.close(); f.close()


def test_the_staged_group_across_unbuilds_with_a_bound_pass1(env):
    """What the ctx keeps when a READY matrix goes back to STAGED, with a caller-bound PASS1 buffer: the binding (pointer, length),
    PASS1's contents (those of a fresh ctx, with a buffer of its own, that ingests the twin's arrays; exactly), cell_origin and
    cell_source; and what the next ingest from outside resets.  4 loci x 3 cells, six entries, finished with min_alt = min_ref = 1
    (three cells cannot meet the default of 4)."""
    import ctypes as C
    import torch
    from cellector_amd import doublets
    ffi = env["ffi"]
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpy.restype = C.c_int
    TL, P1_PLANES = 4, 5

    def fresh_pass1(n_cells, coo):
        f = _make(env)
        f.ingest_coo(TL, n_cells, *coo)
        ptr, n = f.exchange_buffer(ffi.XCHG_PASS1)
        out = np.empty(n)
        assert n == P1_PLANES * TL and hip.hipMemcpy(out.ctypes.data, ptr, n * 8, 2) == 0  # device to host
        f.close()
        return out

    def bound_pass1(g):
        assert g.exchange_buffer(ffi.XCHG_PASS1) == (buf.data_ptr(), P1_PLANES * TL)  # the same buffer, all of it in use
        torch.cuda.synchronize()
        return buf.cpu().numpy()

    u32 = lambda *v: np.array(v, np.uint32)
    coo = [u32(0, 0, 1, 2, 2, 3), u32(0, 2, 1, 0, 1, 2), u32(1, 2, 0, 3, 1, 2), u32(2, 0, 4, 1, 1, 5)]
    buf = torch.zeros(P1_PLANES * TL, dtype=torch.float64, device="cuda:0")
    g = _make(env)
    g.bind_exchange_buffer(ffi.XCHG_PASS1, buf.data_ptr(), buf.numel())
    g.ingest_coo(TL, 3, *coo)
    g.ingest_finish(1, 1)
    # 1. a restage from READY
    keep = np.array([1, 0, 1], np.uint8)
    t1 = env["restage"].restage_coo(*coo, 3, keep)
    g.restage(keep)
    assert bound_pass1(g).tobytes() == fresh_pass1(t1[4], t1[:4]).tobytes()
    assert g.cell_origin().tolist() == [0, 2] and t1[5].tolist() == [0, 2]
    for got, want in zip(g.staged_coo(), t1[:4]):
        assert np.array_equal(got, want)
    # 2. add_doublets from READY
    g.ingest_finish(1, 1)
    t2 = doublets.add_doublets_coo(t1[:4], t1[4], [0], [1], origin=t1[5])
    g.add_doublets([0], [1])
    assert bound_pass1(g).tobytes() == fresh_pass1(t2[4], t2[:4]).tobytes()
    assert g.cell_source().tolist() == [0, 0, 1] and g.cell_origin().tolist() == [0, 2, 0] == t2[5].tolist()
    for got, want in zip(g.staged_coo(), t2[:4]):
        assert np.array_equal(got, want)
    # 3. an ingest from outside: origin and source start again, and so does the combine counter
    other = [u32(0, 1, 3), u32(1, 0, 2), u32(1, 1, 2), u32(0, 3, 1)]
    g.ingest_coo(TL, 3, *other)
    assert g.cell_origin().tolist() == [0, 1, 2] and g.cell_source().tolist() == [0, 0, 0]
    assert bound_pass1(g).tobytes() == fresh_pass1(3, other).tobytes()
    s = _make(env)
    s.ingest_coo(TL, 1, u32(2), u32(0), u32(1), u32(1))
    g.combine(s)
    assert g.cell_source().tolist() == [0, 0, 0, 1]
    bound_pass1(g)
    g.close(); s.close()
