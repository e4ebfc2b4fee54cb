"""GPU: cellector_combine — a second staged matrix merged in on the device — and cellector_cell_source.

1. The kernel against its numpy twin (cellector_amd/combine.py): staged_coo(), dims(), cell_origin() and cell_source() are equal
   exactly and src.staged_coo() is unchanged, on hand-made sides whose entry counts lie around the wave (64), the block (256) and
   the merge tile (combine.TILE), laid out so that the two sides meet the tile edges in every way: one side wholly above or below
   the other, strict alternation, a run of one side longer than a tile, a switch of sides exactly at a tile edge, repeated
   (locus, cell) lines across a tile edge.  Plus a non-monotone map (src goes through the sort), a ctx staged from input that is
   not locus-major, and a map that folds two src loci into one.
2. A combined ctx against a fresh ctx that loads the twin's arrays, both engines: equal to the bit.
3. Against the CPU oracle on the twin's arrays, with the suite's standing bounds.
4. The loop: combine -> finish -> run -> restage(keep = cell_source() == 0) gives ctx's original entries back; a second combine has
   source 2; a loaded src still iterates exactly as before.
5. Every refusal, with both ctxs unchanged.

The equivalence case is the issue's: ctx 1500 x 800 at 10 % (120 148 entries), src 1400 x 300 (41 274 entries), the map
j -> (7 j + 3) mod 1500 for j < 1300 and 1500 + (j - 1300) above, 1600 loci out, keep = default_rng(3).random(300) < 0.25, rate 0.2,
seed 4: 866 cells, 129 204 entries, L = 907; the oracle converges in 2 iterations and excludes exactly the 66 src cells.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POST_ATOL = 1e-6
EINVAL = 1


@pytest.fixture(scope="module")
def env(oracle_lib, hip_lib_path):
    from cellector_amd import Cellector, combine, ffi, restage, synth
    return dict(Cellector=Cellector, ffi=ffi, restage=restage, combine=combine, synth=synth, ob=oracle_lib)


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


# ---- 1. the kernel against the twin -------------------------------------------------------------------------------------------
def _tile():
    from cellector_amd import combine
    return combine.TILE


def _sizes():
    t = _tile()
    return [0, 1, 63, 64, 65, 255, 256, 257, t - 1, t, t + 1, 2 * t + 65]


def _pairs():
    t, xs = _tile(), _sizes()
    out = [(x, x) for x in xs] + [(0, x) for x in xs[1:]] + [(x, 0) for x in xs[1:]]
    return out + [(t - 1, 1), (1, t - 1), (2 * t + 65, 65), (65, 2 * t + 65)]


def _side(loci, seed):
    """a side from its entries' loci (ascending): (n_cells, [locus, cell, alt, ref]), (locus, cell) strictly ascending.  The cell is
    the entry's index inside its locus; the last entry moves to the last cell; the cell before that one never has an entry."""
    loci = np.asarray(loci, dtype=np.uint32)
    n = len(loci)
    rng = np.random.default_rng(7000 + 13 * n + seed)
    first = np.searchsorted(loci, loci, side="left")
    cell = (np.arange(n) - first).astype(np.uint32)
    n_cells = (int(cell.max()) + 1 if n else 0) + 2
    if n > 1:
        cell[-1] = n_cells - 1
    return n_cells, [loci, cell, rng.integers(0, 6, n).astype(np.uint32), rng.integers(0, 8, n).astype(np.uint32)]


SHAPES = ("src_above", "src_below", "alternating", "long_run", "switch_at_tile", "repeats_across_tile")


def _shape(shape, na, nb):
    """(loci of ctx's entries, loci of src's, repeat) or None where the pair cannot form the shape.  src's cells come behind ctx's,
    so inside a locus ctx's entries precede src's; repeat = (side, first index, count): entries of that side made one line"""
    t = _tile()
    if shape == "src_above":
        return np.arange(na) // 3, na // 3 + 1 + np.arange(nb) // 3, None
    if shape == "src_below":
        return nb // 3 + 1 + np.arange(na) // 3, np.arange(nb) // 3, None
    if na == 0 or nb == 0:
        return None
    if shape == "alternating":  # locus i: one entry of each side; what the longer side has left follows, three to a locus
        m = min(na, nb)
        tail = lambda n: np.concatenate([np.arange(m), m + np.arange(n - m) // 3])
        return tail(na), tail(nb), None
    if shape == "long_run":  # the longer side wholly inside locus 1, between two entries of the other (more than a tile at 2T + 65)
        if min(na, nb) < 2:
            return None
        ends = lambda n: np.concatenate([np.zeros(n - 1, np.int64), [2]])
        return (np.ones(na, np.int64), ends(nb), None) if na >= nb else (ends(na), np.ones(nb, np.int64), None)
    if shape == "switch_at_tile":  # output index T - 1 is the last of side X's first stretch, index T the other side's
        if na + nb < t + 1:
            return None
        x, y = max(na, nb), min(na, nb)
        if x >= t:
            lx = np.concatenate([np.arange(t) // 5, 2 * t + np.arange(x - t) // 5])
            ly = np.full(y, t)
        else:  # Y leads with T - x entries, all of X, then the rest of Y
            lead = t - x
            lx = 1 + np.arange(x) // 5
            ly = np.concatenate([np.zeros(lead, np.int64), t + np.arange(y - lead) // 5])
        return (lx, ly, None) if na >= nb else (ly, lx, None)
    if shape == "repeats_across_tile":  # the longer side first in the output; its entries T - 2 .. T + 1 are one (locus, cell) line
        x = max(na, nb)
        if x < t + 2:
            return None
        lx, ly = np.arange(x) // 4, x + np.arange(min(na, nb)) // 4
        rep = ("ctx" if na >= nb else "src", t - 2, 4)
        return (lx, ly, rep) if na >= nb else (ly, lx, rep)
    raise AssertionError(shape)


def _sides(shape, na, nb):
    s = _shape(shape, na, nb)
    if s is None:
        return None
    (n_ctx, ctx), (n_src, src) = _side(s[0], 1), _side(s[1], 2)
    assert len(ctx[0]) == na and len(src[0]) == nb
    if s[2]:
        side, at, cnt = s[2]
        a = ctx if side == "ctx" else src
        a[0][at:at + cnt] = a[0][at]
        a[1][at:at + cnt] = a[1][at]
        a[2][at:at + cnt] = [3, 1, 1, 2]  # (ref, alt) decide: out of order as given
        a[3][at:at + cnt] = [2, 2, 1, 0]
    total_loci = max([1] + [int(a[0].max()) + 1 for a in (ctx, src) if len(a[0])])
    return total_loci, n_ctx, ctx, n_src, src


def _keeps(n_src):
    one = lambda i: np.eye(1, n_src, i, dtype=bool)[0]
    empty = np.arange(n_src) % 3 != 1
    empty[n_src - 2] = True  # a kept cell without entries
    return {"none_given": None, "first": one(0), "last": one(n_src - 1), "alternating": np.arange(n_src) % 2 == 0, "empty_row": empty}


def _combine_and_check(env, g, s, tl, n_ctx, ctx, n_src, src, keep, lmap, tlo, rate, seed=4, **twin_kw):
    """one combine into g (staged with ctx's arrays) from s (src's): everything equal to the twin, s untouched"""
    want = env["combine"].combine_coo(ctx, n_ctx, src, n_src, keep, lmap, tlo, rate, seed, **twin_kw)
    g.combine(s, keep, lmap, tlo, rate, seed)
    _same_arrays(g.staged_coo(), want[:4], "staged_coo")
    d = g.dims()
    assert (d.total_cells, d.total_loci, d.cell_begin, d.cell_end) == (want[4], tlo, 0, want[4])
    assert np.array_equal(g.cell_origin(), want[5]) and np.array_equal(g.cell_source(), want[6])
    return want


@pytest.mark.parametrize("na,nb", _pairs())
def test_kernel_equals_the_twin(env, na, nb):
    g, s = _make(env), _make(env)
    formed = 0
    for shape in SHAPES:
        made = _sides(shape, na, nb)
        if made is None:
            continue
        formed += 1
        tl, n_ctx, ctx, n_src, src = made
        s.ingest_coo(tl, n_src, *src)
        for name, keep in _keeps(n_src).items():
            for rate in (0.0, 0.37, 1.0):
                g.ingest_coo(tl, n_ctx, *ctx)
                want = _combine_and_check(env, g, s, tl, n_ctx, ctx, n_src, src, keep, None, tl, rate)
                if rate == 0.0:
                    assert len(want[0]) == na + (nb if keep is None else int(keep[src[1]].sum()))
        _same_arrays(s.staged_coo(), src, "src after the combines")
        sd = s.dims()
        assert (sd.total_cells, sd.total_loci) == (n_src, tl)
    assert formed >= 2  # the empty pairs form the two one-sided shapes, every other pair at least the first three
    g.close(); s.close()


def test_shapes_meet_the_tile_edges_as_claimed(env):
    """the layouts above do what their names say, at rate 0 with all cells, on the twin's output"""
    t = _tile()
    for na, nb in ((2 * t + 65, 65), (65, 2 * t + 65), (t + 1, t + 1), (t - 1, t - 1)):
        for shape in SHAPES[2:]:
            made = _sides(shape, na, nb)
            if made is None:
                assert shape in ("switch_at_tile", "repeats_across_tile") and max(na, nb) < t + 2
                continue
            tl, n_ctx, ctx, n_src, src = made
            w = env["combine"].combine_coo(ctx, n_ctx, src, n_src, None, None, tl)
            from_src = w[1] >= n_ctx
            if shape == "alternating":
                m = 2 * min(na, nb)
                assert np.array_equal(from_src[:m], np.arange(m) % 2 == 1)
            elif shape == "long_run":
                runs = np.diff(np.flatnonzero(np.diff(from_src.astype(np.int8)) != 0))
                assert runs.max() == max(na, nb) and (max(na, nb) < t or runs.max() > t)
            elif shape == "switch_at_tile":
                assert from_src[t - 1] != from_src[t]
            else:
                key = w[0].astype(np.uint64) << np.uint64(32) | w[1].astype(np.uint64)
                assert len(set(key[t - 2:t + 2].tolist())) == 1 and key[t - 3] != key[t - 2] != key[t + 2]
                assert w[3][t - 2:t + 2].tolist() == [0, 1, 2, 2] and w[2][t - 2:t + 2].tolist() == [2, 1, 1, 3]


T = _tile()


@pytest.mark.parametrize("na,nb", [(257, 257), (65, 2 * T + 65), (T + 1, T + 1)])
def test_map_that_is_not_monotone_sends_src_through_the_sort(env, na, nb):
    made = _sides("alternating", na, nb)
    tl, n_ctx, ctx, n_src, src = made
    rng = np.random.default_rng(na)
    tlo = tl + 9
    lmap = rng.permutation(tlo)[:tl].astype(np.uint32)
    assert (np.diff(lmap[src[0]].astype(np.int64)) < 0).any()
    g, s = _make(env), _make(env)
    s.ingest_coo(tl, n_src, *src)
    for keep in (None, _keeps(n_src)["alternating"]):
        for rate in (0.0, 0.37):
            g.ingest_coo(tl, n_ctx, *ctx)
            _combine_and_check(env, g, s, tl, n_ctx, ctx, n_src, src, keep, lmap, tlo, rate)
    # the default total_loci: the larger of ctx's and 1 + the map's largest value
    g.ingest_coo(tl, n_ctx, *ctx)
    g.combine(s, locus_map=lmap)
    assert g.dims().total_loci == max(tl, int(lmap.max()) + 1)
    _same_arrays(s.staged_coo(), src, "src")
    g.close(); s.close()


@pytest.mark.parametrize("na,nb", [(257, 64), (2 * T + 65, 65), (T, T + 1)])
def test_ctx_staged_from_input_that_is_not_locus_major(env, na, nb):
    tl, n_ctx, ctx, n_src, src = _sides("alternating", na, nb)
    order = np.random.default_rng(nb).permutation(na)
    shuffled = [a[order] for a in ctx]
    assert (np.diff(shuffled[0].astype(np.int64)) < 0).any()
    g, s = _make(env), _make(env)
    s.ingest_coo(tl, n_src, *src)
    for rate in (0.0, 0.37):
        g.ingest_coo(tl, n_ctx, *shuffled)
        _same_arrays(g.staged_coo(), shuffled, "file order while STAGED")
        want = _combine_and_check(env, g, s, tl, n_ctx, shuffled, n_src, src, _keeps(n_src)["empty_row"], None, tl, rate)
        # ctx's reads are not drawn: the same result as from the sorted input
        _same_arrays(want[:4], env["combine"].combine_coo(ctx, n_ctx, src, n_src, _keeps(n_src)["empty_row"], None, tl, rate, 4)[:4])
    g.ingest_finish(1, 1)  # the merged COO is locus-major: the finish takes it as it stands
    _same_arrays(g.staged_coo(), want[:4], "after the finish")
    g.close(); s.close()


@pytest.mark.parametrize("na,nb", [(65, 257), (T + 1, 2 * T + 65)])
def test_map_that_folds_two_src_loci_into_one(env, na, nb):
    tl, n_ctx, ctx, n_src, src = _sides("src_above", na, nb)
    lmap = (np.arange(tl) // 2).astype(np.uint32)  # loci 2 m and 2 m + 1 meet: the same cells twice, (ref, alt) decide
    mapped = lmap[src[0]].astype(np.uint64) << np.uint64(32) | src[1].astype(np.uint64)
    assert len(np.unique(mapped)) < nb
    g, s = _make(env), _make(env)
    s.ingest_coo(tl, n_src, *src)
    for rate in (0.0, 0.37, 1.0):
        g.ingest_coo(tl, n_ctx, *ctx)
        _combine_and_check(env, g, s, tl, n_ctx, ctx, n_src, src, None, lmap, tl, rate)
    g.close(); s.close()


# ---- 2. / 3. the issue's case: a combined ctx, a fresh load of the twin's arrays, the oracle -------------------------------------
L0, N0, LS, NS, LOUT = 1500, 800, 1400, 300, 1600


@pytest.fixture(scope="module")
def case(env):
    dst = env["synth"].generate_coo(L0, N0, 0.1, seed=11, minority_fraction=0)
    src = env["synth"].generate_coo(LS, NS, 0.1, seed=12, minority_fraction=0)
    assert (len(dst[0]), len(src[0])) == (120148, 41274)
    j = np.arange(LS)
    lmap = np.where(j < 1300, (7 * j + 3) % 1500, 1500 + (j - 1300)).astype(np.uint32)
    keep = np.random.default_rng(3).random(NS) < 0.25
    twin = env["combine"].combine_coo(dst, N0, src, NS, keep, lmap, LOUT, 0.2, 4)
    assert (twin[4], len(twin[0])) == (866, 129204)
    return dict(dst=dst, src=src, lmap=lmap, keep=keep, twin=twin)


def _collect(g):
    """everything the equivalence compares, after running to the fixed point (tests/test_gpu_restage.py's)"""
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


def _combined(env, case, engine, loaded=True):
    g, s = _make(env, engine), _make(env, engine)
    s.ingest_coo(LS, NS, *case["src"])
    if loaded:
        g.load_coo(L0, N0, *case["dst"])
        g.run(5.0, 30)
    else:
        g.ingest_coo(L0, N0, *case["dst"])
    g.combine(s, case["keep"], case["lmap"], LOUT, 0.2, 4)
    s.close()
    g.ingest_finish()
    return g


@pytest.mark.parametrize("engine", [2, 1], ids=["tiled", "csr"])
def test_combined_ctx_equals_a_fresh_load(env, case, engine):
    t = case["twin"]
    f = _make(env, engine)
    f.load_coo(LOUT, t[4], *t[:4])
    want = _collect(f)
    f.close()
    g = _combined(env, case, engine)  # (from a loaded ctx that has run: nothing of the former matrix may leak)
    got = _collect(g)
    assert got["dims"][:3] == (866, LOUT, 907) and got["dims"][5] == want["dims"][5]
    _same_bits(got, want)
    _same_arrays(g.staged_coo(), t[:4])
    assert np.array_equal(g.cell_origin(), t[5]) and np.array_equal(g.cell_source(), t[6])
    g.close()


@pytest.mark.parametrize("engine", [2, 1], ids=["tiled", "csr"])
def test_combined_ctx_against_the_oracle(env, case, engine):
    t = case["twin"]
    g = _combined(env, case, engine, loaded=False)  # (in state STAGED this time)
    o = env["ob"].Oracle.from_coo(LOUT, t[4], *t[:4])
    assert np.array_equal(g.locus_ids(), o.locus_ids()) and len(o.locus_ids()) == 907
    assert np.array_equal(g.entries_per_cell(), o.entries_per_cell())
    n_iter = 0
    for _ in range(30):
        sg, so = g.em_iteration(5.0), o.em_iteration(5.0)
        n_iter += 1
        assert sg.n_near_threshold == 0
        assert (sg.any_change, sg.n_new_excluded, sg.n_rescued) == (so.any_change, so.n_new_excluded, so.n_rescued)
        assert np.array_equal(g.excluded(), o.excluded()) and np.array_equal(g.loci_mask(), o.loci_mask())
        if not so.any_change:
            break
    else:
        raise AssertionError("no convergence")
    assert n_iter == 2
    assert np.array_equal(o.excluded() != 0, t[6] == 1) and int(o.excluded().sum()) == 66  # exactly the src cells
    po = o.posteriors()
    pa, aa, _ = o.assignments(po["posterior"], po["doublet_posterior"], 0.999, 30)
    res = g.assign(0.999, 30)
    np.testing.assert_allclose(res["posterior"], po["posterior"], rtol=0, atol=POST_ATOL)
    np.testing.assert_allclose(res["doublet_posterior"], po["doublet_posterior"], rtol=0, atol=POST_ATOL)
    assert np.array_equal(res["posterior_assignment"], pa) and np.array_equal(res["anomaly_assignment"], aa)
    assert (pa[t[6] == 1] == 0).all() and (pa[t[6] == 0] == 1).all()
    g.close(); o.close()


# ---- 4. the loop ------------------------------------------------------------------------------------------------------------------
def test_the_titration_loop(env, case):
    t = case["twin"]
    g = _combined(env, case, 2)
    g.run(5.0, 30)
    assert np.array_equal(g.excluded() != 0, g.cell_source() == 1)
    # peel what came in: ctx's original entries are back, in the order of the sort (the synthetic order)
    g.restage(keep=g.cell_source() == 0)
    d = g.dims()
    assert (d.total_cells, d.total_loci) == (N0, LOUT)
    _same_arrays(g.staged_coo(), case["dst"], "ctx's own entries")
    assert not g.cell_source().any() and np.array_equal(g.cell_origin(), np.arange(N0))
    # a second combine, another keep: the twin again, the new cells' source is 2
    s = _make(env)
    s.ingest_coo(LS, NS, *case["src"])
    keep2 = np.random.default_rng(8).random(NS) < 0.1
    first = env["combine"].combine_coo(case["dst"], N0, case["src"], NS, case["keep"], case["lmap"], LOUT, 0.2, 4)
    g.ingest_coo(L0, N0, *case["dst"])
    g.combine(s, case["keep"], case["lmap"], LOUT, 0.2, 4)
    want = _combine_and_check(env, g, s, LOUT, first[4], first[:4], NS, case["src"], keep2, case["lmap"], LOUT, 0.0,
                              dst_origin=first[5], dst_source=first[6], k=2)
    n2 = int(keep2.sum())
    assert want[6].tolist() == [0] * N0 + [1] * 66 + [2] * n2
    # a restage composes source and origin alike
    pick = np.arange(want[4]) % 2 == 0
    g.restage(keep=pick)
    assert np.array_equal(g.cell_source(), want[6][pick]) and np.array_equal(g.cell_origin(), want[5][pick])
    # src restaged first: the new cells' origin is src's origin
    half = np.arange(NS) % 2 == 1
    s.restage(keep=half)
    g.ingest_coo(L0, N0, *case["dst"])
    g.combine(s, locus_map=case["lmap"], total_loci=LOUT)
    assert np.array_equal(g.cell_origin(), np.concatenate([np.arange(N0), np.flatnonzero(half)]))
    assert np.array_equal(g.cell_source(), np.concatenate([np.zeros(N0), np.ones(int(half.sum()))]))
    g.load_coo(L0, N0, *case["dst"])  # an ingest from outside: all 0 again, and 255 combines to go
    assert not g.cell_source().any()
    g.close(); s.close()


def test_a_loaded_src_iterates_as_before(env, case):
    s, f, g = _make(env), _make(env), _make(env)
    for x in (s, f):
        x.load_coo(LS, NS, *case["src"])
    a0, b0 = s.em_iteration(5.0), f.em_iteration(5.0)
    g.ingest_coo(L0, N0, *case["dst"])
    g.combine(s, case["keep"], case["lmap"], LOUT, 0.2, 4)
    _same_arrays(g.staged_coo(), case["twin"][:4])
    a1, b1 = s.em_iteration(5.0), f.em_iteration(5.0)
    for a, b in ((a0, b0), (a1, b1)):
        _same_bits(tuple(getattr(a, k) for k, _ in a._fields_), tuple(getattr(b, k) for k, _ in b._fields_))
    _same_bits(s.cell_outputs(), f.cell_outputs())
    _same_bits(s.locus_outputs(), f.locus_outputs())
    assert np.array_equal(s.excluded(), f.excluded())
    _same_arrays(s.staged_coo(), case["src"])
    for x in (s, f, g):
        x.close()


# ---- 5. refusals: both ctxs unchanged -----------------------------------------------------------------------------------------------
def _state(x):
    d = x.dims()
    return (d.total_cells, d.total_loci, d.loci_used, d.nnz_used), x.staged_coo()


def _unchanged(x, before):
    now = _state(x)
    assert now[0] == before[0]
    _same_arrays(now[1], before[1])


def test_refusals_leave_both_ctxs_unchanged(env, case):
    dst, src, lmap, keep = case["dst"], case["src"], case["lmap"], case["keep"]
    g, s = _make(env), _make(env)
    g.load_coo(L0, N0, *dst)
    s.load_coo(LS, NS, *src)
    sg0, ss0 = g.em_iteration(5.0), s.em_iteration(5.0)
    bg, bs = _state(g), _state(s)
    bad_map = lmap.copy()
    bad_map[[700, 900]] = LOUT, LOUT + 5
    calls = [
        (dict(src=g), "same"),
        (dict(src=s, downsample_rate=1.5, locus_map=lmap), "downsample_rate"),
        (dict(src=s, downsample_rate=-0.25, locus_map=lmap), "downsample_rate"),
        (dict(src=s, downsample_rate=float("nan"), locus_map=lmap), "downsample_rate"),
        (dict(src=s, keep=np.zeros(NS, bool), locus_map=lmap), "none"),
        (dict(src=s, locus_map=lmap % 1400, total_loci=L0 - 1), "total_loci_out"),
        (dict(src=s, locus_map=lmap, total_loci=2 ** 32), "32-bit"),
        (dict(src=s, locus_map=bad_map, total_loci=LOUT), "locus_map[700]"),
    ]
    for kw, word in calls:
        assert word in _einval(env, g.combine, **kw), kw
    # a NULL map with src's total_loci above total_loci_out: the other way round (s has 1400 loci, g 1500)
    assert "locus_map" in _einval(env, s.combine, g, total_loci=LS)
    # an iteration in flight, on either side
    g.em_begin()
    assert "em_begin" in _einval(env, g.combine, s, keep, lmap, LOUT)
    assert "em_begin" in _einval(env, s.combine, g)
    g.em_threshold(5.0)
    _einval(env, g.combine, s, keep, lmap, LOUT)
    sg1 = g.em_finish()
    ss1 = s.em_iteration(5.0)
    _unchanged(g, bg); _unchanged(s, bs)
    # ... and both are the runs they would have been
    for x, coo, tl, n, first, second in ((g, dst, L0, N0, sg0, sg1), (s, src, LS, NS, ss0, ss1)):
        f = _make(env)
        f.load_coo(tl, n, *coo)
        for mine in (first, second):
            theirs = f.em_iteration(5.0)
            _same_bits(tuple(getattr(mine, k) for k, _ in mine._fields_), tuple(getattr(theirs, k) for k, _ in theirs._fields_))
        assert np.array_equal(x.excluded(), f.excluded())
        f.close()

    # a ctx that cannot take part, on either side
    e = _make(env)  # state EMPTY
    assert "staged" in _einval(env, g.combine, e) and "staged" in _einval(env, e.combine, g)
    e.close()
    m = _make(env, devices=[0, 0])
    m.load_coo(L0, N0, *dst)
    assert "multi-device" in _einval(env, g.combine, m) and "multi-device" in _einval(env, m.combine, g)
    assert m.dims().total_cells == N0
    m.close()
    h = _make(env)
    h.set_shard(0, 400)
    h.ingest_coo(L0, N0, *dst)
    assert "set_shard" in _einval(env, g.combine, h) and "set_shard" in _einval(env, h.combine, g)
    h.close()
    k = _make(env, keep_coo=0)
    k.load_coo(LS, NS, *src)
    assert "keep_coo" in _einval(env, g.combine, k) and "keep_coo" in _einval(env, k.combine, g)
    sk = k.em_iteration(5.0)
    _same_bits(tuple(getattr(sk, f) for f, _ in sk._fields_), tuple(getattr(ss0, f) for f, _ in ss0._fields_))
    k.close()
    _unchanged(g, bg); _unchanged(s, bs)
    g.close(); s.close()


def _summary(s):
    return tuple(getattr(s, k) for k, _ in s._fields_)


def test_a_ctx_with_a_communicator_is_refused_on_either_side(env, case):
    """a one-rank communicator (the RCCL self-test of tests/test_gpu_em_state.py) makes the ctx one whose ranks stage their own cells"""
    import os
    dst, src = case["dst"], case["src"]

    def with_communicator():
        os.environ["CELLECTOR_COMM_SELFTEST"] = "1"
        try:
            x = _make(env)
            x.comm_init_rank(env["ffi"].comm_unique_id(), 1, 0)
        finally:
            os.environ.pop("CELLECTOR_COMM_SELFTEST", None)
        x.load_coo(LS, NS, *src)
        return x

    m, h = with_communicator(), with_communicator()
    g, f = _make(env), _make(env)
    g.load_coo(L0, N0, *dst)
    f.load_coo(L0, N0, *dst)
    sm0, sg0 = m.em_iteration(5.0), g.em_iteration(5.0)
    bm, bg = _state(m), _state(g)
    assert "src" in (msg := _einval(env, g.combine, m, case["keep"], case["lmap"], LOUT)) and "communicator" in msg
    assert "ctx" in (msg := _einval(env, m.combine, g)) and "communicator" in msg
    _unchanged(m, bm); _unchanged(g, bg)
    # one more iteration of both: the runs they would have been (h, f: the same ctxs without the refused calls)
    assert _summary(h.em_iteration(5.0)) == _summary(sm0) and _summary(f.em_iteration(5.0)) == _summary(sg0)
    sm1, sg1 = m.em_iteration(5.0), g.em_iteration(5.0)
    _same_bits(_summary(sm1), _summary(h.em_iteration(5.0)))
    _same_bits(_summary(sg1), _summary(f.em_iteration(5.0)))
    assert np.array_equal(m.excluded(), h.excluded()) and np.array_equal(g.excluded(), f.excluded())
    for x in (m, g, f, h):
        x.close()


def test_ctxs_on_different_devices_are_refused(env, case):
    if env["ffi"].device_count() < 2:
        pytest.skip("needs two GPUs: the refusal of ctxs on different devices cannot be reached on one")
    g, o = _make(env), env["Cellector"](1)
    g.ingest_coo(L0, N0, *case["dst"])
    o.ingest_coo(LS, NS, *case["src"])
    bg, bo = _state(g), _state(o)
    assert "device" in _einval(env, g.combine, o) and "device" in _einval(env, o.combine, g, total_loci=L0)
    _unchanged(g, bg); _unchanged(o, bo)
    g.close(); o.close()


def test_refusals_by_the_counts(env):
    one = [np.zeros(1, np.uint32)] * 2 + [np.ones(1, np.uint32)] * 2
    s = _make(env)
    s.ingest_coo(1, 1, *one)
    # n_ctx + n_kept above 2^32 - 1: a ctx of 2^32 - 1 cells without entries costs nothing while STAGED
    g = _make(env)
    none = [np.zeros(0, np.uint32)] * 4
    g.ingest_coo(1, 2 ** 32 - 1, *none)
    assert "cells" in _einval(env, g.combine, s)
    assert g.dims().total_cells == 2 ** 32 - 1 and len(g.staged_coo()[0]) == 0
    # 255 combines since the last ingest from outside, the next one is refused
    g.ingest_coo(1, 1, *one)
    for k in range(255):
        g.combine(s)
    assert g.dims().total_cells == 256 and np.array_equal(g.cell_source(), np.arange(256))
    before = _state(g)
    assert "255" in _einval(env, g.combine, s)
    _unchanged(g, before)
    _same_arrays(g.staged_coo(), [np.zeros(256, np.uint32), np.arange(256, dtype=np.uint32), np.ones(256, np.uint32), np.ones(256, np.uint32)])
    _same_arrays(s.staged_coo(), one)
    g.ingest_coo(1, 1, *one)  # the counter starts again
    g.combine(s)
    assert g.cell_source().tolist() == [0, 1]
    g.close()

    # a caller-bound PASS1 buffer: the size it was bound with counts, whatever the last ingest used of it
    import torch
    big = torch.zeros(5 * 6, dtype=torch.float64, device="cuda:0")
    g = _make(env)
    g.bind_exchange_buffer(env["ffi"].XCHG_PASS1, big.data_ptr(), big.numel())
    four = [np.arange(4, dtype=np.uint32), np.zeros(4, np.uint32), np.ones(4, np.uint32), np.ones(4, np.uint32)]
    g.ingest_coo(4, 1, *four)
    before = _state(g)
    assert "PASS1" in _einval(env, g.combine, s, total_loci=7)  # 35 values
    _unchanged(g, before)
    g.combine(s, total_loci=6)  # 30: the buffer holds it
    torch.cuda.synchronize()
    p1 = big.cpu().numpy().reshape(5, 6)
    assert p1[4].tolist() == [2, 1, 1, 1, 0, 0] and p1[3].tolist() == [2, 1, 1, 1, 0, 0]
    assert g.dims().total_loci == 6
    g.ingest_coo(5, 1, *four)  # ... and a reload with more loci than the first ingest had
    assert g.dims().total_loci == 5
    g.close()
    buf = torch.zeros(5 * 4, dtype=torch.float64, device="cuda:0")
    g = _make(env)
    g.bind_exchange_buffer(env["ffi"].XCHG_PASS1, buf.data_ptr(), buf.numel())
    g.ingest_coo(4, 1, *four)
    before = _state(g)
    assert "PASS1" in _einval(env, g.combine, s, total_loci=5)
    _unchanged(g, before)
    g.combine(s, total_loci=4)
    torch.cuda.synchronize()
    p1 = buf.cpu().numpy().reshape(5, 4)
    assert p1[4].tolist() == [2, 1, 1, 1] and p1[3].tolist() == [2, 1, 1, 1]  # entries and alt sums per locus, both sides
    g.close(); s.close()
