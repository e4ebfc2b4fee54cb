"""GPU: the joined ingests (cellector_ingest_coo_joined / _mtx_joined / cellector_load_mtx_joined, csrc/kernels_join.hip).

1. The kernels against the numpy twin (cellector_amd/join.py): staged_coo() and the summary are equal exactly, on hand-built streams
   whose lengths lie around T = join_tile as the summary reports it — (n_first, n_second) from {0, 1, T - 1, T, T + 1, 3 T + 5} —
   laid out so that the tile edges are met in every way: all keys matched, none, alternating, a run of one stream longer than 2 T
   inside matched keys (and its mirror image), a matched key on every cross-diagonal cut, the last key matched / unmatched; keys that
   differ only in the locus, only in the cell, and keys spread over 70 000 x 70 000 up to (total - 1, total - 1).  Both modes; either
   side shuffled: the summary then says that the sort ran and the entries are those of the ascending case.
2. Every refusal names the smallest offender and leaves the ctx as a failed cellector_ingest_mtx does; an EM loop on another ctx keeps
   its bits across the failed calls.
3. The text route on files of a few hundred lines: option parse_window at its smallest (both files windowed), both modes, CRLF and an
   unterminated last line in SECOND.
4. load_mtx_joined + run() on a planted 1500 x 700 matrix, both engines: the iteration summaries and assignments of load_mtx of the
   completed pair, bit for bit."""
import os

import numpy as np
import pytest

import mtx_text_reference as mt

pytestmark = pytest.mark.gpu

EINVAL, EPARSE = 1, 3
TOTAL = 70000  # total_loci = total_cells of the hand-built streams


@pytest.fixture(scope="module")
def mods(hip_lib_path):
    from cellector_amd import Cellector, ffi, join, synth
    return dict(Cellector=Cellector, ffi=ffi, join=join, synth=synth)


@pytest.fixture(scope="module")
def ctx(mods):
    g = mods["Cellector"](0)
    g.set_option("keep_coo", 1)
    yield g
    g.close()


@pytest.fixture(scope="module")
def tile(mods, ctx):
    one = (np.zeros(1, np.uint32),) * 3
    t = ctx.ingest_coo_joined(4, 4, one, one).join_tile
    assert t == mods["join"].TILE and t >= 64
    return t


# ---- 1. the kernels against the twin ----------------------------------------------------------------------------------------------
LAYOUTS = ("wide", "cell_only", "locus_only")


def keys_of(ranks, n_ranks, layout):
    """ascending ranks -> ascending (locus, cell) keys"""
    r = np.asarray(ranks, np.int64)
    if layout == "cell_only":  # one locus at 2^16, cells across 2^16
        return np.full(r.size, 65536, np.int64), 56000 + r
    if layout == "locus_only":  # one cell, the last one
        return 57000 + r, np.full(r.size, TOTAL - 1, np.int64)
    # wide: the flat index rank * stride over the whole 70 000 x 70 000 grid; the last rank is the last key of the matrix
    stride = (TOTAL * TOTAL - 1) // max(1, n_ranks - 1)
    flat = r * stride
    flat[r == n_ranks - 1] = TOTAL * TOTAL - 1
    return flat // TOTAL, flat % TOTAL


def on_every_cut(na, nb, t):
    """ranks of two streams whose merge (FIRST first among equals) has a matched pair exactly across every cross-diagonal cut d = k t
    (across the first min(na, nb) cuts where a stream is shorter than their number), and the cuts planted"""
    n = na + nb
    cuts = list(range(t, n, t))[:min(na, nb)]
    a_free, b_free = na - len(cuts), nb - len(cuts)  # the entries outside the planted pairs
    ra, rb, p, r, pending = [], [], 0, 0, list(cuts)
    while p < n:  # p: the step of the merge the next entry takes
        if pending and p == pending[0] - 1:
            ra.append(r); rb.append(r); p += 2; pending.pop(0)
        elif b_free and (p % 5 == 2 or not a_free):
            rb.append(r); p += 1; b_free -= 1
        else:
            ra.append(r); p += 1; a_free -= 1
        r += 1
    assert (a_free, b_free, pending) == (0, 0, [])
    return np.array(ra, np.int64), np.array(rb, np.int64), cuts


def shape(name, na, nb, t, rng):
    """(ranks of FIRST, ranks of SECOND) ascending, or None where the pair of lengths cannot form the shape"""
    if name == "all_matched":
        return (np.arange(na), np.arange(nb)) if na == nb else None
    if name == "none_matched":
        return np.arange(na), na + np.arange(nb)
    if name == "alternating":
        return 2 * np.arange(na), 2 * np.arange(nb) + 1
    if name in ("first_run", "second_run"):  # the longer stream holds every key; the other one its first 5 and its last ones
        x, y = (na, nb) if name == "first_run" else (nb, na)
        if y < 6 or x - y <= 2 * t:
            return None
        rx = np.arange(x)
        ry = np.concatenate([rx[:5], rx[x - (y - 5):]])
        return (rx, ry) if name == "first_run" else (ry, rx)
    if name == "cuts":
        if na != 3 * t + 5 or nb == 0:
            return None
        return on_every_cut(na, nb, t)[:2]
    if name in ("random_last_matched", "random_last_first", "random_last_second"):
        if na == 0 or nb == 0:
            return None
        pool = rng.permutation(na + nb)  # ranks 0 .. na + nb - 1, a random share of them in both streams
        both = int(rng.integers(0, min(na, nb) + 1))
        ra = np.sort(np.concatenate([pool[:both], pool[both:na]]))
        rb = np.sort(np.concatenate([pool[:both], pool[na:na + nb - both]]))
        top = na + nb + 1
        if name == "random_last_matched":
            ra[-1] = rb[-1] = top
        elif name == "random_last_first":
            ra[-1] = top
        else:
            rb[-1] = top
        return ra, rb
    raise AssertionError(name)


SHAPES = ("all_matched", "none_matched", "alternating", "first_run", "second_run", "cuts", "random_last_matched", "random_last_first",
          "random_last_second")


def counts_for(ra, rb, mode, join, rng):
    """counts of the two streams (explicit zeros among them); under DEPTH the second one is alt + ref and a key without a depth has alt 0"""
    n_ranks = int(max(ra.max(initial=-1), rb.max(initial=-1))) + 1
    alt = rng.integers(0, 4, n_ranks)
    ref = rng.integers(0, 4, n_ranks)
    if mode == join.MODE_REF:
        return alt[ra], ref[rb], n_ranks
    in_b = np.zeros(n_ranks, bool)
    in_b[rb] = True
    in_a = np.zeros(n_ranks, bool)
    in_a[ra] = True
    alt[~in_b] = 0
    return alt[ra], (np.where(in_a, alt, 0) + ref)[rb], n_ranks


def same(got, want, what):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and np.array_equal(a, b), (what, k)


def test_the_planted_cuts_are_where_the_kernel_cuts(tile):
    for nb in (1, tile - 1, tile, tile + 1, 3 * tile + 5):
        ra, rb, cuts = on_every_cut(3 * tile + 5, nb, tile)
        assert len(ra) == 3 * tile + 5 and len(rb) == nb and np.all(np.diff(ra) > 0) and np.all(np.diff(rb) > 0)
        assert len(cuts) == min(nb, (3 * tile + 5 + nb - 1) // tile) and cuts[0] == tile
        matched = np.intersect1d(ra, rb)
        assert len(matched) == len(cuts)
        for key, d in zip(matched, cuts):  # FIRST's entry of the pair is step d - 1 of the merge, SECOND's is step d
            assert int(np.searchsorted(ra, key)) + int(np.searchsorted(rb, key)) == d - 1, (nb, d)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", SHAPES)
def test_kernels_match_the_twin(mods, ctx, tile, name, layout):
    join = mods["join"]
    sizes = [0, 1, tile - 1, tile, tile + 1, 3 * tile + 5]
    rng = np.random.default_rng(100 * SHAPES.index(name) + LAYOUTS.index(layout))
    ran = 0
    for na in sizes:
        for nb in sizes:
            made = shape(name, na, nb, tile, rng)
            if made is None:
                continue
            ra, rb = made
            assert len(ra) == na and len(rb) == nb
            for mode in (join.MODE_REF, join.MODE_DEPTH):
                va, vb, n_ranks = counts_for(ra, rb, mode, join, rng)
                first = keys_of(ra, n_ranks, layout) + (va,)
                second = keys_of(rb, n_ranks, layout) + (vb,)
                want = join.join_coo(first, second, mode, TOTAL, TOTAL)
                assert want[4]["first_sorted"] == want[4]["second_sorted"] == 1 and want[4]["n_out"] == len(np.union1d(ra, rb))
                for shuffled in (None, 0, 1):
                    sides = [first, second]
                    if shuffled is not None:
                        if len(sides[shuffled][0]) < 2:
                            continue
                        p = rng.permutation(len(sides[shuffled][0]))
                        p = p[::-1] if np.all(np.diff(p) > 0) else p
                        sides[shuffled] = tuple(x[p] for x in sides[shuffled])
                    what = (name, layout, na, nb, mode, shuffled)
                    s = ctx.ingest_coo_joined(TOTAL, TOTAL, sides[0], sides[1], mode)
                    twin = join.join_coo(sides[0], sides[1], mode, TOTAL, TOTAL)
                    assert s.as_dict() == twin[4], what
                    if shuffled is not None:  # the sort ran on that side and only there; the entries are the ascending case's
                        assert (s.first_sorted, s.second_sorted) == ((0, 1) if shuffled == 0 else (1, 0)), what
                    same(ctx.staged_coo(), want[:4], what)
                    d = ctx.dims()
                    assert (d.total_loci, d.total_cells) == (TOTAL, TOTAL)
                    ran += 1
    assert ran >= (6 if name in ("first_run", "second_run") else 20), ran


def test_the_wide_layout_reaches_the_corners(tile):
    n = 3 * tile + 5
    l, c = keys_of(np.arange(n), n, "wide")
    assert (l[-1], c[-1]) == (TOTAL - 1, TOTAL - 1) and (l >= 65536).any() and (c >= 65536).any() and (l[1:] >= l[:-1]).all()
    k = l.astype(np.int64) << 32 | c
    assert np.all(k[1:] > k[:-1])


# ---- 2. refusals ----------------------------------------------------------------------------------------------------------------
def clean():
    """6000 keys in both streams, ascending (three tiles of the join), counts that satisfy either mode"""
    flat = np.arange(0, 60000, 10)
    return [flat // 30, flat % 30, np.full(6000, 3)], [flat // 30, flat % 30, np.full(6000, 7)]


def refused(mods, g, first, second, mode, twin=True, tl=2000, tc=30):
    with pytest.raises(mods["ffi"].CellectorError) as e:
        g.ingest_coo_joined(tl, tc, first, second, mode)
    assert e.value.status == EINVAL
    if twin:  # the twin refuses with the same words
        with pytest.raises(mods["join"].JoinError) as t:
            mods["join"].join_coo(first, second, mode, tl, tc)
        assert str(e.value) == "EINVAL: " + str(t.value)
    return str(e.value)


def left_empty(mods, g, tl=2000, tc=30):
    """as a failed cellector_ingest_mtx leaves a ctx: the former matrix gone, nothing staged, the new dims noted"""
    with pytest.raises(mods["ffi"].CellectorError, match="without a staged matrix"):
        g.staged_coo()
    with pytest.raises(mods["ffi"].CellectorError, match="without a staged matrix"):
        g.ingest_finish()
    assert (g.dims().total_loci, g.dims().total_cells) == (tl, tc)


def test_refusals_name_the_smallest_offender(mods):
    join = mods["join"]
    g = mods["Cellector"](0)
    for side in (0, 1):
        for kind, (col, value) in {join.KIND_LOCUS: (0, 2000), join.KIND_CELL: (1, 30), join.KIND_COUNT: (2, 65536)}.items():
            s = clean()
            s[side][col][400] = value
            s[side][2][5000] = 70000
            if side == 0:
                s[1][2][7] = 1 << 20  # (FIRST is checked first, SECOND only then)
            msg = refused(mods, g, s[0], s[1], join.MODE_REF)
            assert msg == f"EINVAL: join: {join.SIDES[side]} entry 400: {join.KINDS[kind]}", msg
            left_empty(mods, g)
        # a key listed twice: the smallest such key, not the first one met; the side is unsorted on the way
        s = clean()
        for src in (200, 50):
            for k in range(3):
                s[side][k] = np.append(s[side][k], s[side][k][src])
        msg = refused(mods, g, s[0], s[1], join.MODE_DEPTH)
        assert msg == f"EINVAL: join: {join.SIDES[side]} lists (locus {s[side][0][50] + 1}, cell {s[side][1][50] + 1}) twice", msg
        left_empty(mods, g)
    # depth below alt: the smallest key, in tiles far apart; an absent depth counts as 0
    first, second = clean()
    second[2][5800], second[2][31] = 2, 0
    msg = refused(mods, g, first, second, join.MODE_DEPTH)
    assert msg == f"EINVAL: join: depth below alt at (locus {first[0][31] + 1}, cell {first[1][31] + 1})", msg
    left_empty(mods, g)
    assert g.ingest_coo_joined(2000, 30, first, second, join.MODE_REF).n_both == 6000  # (fine as an alt / ref pair)
    first, second = clean()
    second = [x[np.arange(6000) != 77] for x in second]
    msg = refused(mods, g, first, second, join.MODE_DEPTH)
    assert f"(locus {first[0][77] + 1}, cell {first[1][77] + 1})" in msg
    # the documented order: entry checks before duplicates before depth
    first, second = clean()
    second[2][0] = 1
    second = [np.append(x, x[1]) for x in second]
    assert "SECOND lists" in refused(mods, g, first, second, join.MODE_DEPTH)
    first[1][5999] = 30
    assert "FIRST entry 5999: cell index out of range" in refused(mods, g, first, second, join.MODE_DEPTH)
    g.close()


def test_scope_and_argument_refusals_leave_the_ctx_untouched(mods):
    join, ffi = mods["join"], mods["ffi"]
    first, second = clean()
    g = mods["Cellector"](0)
    g.ingest_coo_joined(2000, 30, first, second, join.MODE_REF)
    before = g.staged_coo()
    assert "mode must be" in refused(mods, g, first, second, 3, twin=False)
    lib = ffi.load_library()
    a = np.zeros(4, np.uint32)
    p = a.ctypes.data_as(ffi.C.c_void_p)
    assert lib.cellector_ingest_coo_joined(g.h, 2000, 30, 4, p, p, None, 0, None, None, None, 1, None) == EINVAL
    assert b"null COO array" in lib.cellector_last_error(g.h)
    same(g.staged_coo(), before, "after refused arguments")
    g.close()
    g = mods["Cellector"](0)
    g.set_shard(0, 10)
    assert "cellector_set_shard range" in refused(mods, g, first, second, join.MODE_REF, twin=False)
    g.close()
    g = mods["Cellector"](devices=[0, 0])
    assert "multi-device ctx" in refused(mods, g, first, second, join.MODE_REF, twin=False)
    with pytest.raises(ffi.CellectorError, match="multi-device ctx"):
        g.ingest_mtx_joined("a.mtx", "b.mtx", "depth")
    g.close()


def test_a_loop_on_another_ctx_keeps_its_bits_across_failed_joins(mods):
    join, synth = mods["join"], mods["synth"]
    L, N = 600, 500
    coo = synth.generate_coo(L, N, 0.2, seed=4, minority_fraction=0.08)
    x, y, z = (mods["Cellector"](0) for _ in range(3))
    x.load_coo(L, N, *coo)
    y.load_coo(L, N, *coo)
    want = x.run(5.0, 40)
    assert len(want) >= 2 and not want[-1].any_change
    want.append(x.em_iteration(5.0))
    got = []
    for it in range(len(want)):
        got.append(y.em_iteration(5.0))
        if it == 1:
            first, second = clean()
            second[2][31] = 0
            refused(mods, z, first, second, join.MODE_DEPTH)
            first[0][5] = 2000
            refused(mods, z, first, second, join.MODE_REF)
    assert [bytes(s) for s in got] == [bytes(s) for s in want]
    assert np.array_equal(x.excluded(), y.excluded())
    for k, v in x.cell_outputs().items():
        assert v.tobytes() == y.cell_outputs()[k].tobytes(), k
    for g in (x, y, z):
        g.close()


# ---- 3. the text route ------------------------------------------------------------------------------------------------------------
TL, TC = 90, 70


def text_streams(mode, join, seed):
    """two streams of a few hundred lines over random keys, FIRST in file order of a shuffled tool, SECOND ascending"""
    rng = np.random.default_rng(seed)
    flat = np.sort(rng.choice(TL * TC, 500, replace=False))
    in_a, in_b = rng.random(500) < 0.7, rng.random(500) < 0.7
    in_b |= ~in_a
    alt, ref = rng.integers(0, 300, 500), rng.integers(0, 300, 500)
    alt[rng.random(500) < 0.1] = 0
    if mode == join.MODE_DEPTH:
        alt[~in_b] = 0
    second = ref if mode == join.MODE_REF else np.where(in_a, alt, 0) + ref
    p = rng.permutation(int(in_a.sum()))
    first = tuple(x[in_a][p] for x in (flat // TC, flat % TC, alt))
    return first, tuple(x[in_b] for x in (flat // TC, flat % TC, second))


def write_stream(path, t, seed, style="mix", terminated=True, crlf=False):
    entries = [(int(l), int(c), int(v), 0) for l, c, v in zip(*t)]
    lines, _ = mt.build_sections(entries, [None] * len(entries), seed, style=style, terminated=terminated)
    if crlf:
        lines = [x[:-1] + b"\r\n" if x.endswith(b"\n") and not x.endswith(b"\r\n") else x for x in lines]
    with open(path, "wb") as f:
        f.write(mt.mtx_file(TL, TC, b"".join(lines), nnz=len(entries)))
    return len(b"".join(lines))


@pytest.mark.parametrize("mode_name", ["ref", "depth"])
@pytest.mark.parametrize("window", [0, 1])
def test_text_route(mods, tmp_path, mode_name, window):
    join = mods["join"]
    mode = join.MODE_REF if mode_name == "ref" else join.MODE_DEPTH
    first, second = text_streams(mode, join, seed=mode + 10 * window)
    a, b = str(tmp_path / "first.mtx"), str(tmp_path / "second.mtx")
    na = write_stream(a, first, 1)
    nb = write_stream(b, second, 2, style="blanks", terminated=False, crlf=True)
    assert open(b, "rb").read().count(b"\r\n") >= 300 and not open(b, "rb").read().endswith(b"\n")
    want = join.join_coo(first, second, mode, TL, TC)
    g = mods["Cellector"](0)
    if window:
        g.set_option("parse_window", 1)  # (the smallest window the library takes: 512 bytes; both files are many windows long)
        assert min(na, nb) > 4 * 512
    s = g.ingest_mtx_joined(a, b, mode_name)
    assert s.as_dict() == want[4] and s.first_sorted == 0 and s.second_sorted == 1
    same(g.staged_coo(), want[:4], (mode_name, window))
    assert (g.dims().total_loci, g.dims().total_cells) == (TL, TC)
    # refusals of the text route: a line that does not parse, FIRST before SECOND, before any range error; index 0; size lines
    raw_a, raw_b = open(a, "rb").read(), open(b, "rb").read()
    head_a, sec_a = raw_a.split(b"\n", 3)[:3], raw_a.split(b"\n", 3)[3]
    la = sec_a.split(b"\n")
    bad_b = str(tmp_path / "bad_second.mtx")
    lb = raw_b.split(b"\n")
    lb[3 + 40] = b"7 x 1\r"
    open(bad_b, "wb").write(b"\n".join(lb))
    with pytest.raises(mods["ffi"].CellectorError) as e:
        g.ingest_mtx_joined(a, bad_b, mode_name)
    assert e.value.status == EPARSE and "SECOND file: cannot parse mtx entry 40 (line 41 of the data section)" in str(e.value)
    bad_a = str(tmp_path / "bad_first.mtx")
    la2 = list(la)
    la2[100], la2[3] = b"1 2", b"%d 1 1" % (TL + 1)
    open(bad_a, "wb").write(b"\n".join(head_a + la2))
    with pytest.raises(mods["ffi"].CellectorError) as e:
        g.ingest_mtx_joined(bad_a, bad_b, mode_name)
    assert e.value.status == EPARSE and "FIRST file: cannot parse mtx entry 100 " in str(e.value)
    la2[100] = la[100]
    la2[200] = b"0 5 1"
    open(bad_a, "wb").write(b"\n".join(head_a + la2))
    with pytest.raises(mods["ffi"].CellectorError) as e:
        g.ingest_mtx_joined(bad_a, b, mode_name)
    assert e.value.status == EINVAL and str(e.value) == "EINVAL: join: FIRST entry 3: locus index out of range"
    la2[3] = la[3]
    open(bad_a, "wb").write(b"\n".join(head_a + la2))
    with pytest.raises(mods["ffi"].CellectorError) as e:
        g.ingest_mtx_joined(bad_a, b, mode_name)
    assert str(e.value) == "EINVAL: join: FIRST entry 200: index 0 (indices are 1-based)"
    left_empty(mods, g, TL, TC)
    s = g.ingest_mtx_joined(a, b, mode_name)  # (and the ctx takes the good pair again)
    same(g.staged_coo(), want[:4], "again")
    open(bad_a, "wb").write(b"\n".join([head_a[0], head_a[1], b"%d %d 5" % (TL, TC + 1)] + la))
    with pytest.raises(mods["ffi"].CellectorError, match="size lines disagree") as e:
        g.ingest_mtx_joined(bad_a, b, mode_name)
    assert e.value.status == EINVAL
    same(g.staged_coo(), want[:4], "a refusal before the ingest began")
    g.close()


# ---- 4. the loop on a joined load ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted(mods, tmp_path_factory):
    """1500 loci x 700 cells with a planted minority, written three ways: the completed aligned pair, an alt / ref pair with each
    file's zero lines dropped and the ref file shuffled, an AD / DP pair"""
    join, synth = mods["join"], mods["synth"]
    L, N = 1500, 700
    l, c, a, r = synth.generate_coo(L, N, 0.1, seed=4, minority_fraction=0.08)
    tmp = str(tmp_path_factory.mktemp("join_planted"))
    rng = np.random.default_rng(2)

    def write(path, idx, vals):
        body = np.stack([l[idx].astype(np.int64) + 1, c[idx].astype(np.int64) + 1, vals[idx].astype(np.int64)], 1)
        with open(path, "w") as f:
            f.write("%%MatrixMarket matrix coordinate integer general\n%\n" + f"{L} {N} {len(idx)}\n")
            np.savetxt(f, body, fmt="%d")
        return path
    nz_a, nz_r, nz_d = np.flatnonzero(a), rng.permutation(np.flatnonzero(r)), np.flatnonzero(a + r)
    first = (l[nz_a], c[nz_a], a[nz_a])
    pair = join.join_coo(first, (l[nz_r], c[nz_r], r[nz_r]), join.MODE_REF, L, N)
    depth = join.join_coo(first, (l[nz_d], c[nz_d], (a + r)[nz_d]), join.MODE_DEPTH, L, N)
    same(pair[:4], depth[:4], "the two ways to write the matrix")
    aligned = synth.write_mtx_pair(os.path.join(tmp, "aligned"), L, N, *pair[:4])
    return dict(L=L, N=N, aligned=aligned, n_out=pair[4]["n_out"],
                ref=(write(os.path.join(tmp, "alt.mtx"), nz_a, a), write(os.path.join(tmp, "ref.mtx"), nz_r, r), "ref"),
                depth=(write(os.path.join(tmp, "ad.mtx"), nz_a, a), write(os.path.join(tmp, "dp.mtx"), nz_d, a + r), "depth"))


@pytest.mark.parametrize("engine", [1, 2])
@pytest.mark.parametrize("which", ["ref", "depth"])
def test_joined_load_runs_like_the_completed_pair(mods, planted, which, engine):
    def run(load):
        g = mods["Cellector"](0)
        g.set_option("engine", engine)
        load(g)
        d = g.dims()
        summaries = g.run(5.0, 40)
        out = ((d.total_loci, d.total_cells, d.loci_used, d.nnz_used), [bytes(s) for s in summaries], g.excluded(), g.cell_outputs(),
               g.posteriors(), g.entries_per_cell(), g.staged_coo())
        g.close()
        return out
    want = run(lambda g: g.load_mtx(*planted["aligned"]))
    first, second, mode = planted[which]
    got = run(lambda g: g.load_mtx_joined(first, second, mode))
    assert got[0] == want[0] and got[0][2] > 100 and len(want[1]) >= 2
    assert got[1] == want[1]
    assert np.array_equal(got[2], want[2]) and want[2].sum() > 10
    for a, b in ((got[3], want[3]), (got[4], want[4])):
        assert sorted(a) == sorted(b)
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
    assert np.array_equal(got[5], want[5])
    same(got[6], want[6], "staged entries")
    assert len(got[6][0]) == planted["n_out"]
