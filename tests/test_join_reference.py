"""cellector_amd/join.py, the numpy twin of the joined ingests, against a dict-based restatement of the contract in
include/cellector_ffi.h: the join itself, the completed-pair statement, every refusal's smallest offender and their order."""
import numpy as np
import pytest

from cellector_amd import join
import mtx_text_reference as mt

TL, TC = 40, 30


def restate(first, second, mode):
    """the contract in ten lines: one entry per key of either stream, ascending; a missing count is 0"""
    a = {(int(l), int(c)): int(v) for l, c, v in zip(*first)}
    b = {(int(l), int(c)): int(v) for l, c, v in zip(*second)}
    out = []
    for k in sorted(set(a) | set(b)):
        alt, other = a.get(k, 0), b.get(k, 0)
        out.append(k + (alt, other if mode == join.MODE_REF else other - alt))
    counts = dict(n_first=len(a), n_second=len(b), n_both=len(set(a) & set(b)), n_first_only=len(set(a) - set(b)),
                  n_second_only=len(set(b) - set(a)), n_out=len(out))
    return np.array(out, np.int64).reshape(-1, 4), counts


def ascending(t):
    k = np.asarray(t[0], np.int64) << 32 | np.asarray(t[1], np.int64)
    return int(k.size < 2 or bool(np.all(k[1:] > k[:-1])))


def streams(rng, n_keys, p_first, p_second, mode, zeros=0.2, shuffle=(False, False)):
    """two streams over n_keys random keys: a key is in FIRST / SECOND with the given probabilities (never in neither); explicit
    zeros; in mode DEPTH the second count is alt + ref"""
    flat = rng.choice(TL * TC, size=n_keys, replace=False)
    flat.sort()
    in_a, in_b = rng.random(n_keys) < p_first, rng.random(n_keys) < p_second
    in_a |= ~in_b & (rng.random(n_keys) < 0.5)
    in_b |= ~in_a
    alt = np.where(rng.random(n_keys) < zeros, 0, rng.integers(0, 300, n_keys))
    ref = np.where(rng.random(n_keys) < zeros, 0, rng.integers(0, 300, n_keys))
    alt[~in_a] = 0
    second = ref if mode == join.MODE_REF else alt + np.where(in_b, ref, 0)
    if mode == join.MODE_DEPTH:
        alt[~in_b] = 0  # (a key without a depth line has depth 0: only alt 0 is consistent)
    out = []
    for keep, v, sh in ((in_a, alt, shuffle[0]), (in_b, second, shuffle[1])):
        l, c, v = flat[keep] // TC, flat[keep] % TC, v[keep]
        if sh:
            p = rng.permutation(l.size)
            l, c, v = l[p], c[p], v[p]
        out.append((l, c, v))
    return out


CASES = {
    "mixed": dict(n_keys=300, p_first=0.7, p_second=0.7),
    "all_matched": dict(n_keys=200, p_first=1.0, p_second=1.0),
    "none_matched": dict(n_keys=200, p_first=0.5, p_second=0.0),
    "all_zeros": dict(n_keys=100, p_first=0.8, p_second=0.8, zeros=1.0),
}


@pytest.mark.parametrize("mode", [join.MODE_REF, join.MODE_DEPTH])
@pytest.mark.parametrize("shuffle", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("case", sorted(CASES))
def test_join_matches_the_restatement(case, shuffle, mode):
    rng = np.random.default_rng(sorted(CASES).index(case) * 16 + shuffle[0] * 2 + shuffle[1] + mode * 4)
    first, second = streams(rng, mode=mode, shuffle=shuffle, **CASES[case])
    if case == "none_matched":
        assert not set(zip(*first[:2])) & set(zip(*second[:2]))
    want, counts = restate(first, second, mode)
    l, c, a, r, s = join.join_coo(first, second, mode, TL, TC)
    assert all(x.dtype == np.uint32 for x in (l, c, a, r))
    assert np.array_equal(np.stack([l, c, a, r], 1).astype(np.int64).reshape(-1, 4), want)
    assert {k: s[k] for k in counts} == counts
    assert (s["first_sorted"], s["second_sorted"]) == (ascending(first), ascending(second)) and s["join_tile"] == join.TILE
    if case == "all_matched":
        assert s["n_both"] == s["n_out"] == s["n_first"]
    if case == "none_matched":
        assert s["n_both"] == 0


@pytest.mark.parametrize("mode", [join.MODE_REF, join.MODE_DEPTH])
def test_empty_sides(mode):
    rng = np.random.default_rng(5)
    first, _ = streams(rng, 50, 1.0, 1.0, join.MODE_REF)
    none = (np.zeros(0, np.uint32),) * 3
    first = (first[0], first[1], first[2] * 0) if mode == join.MODE_DEPTH else first  # (FIRST alone under DEPTH: only alt 0 has depth 0)
    for a, b in ((first, none), (none, first), (none, none)):
        want, counts = restate(a, b, mode)
        l, c, alt, ref, s = join.join_coo(a, b, mode, TL, TC)
        assert np.array_equal(np.stack([l, c, alt, ref], 1).astype(np.int64).reshape(-1, 4), want)
        assert {k: s[k] for k in counts} == counts and s["first_sorted"] == s["second_sorted"] == 1


@pytest.mark.parametrize("mode", [join.MODE_REF, join.MODE_DEPTH])
def test_completed_pair_read_by_the_aligned_reader_is_the_join(mode):
    """both files rewritten over the union of keys, ascending, explicit zeros: the aligned text contract reads the join"""
    rng = np.random.default_rng(11 + mode)
    first, second = streams(rng, 250, 0.6, 0.7, mode, shuffle=(True, True))
    l, c, a, r, _ = join.join_coo(first, second, mode, TL, TC)
    entries = [tuple(int(x) for x in e) for e in zip(l, c, a, r)]
    alt_lines, ref_lines = mt.build_sections(entries, [None] * len(entries), seed=3)
    m = mt.read_pair(mt.mtx_file(TL, TC, b"".join(alt_lines)), mt.mtx_file(TL, TC, b"".join(ref_lines)))
    assert isinstance(m, mt.Matrix) and (m.total_loci, m.total_cells) == (TL, TC)
    assert m.entries == entries
    # ... and the 1-based form of the same streams (what the text route hands the join) gives the same entries
    one = [tuple(np.asarray(x) + (1 if k < 2 else 0) for k, x in enumerate(t)) for t in (first, second)]
    l1, c1, a1, r1, _ = join.join_coo(one[0], one[1], mode, TL, TC, one_based=True)
    assert [tuple(int(x) for x in e) for e in zip(l1, c1, a1, r1)] == entries


def _clean(mode=join.MODE_REF):
    """sorted FIRST and SECOND over the same 60 keys, counts that satisfy either mode"""
    flat = np.arange(0, 600, 10)
    l, c = flat // TC, flat % TC
    return [l.copy(), c.copy(), np.full(60, 3)], [l.copy(), c.copy(), np.full(60, 7)]


def _refused(first, second, mode=join.MODE_REF, **kw):
    with pytest.raises(join.JoinError) as e:
        join.join_coo(first, second, mode, TL, TC, **kw)
    assert e.value.status == join.EINVAL and str(e.value) == e.value.message
    return e.value


@pytest.mark.parametrize("side", [0, 1])
def test_entry_refusals_name_the_smallest_entry_with_its_own_kind(side):
    for kind, (col, value) in {join.KIND_LOCUS: (0, TL), join.KIND_CELL: (1, TC), join.KIND_COUNT: (2, 65536)}.items():
        s = _clean()
        s[side][col][40] = value
        s[side][2][50] = 70000  # (a later offender of another kind does not matter)
        e = _refused(*s)
        assert (e.what, e.side, e.entry, e.kind) == ("entry", side, 40, kind)
        assert str(e) == f"join: {join.SIDES[side]} entry 40: {join.KINDS[kind]}"
    # one entry with several faults: the order of the aligned reader's kinds
    s = _clean()
    s[side][0][7], s[side][1][7], s[side][2][7] = TL + 3, TC, 1 << 20
    assert _refused(*s).kind == join.KIND_LOCUS
    s[side][0][7] = 0
    assert _refused(*s).kind == join.KIND_CELL
    # 1-based streams: index 0 comes first, and TL itself is in range
    s = [[x + 1, y + 1, v] for x, y, v in _clean()]
    s[side][0][9] = TL
    join.join_coo(s[0], s[1], join.MODE_REF, TL, TC, one_based=True)
    s[side][1][9] = 0
    e = _refused(*s, one_based=True)
    assert (e.entry, e.kind) == (9, join.KIND_INDEX0) and "index 0" in str(e)
    assert 65535 == join.MAX_COUNT and join.join_coo(*_clean(), join.MODE_REF, TL, TC)[4]["n_out"] == 60


@pytest.mark.parametrize("side", [0, 1])
def test_duplicate_refusal_names_the_smallest_key(side):
    s = _clean()
    # key 20 -> listed again at the end; key 5 -> listed again in the middle: the smallest duplicated KEY wins, not the first met
    for src in (20, 5):
        for k in range(3):
            s[side][k] = np.append(s[side][k], s[side][k][src])
    e = _refused(*s)
    assert (e.what, e.side, e.locus, e.cell) == ("duplicate", side, int(s[side][0][5]), int(s[side][1][5]))
    assert str(e) == f"join: {join.SIDES[side]} lists (locus {e.locus + 1}, cell {e.cell + 1}) twice"
    # the same key in FIRST and in SECOND is the join's business, not a duplicate
    join.join_coo(*_clean(), join.MODE_REF, TL, TC)


def test_depth_refusal_names_the_smallest_key():
    first, second = _clean()
    second[2][30], second[2][12] = 2, 0  # depth 2 and 0 under alt 3
    e = _refused(first, second, join.MODE_DEPTH)
    assert (e.what, e.locus, e.cell) == ("depth", int(first[0][12]), int(first[1][12]))
    assert str(e) == f"join: depth below alt at (locus {e.locus + 1}, cell {e.cell + 1})"
    join.join_coo(first, second, join.MODE_REF, TL, TC)  # (the same streams are fine as alt / ref)
    # a FIRST key without a depth line has depth 0
    first, second = _clean()
    second = [x[np.arange(60) != 4] for x in second]
    e = _refused(first, second, join.MODE_DEPTH)
    assert (e.locus, e.cell) == (int(first[0][4]), int(first[1][4]))
    first[2][4] = 0
    l, c, a, r, s = join.join_coo(first, second, join.MODE_DEPTH, TL, TC)
    assert (int(a[4]), int(r[4])) == (0, 0) and s["n_first_only"] == 1 and np.all(r[np.arange(60) != 4] == 4)


def test_the_documented_order_decides_among_several_errors():
    def faulty(entry_first=False, entry_second=False, dup_first=False, dup_second=False, depth=False):
        first, second = _clean()
        if depth:
            second[2][0] = 1  # (the smallest key of all: still the last refusal)
        if dup_second:
            second = [np.append(x, x[1]) for x in second]
        if dup_first:
            first = [np.append(x, x[2]) for x in first]
        if entry_second:
            second[2][3] = 65536
        if entry_first:
            first[0][59] = TL
        return first, second
    e = _refused(*faulty(True, True, True, True, True), join.MODE_DEPTH)
    assert (e.what, e.side, e.entry) == ("entry", 0, 59)  # FIRST's entry check, although SECOND's offender comes earlier in its file
    e = _refused(*faulty(False, True, True, True, True), join.MODE_DEPTH)
    assert (e.what, e.side, e.entry) == ("entry", 1, 3)
    e = _refused(*faulty(False, False, True, True, True), join.MODE_DEPTH)
    assert (e.what, e.side) == ("duplicate", 0)  # ... although SECOND's duplicated key is the smaller one
    e = _refused(*faulty(False, False, False, True, True), join.MODE_DEPTH)
    assert (e.what, e.side) == ("duplicate", 1)
    assert _refused(*faulty(depth=True), join.MODE_DEPTH).what == "depth"
    with pytest.raises(join.JoinError) as bad_mode:
        join.join_coo(*faulty(True), 3, TL, TC)
    assert bad_mode.value.what == "mode"
