"""The numpy twin of cellector_add_doublets (cellector_amd/doublets.py) against a brute-force dict-of-dicts implementation in
plain Python integers, and the properties of the draw: independent per (pair, side), deterministic in (seed, i, j, s), untouched
by the presence of other pairs (no GPU needed)."""
import numpy as np
import pytest

from cellector_amd import doublets

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15


def mix64(z):
    z &= M64
    z ^= z >> 30; z = z * 0xBF58476D1CE4E5B9 & M64
    z ^= z >> 27; z = z * 0x94D049BB133111EB & M64
    return z ^ z >> 31


def brute(coo, n_cells, cell_a, cell_b, rate=0.0, seed=4):
    """the staged entries after the call, as a sorted list of (locus, cell, ref, alt): one dict of loci per new cell"""
    locus, cell, alt, ref = [[int(x) for x in a] for a in coo]
    t = int(float(rate) * 9007199254740992.0)
    rows = {}
    for j, (a, b) in enumerate(zip(cell_a, cell_b)):
        row = rows.setdefault(n_cells + j, {})
        for s, parent in enumerate((int(a), int(b))):
            for i in range(len(locus)):
                if cell[i] != parent:
                    continue
                h = mix64(mix64((seed * GOLD & M64) ^ ((i + 1) * GOLD & M64)) ^ ((2 * j + s + 1) * GOLD & M64))
                kept = []
                for allele, count in ((0, ref[i]), (1, alt[i])):
                    kept.append(sum(1 for r in range(count) if t == 0 or (mix64(h + (2 * r + allele + 1) * GOLD) >> 11) >= t))
                at = row.setdefault(locus[i], [0, 0])
                at[0] += kept[0]
                at[1] += kept[1]
    lines = [(locus[i], cell[i], ref[i], alt[i]) for i in range(len(locus))]
    for c, row in rows.items():
        for l, (r, a) in row.items():
            if r > 65535 or a > 65535:
                raise ValueError("overflow")
            lines.append((l, c, r, a))
    return sorted(lines)


def lines_of(out):
    return list(zip(out[0].tolist(), out[1].tolist(), out[3].tolist(), out[2].tolist()))


def random_coo(rng, n_loci, n_cells, n, repeats=True, top=9):
    locus = rng.integers(0, n_loci, n)
    cell = rng.integers(0, n_cells, n)
    if not repeats:
        key = np.unique(locus * n_cells + cell)
        rng.shuffle(key)
        locus, cell = key // n_cells, key % n_cells
    n = len(locus)
    return [locus.astype(np.uint32), cell.astype(np.uint32), rng.integers(0, top, n).astype(np.uint32), rng.integers(0, top, n).astype(np.uint32)]


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("rate", [0.0, 0.5, 1.0])
def test_twin_equals_brute_force_on_random_coos(seed, rate):
    rng = np.random.default_rng(100 + seed)
    n_loci, n_cells = int(rng.integers(1, 12)), int(rng.integers(2, 14))
    coo = random_coo(rng, n_loci, n_cells, int(rng.integers(0, 80)), repeats=seed % 2 == 0)  # (repeated lines in half of them)
    n_pairs = int(rng.integers(1, 9))
    a = rng.integers(0, n_cells, n_pairs)
    b = (a + rng.integers(1, n_cells, n_pairs)) % n_cells
    out = doublets.add_doublets_coo(coo, n_cells, a, b, rate, seed + 1)
    assert lines_of(out) == brute(coo, n_cells, a, b, rate, seed + 1)
    assert out[4] == n_cells + n_pairs
    assert out[5].tolist() == list(range(n_cells)) + a.tolist() and out[6].tolist() == [0] * n_cells + [1] * n_pairs
    for arr in out[:4]:
        assert arr.dtype == np.uint32
    assert out[5].dtype == np.uint32 and out[6].dtype == np.uint8


def test_origin_and_source_compose():
    rng = np.random.default_rng(5)
    coo = random_coo(rng, 5, 6, 30)
    origin = np.array([10, 11, 12, 3, 4, 5], np.uint32)
    source = np.array([0, 0, 0, 1, 1, 2], np.uint8)
    out = doublets.add_doublets_coo(coo, 6, [3, 0], [1, 5], origin=origin, source=source, k=3)
    assert out[5].tolist() == [10, 11, 12, 3, 4, 5, 3, 10] and out[6].tolist() == [0, 0, 0, 1, 1, 2, 3, 3]


def test_repeated_lines_empty_parents_and_the_same_pair_twice():
    # cell 0: locus 2 three times; cell 1: loci 2 and 4; cells 2 and 3: no entry
    coo = [np.array([2, 4, 2, 2, 2], np.uint32), np.array([0, 1, 0, 1, 0], np.uint32), np.array([1, 2, 3, 4, 5], np.uint32),
           np.array([6, 7, 8, 9, 10], np.uint32)]
    out = doublets.add_doublets_coo(coo, 4, [0, 0, 2, 1, 0], [1, 2, 3, 0, 1])
    new = [x for x in lines_of(out) if x[1] >= 4]
    both = [(2, 6 + 8 + 10 + 9, 1 + 3 + 5 + 4), (4, 7, 2)]
    assert new == sorted([(l, 4, r, a) for l, r, a in both] + [(2, 5, 24, 9)] + [(l, 7, r, a) for l, r, a in both] +
                         [(l, 8, r, a) for l, r, a in both])  # cell 6 (two empty parents) has no entry
    assert out[4] == 9 and lines_of(out) == brute(coo, 4, [0, 0, 2, 1, 0], [1, 2, 3, 0, 1])
    # the same pair twice: equal at rate 0, two independent draws at rate 0.5
    coo[2][:] = 40; coo[3][:] = 40
    half = doublets.add_doublets_coo(coo, 4, [0, 0], [1, 1], 0.5, 9)
    first = [x[2:] for x in lines_of(half) if x[1] == 4]
    second = [x[2:] for x in lines_of(half) if x[1] == 5]
    assert len(first) == len(second) == 2 and first != second
    assert lines_of(half) == brute(coo, 4, [0, 0], [1, 1], 0.5, 9)


def test_a_hub_cell_in_130_pairs():
    rng = np.random.default_rng(8)
    n_cells = 140
    coo = random_coo(rng, 7, n_cells, 500, top=30)
    others = np.arange(1, 131)
    a = np.where(others % 2 == 0, 0, others)  # the hub is side a in some pairs, side b in the others
    b = np.where(others % 2 == 0, others, 0)
    out = doublets.add_doublets_coo(coo, n_cells, a, b, 0.5, 4)
    assert lines_of(out) == brute(coo, n_cells, a, b, 0.5, 4)
    # the hub's reads are drawn anew for every pair: against a partner without entries the doublet is the thinned hub alone
    lonely = [np.concatenate([x, y]) for x, y in zip(coo, [np.zeros(0, np.uint32)] * 4)]
    n2 = n_cells + 2
    two = doublets.add_doublets_coo(lonely, n2, [0, n_cells], [n_cells, 0], 0.5, 4)
    rows = [[x[2:] for x in lines_of(two) if x[1] == n2 + j] for j in (0, 1)]
    assert rows[0] != rows[1] and len(rows[0]) == len(rows[1]) > 0


def test_draws_are_independent_across_pairs_and_sides():
    # one parent entry of 2000 + 2000 reads, partner rows empty: every doublet is one draw of the same entry
    coo = [np.zeros(1, np.uint32), np.zeros(1, np.uint32), np.array([2000], np.uint32), np.array([2000], np.uint32)]
    out = doublets.add_doublets_coo(coo, 3, [0, 0, 1, 2], [1, 2, 0, 0], 0.5, 4)
    draws = [x[2:] for x in lines_of(out) if x[1] >= 3]
    assert len(draws) == 4 and len(set(draws)) == 4  # two pairs sharing a parent differ; side a and side b differ
    for r, a in draws:
        assert 850 < r < 1150 and 850 < a < 1150  # 2000 fair coins: six standard deviations are 134


def test_draws_are_deterministic_and_do_not_depend_on_other_pairs():
    rng = np.random.default_rng(21)
    coo = random_coo(rng, 9, 12, 120, top=40)
    a = np.array([0, 3, 5, 3, 7])
    b = np.array([1, 4, 3, 9, 2])
    full = doublets.add_doublets_coo(coo, 12, a, b, 0.5, 6)
    again = doublets.add_doublets_coo(coo, 12, a, b, 0.5, 6)
    assert lines_of(full) == lines_of(again)
    other_seed = doublets.add_doublets_coo(coo, 12, a, b, 0.5, 7)
    assert lines_of(full) != lines_of(other_seed)
    # pair j alone at its own index: pad the front with pairs of other cells and take only cell 12 + j
    for j in range(len(a)):
        rest_a, rest_b = a.copy(), b.copy()
        for m in range(len(a)):
            if m != j:
                rest_a[m], rest_b[m] = 10, 11
        alone = doublets.add_doublets_coo(coo, 12, rest_a, rest_b, 0.5, 6)
        pick = lambda out: [x for x in lines_of(out) if x[1] == 12 + j]
        assert pick(alone) == pick(full)
    # ... but the index j is part of the key: the same parents at another index draw differently
    moved = doublets.add_doublets_coo(coo, 12, a[::-1], b[::-1], 0.5, 6)
    assert [x[2:] for x in lines_of(moved) if x[1] == 12 + 4] != [x[2:] for x in lines_of(full) if x[1] == 12]


def test_rates_0_and_1():
    rng = np.random.default_rng(2)
    coo = random_coo(rng, 6, 8, 60, repeats=False, top=50)
    a, b = np.array([0, 2, 4]), np.array([1, 3, 5])
    zero = doublets.add_doublets_coo(coo, 8, a, b, 0.0, 4)
    for j in range(3):
        for l in range(6):
            mine = [x for x in lines_of(zero) if x[:2] == (l, 8 + j)]
            rows = [i for i in range(len(coo[0])) if coo[0][i] == l and coo[1][i] in (a[j], b[j])]
            assert len(mine) == (1 if rows else 0)
            if rows:
                assert mine[0][2:] == (int(coo[3][rows].sum()), int(coo[2][rows].sum()))
    assert lines_of(zero) == lines_of(doublets.add_doublets_coo(coo, 8, a, b, 0.0, 99))  # rate 0 draws nothing
    one = doublets.add_doublets_coo(coo, 8, a, b, 1.0, 4)
    new0, new1 = [x for x in lines_of(zero) if x[1] >= 8], [x for x in lines_of(one) if x[1] >= 8]
    assert [x[:2] for x in new1] == [x[:2] for x in new0] and all(x[2:] == (0, 0) for x in new1)  # the entries stay, at 0
    # the parents' own entries are never changed
    for out in (zero, one, doublets.add_doublets_coo(coo, 8, a, b, 0.5, 4)):
        assert [x for x in lines_of(out) if x[1] < 8] == sorted(zip(coo[0].tolist(), coo[1].tolist(), coo[3].tolist(), coo[2].tolist()))


def test_a_sum_of_exactly_65535_is_accepted_and_40000_plus_40000_raises():
    coo = [np.array([3, 3, 5, 5], np.uint32), np.array([0, 1, 0, 1], np.uint32), np.array([65535, 0, 30000, 35535], np.uint32),
           np.array([1, 65534, 7, 8], np.uint32)]
    out = doublets.add_doublets_coo(coo, 2, [0], [1])
    assert [x for x in lines_of(out) if x[1] == 2] == [(3, 2, 65535, 65535), (5, 2, 15, 65535)]
    coo[3][2:] = 40000  # ref at locus 5; alt at locus 5 made too large as well: ref is named, the first allele of the entry
    coo[2][3] = 35536
    with pytest.raises(ValueError) as e:
        doublets.add_doublets_coo(coo, 2, [1, 0], [0, 1])
    assert "pair 0 (1, 0)" in str(e.value) and "locus 5" in str(e.value) and "ref" in str(e.value)
    coo[3][2:] = 1
    with pytest.raises(ValueError) as e:
        doublets.add_doublets_coo(coo, 2, [1, 0], [0, 1])
    assert "pair 0 (1, 0)" in str(e.value) and "locus 5" in str(e.value) and "alt" in str(e.value)
    # thinned below the bound, the same parents are accepted
    assert doublets.add_doublets_coo(coo, 2, [1, 0], [0, 1], 0.5)[4] == 4
