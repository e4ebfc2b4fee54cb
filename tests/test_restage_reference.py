"""The numpy twin of cellector_restage (cellector_amd/restage.py) against a plain per-entry Python loop that restates the
definition with Python integers (no GPU needed), and one seeded statistical check of the stream."""
import math

import numpy as np
import pytest

from cellector_amd import restage, synth

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15


def mix64(z):
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def loop_restage(locus, cell, alt, ref, total_cells, keep=None, rate=0.0, seed=4):
    """the definition, entry by entry"""
    T = int(rate * 9007199254740992.0)
    keep = [1] * total_cells if keep is None else [int(bool(k)) for k in keep]
    new_index, origin = {}, []
    for c in range(total_cells):
        if keep[c]:
            new_index[c] = len(origin)
            origin.append(c)
    out = [[], [], [], []]
    for i in range(len(locus)):
        counts = {0: int(ref[i]), 1: int(alt[i])}
        if T:  # rate 0: no draw is made
            h = mix64(((seed * GOLD) & M64) ^ (((i + 1) * GOLD) & M64))
            for a in (0, 1):
                counts[a] = sum(1 for r in range(counts[a]) if not (mix64(h + (2 * r + a + 1) * GOLD) >> 11) < T)
        if keep[int(cell[i])]:
            for o, v in zip(out, (int(locus[i]), new_index[int(cell[i])], counts[1], counts[0])):
                o.append(v)
    return [np.array(o, np.uint32) for o in out] + [len(origin), np.array(origin, np.uint32)]


def _same(a, b):
    assert len(a) == len(b) == 6
    for k in (0, 1, 2, 3, 5):
        assert a[k].dtype == np.uint32 and np.array_equal(a[k], b[k]), k
    assert a[4] == b[4]


@pytest.fixture(scope="module")
def coo():
    rng = np.random.default_rng(7)
    n, n_cells = 400, 37
    locus = np.sort(rng.integers(0, 50, n)).astype(np.uint32)
    cell = rng.integers(0, n_cells - 1, n).astype(np.uint32)  # (the last cell has no entries)
    alt = rng.integers(0, 6, n).astype(np.uint32)
    ref = rng.integers(0, 9, n).astype(np.uint32)
    alt[5], ref[5] = 300, 70000 & 0xffff
    keep = rng.random(n_cells) < 0.6
    keep[0], keep[n_cells - 1] = False, True
    return locus, cell, alt, ref, n_cells, keep


def test_rate_zero_is_the_identity(coo):
    locus, cell, alt, ref, n_cells, _ = coo
    out = restage.restage_coo(locus, cell, alt, ref, n_cells)
    _same(out, [locus, cell, alt, ref, n_cells, np.arange(n_cells, dtype=np.uint32)])
    _same(out, loop_restage(locus, cell, alt, ref, n_cells))


def test_rate_one_zeroes_every_count_and_keeps_every_entry(coo):
    locus, cell, alt, ref, n_cells, _ = coo
    out = restage.restage_coo(locus, cell, alt, ref, n_cells, downsample_rate=1.0)
    z = np.zeros(len(locus), np.uint32)
    _same(out, [locus, cell, z, z, n_cells, np.arange(n_cells, dtype=np.uint32)])
    _same(out, loop_restage(locus, cell, alt, ref, n_cells, rate=1.0))


@pytest.mark.parametrize("rate,seed", [(0.37, 4), (0.5, 0), (0.9, (1 << 63) + 12345)])
def test_twin_equals_the_loop(coo, rate, seed):
    locus, cell, alt, ref, n_cells, keep = coo
    _same(restage.restage_coo(locus, cell, alt, ref, n_cells, keep, rate, seed), loop_restage(locus, cell, alt, ref, n_cells, keep, rate, seed))
    _same(restage.restage_coo(locus, cell, alt, ref, n_cells, None, rate, seed), loop_restage(locus, cell, alt, ref, n_cells, None, rate, seed))


def test_the_draw_does_not_depend_on_keep(coo):
    locus, cell, alt, ref, n_cells, keep = coo
    thinned = restage.restage_coo(locus, cell, alt, ref, n_cells, None, 0.37, 9)
    two_steps = restage.restage_coo(*thinned[:4], n_cells, keep)
    _same(two_steps, restage.restage_coo(locus, cell, alt, ref, n_cells, keep, 0.37, 9))
    # an entry whose counts both reach 0 stays
    assert ((thinned[2] == 0) & (thinned[3] == 0)).any() and len(thinned[0]) == len(locus)


def test_renumbering_and_origin(coo):
    locus, cell, alt, ref, n_cells, keep = coo
    l2, c2, a2, r2, n2, origin = restage.restage_coo(locus, cell, alt, ref, n_cells, keep)
    assert n2 == int(keep.sum()) and np.array_equal(origin, np.nonzero(keep)[0])
    sel = keep[cell]
    assert np.array_equal(origin[c2], cell[sel])  # every survivor names its old cell, in the old order
    assert np.array_equal(l2, locus[sel]) and np.array_equal(a2, alt[sel]) and np.array_equal(r2, ref[sel])
    assert n2 - 1 not in c2 and origin[-1] == n_cells - 1  # the kept cell without entries stays, as an empty row
    with pytest.raises(ValueError):
        restage.restage_coo(locus, cell, alt, ref, n_cells, np.zeros(n_cells, bool))
    for bad in (1.5, -0.1, float("nan")):
        with pytest.raises(ValueError):
            restage.restage_coo(locus, cell, alt, ref, n_cells, None, bad)


def test_two_restages_compose(coo):
    locus, cell, alt, ref, n_cells, keep = coo
    first = restage.restage_coo(locus, cell, alt, ref, n_cells, keep)
    keep2 = np.arange(first[4]) % 3 != 1
    second = restage.restage_coo(*first[:5], keep2)
    both = keep.copy()
    both[first[5][~keep2]] = False
    direct = restage.restage_coo(locus, cell, alt, ref, n_cells, both)
    for k in range(5):
        assert np.array_equal(second[k], direct[k]) if k != 4 else second[k] == direct[k]
    assert np.array_equal(first[5][second[5]], direct[5])  # origins compose


@pytest.mark.parametrize("rate,seed,kept", [(0.3, 4, 120039), (0.6, 4, 68559)])
def test_kept_reads_are_binomial(rate, seed, kept):
    """N reads kept independently with probability 1 - r: the kept total lies within 5 sigma of N (1 - r)"""
    _, _, alt, ref = synth.generate_coo(1500, 800, 0.1, seed=11, minority_fraction=0.08, doublet_fraction=0.01)
    n = int(alt.sum()) + int(ref.sum())
    assert n == 171551
    a2, r2 = restage.thin_counts(alt, ref, rate, seed)
    got = int(a2.sum()) + int(r2.sum())
    sigma = math.sqrt(n * rate * (1 - rate))
    print(f"rate {rate} seed {seed}: kept {got} of {n}, {(got - n * (1 - rate)) / sigma:+.2f} sigma")
    assert abs(got - n * (1 - rate)) <= 5 * sigma
    assert got == kept  # the stream's own figure (deterministic)
    assert (a2 <= alt).all() and (r2 <= ref).all()
