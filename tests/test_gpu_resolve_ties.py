"""Option resolve_ties (kernels_resolve.hip) on the MI355X against the CPU oracle: with it on, median, iqr, threshold and the
exclusion flags of every iteration are the oracle's bits, and so are the normalised LLs of the cells it evaluates."""
import subprocess

import numpy as np
import pytest

from test_gpu_parity import mods  # noqa: F401  (the two-engine fixture)
from test_host_cli import _write_inputs, host_bin, rust_display  # noqa: F401

pytestmark = pytest.mark.gpu


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _order_stats(norm):
    """The oracle's six order statistics (median pair, R-8 quartile pairs) and nothing else: values, not ranks."""
    s = np.sort(norm)
    n = s.size
    out = [s[n // 2], s[max(n // 2 - 1, 0)]]
    for tau in (0.25, 0.75):
        hf = int((n + 1.0 / 3.0) * tau + 1.0 / 3.0)
        out += [s[min(max(hf - 1, 0), n - 1)], s[min(max(hf, 0), n - 1)]]
    return out


def _run_resolved(g, o, max_iter=30, check_all=False):
    """Iterations until the oracle converges; every summary, flag set and near-band normalised LL is the oracle's."""
    res = []
    for it in range(max_iter):
        sg, so = g.em_iteration(5.0), o.em_iteration(5.0)
        assert (sg.median, sg.iqr, sg.threshold) == (so.median, so.iqr, so.threshold), f"iteration {it + 1}"
        assert np.array_equal(g.excluded(), o.excluded()), f"iteration {it + 1}"
        assert (sg.n_new_excluded, sg.n_rescued, sg.any_change) == (so.n_new_excluded, so.n_rescued, so.any_change)
        cg, co = g.cell_outputs(), o.cell_outputs()
        r = g.resolution()
        assert r.mode == (2 if check_all else 1)
        if check_all:
            assert r.n_evaluated == o.total_cells
            assert np.array_equal(_bits(cg["normalized"]), _bits(co["normalized"])), f"iteration {it + 1}"
            assert np.array_equal(_bits(cg["ll"]), _bits(co["ll"]))
        else:
            # every evaluated cell has the oracle's bits, and the cells next to the oracle's order statistics and threshold
            # are among them
            ev = g.resolved_cells()
            assert ev.size == r.n_evaluated and np.unique(ev).size == ev.size
            norm = co["normalized"]
            assert np.array_equal(_bits(cg["normalized"][ev]), _bits(norm[ev])), f"iteration {it + 1}"
            assert np.array_equal(_bits(cg["ll"][ev]), _bits(co["ll"][ev]))
            near = np.zeros(norm.size, bool)
            for v in _order_stats(norm) + [so.threshold]:
                near |= np.abs(norm - v) <= 1e-10 * max(1.0, abs(v))
            assert near.sum() > 0 and np.isin(np.flatnonzero(near), ev).all(), f"iteration {it + 1}"
        res.append((sg, cg, g.excluded(), r))
        if not so.any_change:
            break
    return res


def _resolved_case(mods, mode, L, N, d, seed=4, minority=0.05, doublet=0.0):
    """_case with the option set before the ingest (which then keeps every cell's entries in file order)"""
    lo, ce, al, re = mods["synth"].generate_coo(L, N, d, seed=seed, minority_fraction=minority, doublet_fraction=doublet)
    g = mods["Cellector"](0)
    g.set_option("resolve_ties", mode)
    g.load_coo(L, N, lo, ce, al, re)
    return g, mods["ob"].Oracle.from_coo(L, N, lo, ce, al, re), (lo, ce, al, re)


@pytest.mark.parametrize("shape", ["cfg1", "doublets", "wide"])
def test_whole_runs_match_the_oracle_bit_for_bit(mods, shape):
    if shape == "cfg1":
        g, o, _ = _resolved_case(mods, 1, 2000, 1000, 0.10)
    elif shape == "doublets":
        g, o, _ = _resolved_case(mods, 1, 3000, 1500, 0.08, seed=7, minority=0.1, doublet=0.03)
    else:
        lo, ce, al, re = mods["synth"].generate_coo(1200, 900, 0.1, seed=21, minority_fraction=0.09)
        g = mods["Cellector"](0)
        g.set_option("compact_bits", 32)
        g.set_option("resolve_ties", 1)
        g.load_coo(1200, 900, lo, ce, al, re)
        o = mods["ob"].Oracle.from_coo(1200, 900, lo, ce, al, re)
    assert len(_run_resolved(g, o)) >= 2
    g.close(); o.close()


def test_deep_coverage_run_matches_the_oracle(mods):
    L, N = 1500, 800
    lo, ce, al, re = mods["synth"].generate_coo(L, N, 0.1, seed=13, minority_fraction=0.08, continue_pct=60)
    g = mods["Cellector"](0)
    g.set_option("resolve_ties", 1)
    g.load_coo(L, N, lo, ce, al, re)
    o = mods["ob"].Oracle.from_coo(L, N, lo, ce, al, re)
    _run_resolved(g, o)
    g.close(); o.close()


def test_every_cell_mode_equals_band_mode(mods):
    """Mode 2 evaluates every cell: its normalised LLs are the oracle's everywhere, and its summaries and flags are mode 1's
    (the band argument of DESIGN §5 loses nothing)."""
    g1, o1, coo = _resolved_case(mods, 1, 2000, 1000, 0.10, seed=9, minority=0.08)
    g2, o2, _ = _resolved_case(mods, 2, 2000, 1000, 0.10, seed=9, minority=0.08)
    r1 = _run_resolved(g1, o1)
    r2 = _run_resolved(g2, o2, check_all=True)
    assert len(r1) == len(r2)
    for (s1, _, x1, _), (s2, _, x2, _) in zip(r1, r2):
        assert _bits([s1.median, s1.iqr, s1.threshold]).tolist() == _bits([s2.median, s2.iqr, s2.threshold]).tolist()
        assert (s1.n_excluded, s1.n_new_excluded, s1.n_rescued) == (s2.n_excluded, s2.n_new_excluded, s2.n_rescued)
        assert np.array_equal(x1, x2)
    for x in (g1, g2, o1, o2):
        x.close()


def _flip_coo(perm, L=400, n_same=8):
    """n_same identical cells and one more (the last) with the same entries in the order `perm`; COO in cell order.
    (Few identical cells keep alpha and beta small.  With some 40 of them every term is a multiple of the ulp of its ln_gamma
    values, ~2^-40, and a sum of a few hundred such terms is exact in any order: no permutation could flip the cell.)"""
    loci = np.arange(L, dtype=np.uint32)
    alt = (1 + (loci * 7) % 3).astype(np.uint32)
    ref = (1 + (loci * 5) % 4).astype(np.uint32)
    lo = np.concatenate([loci] * n_same + [loci[perm]])
    ce = np.repeat(np.arange(n_same + 1, dtype=np.uint32), L)
    al = np.concatenate([alt] * n_same + [alt[perm]])
    re = np.concatenate([ref] * n_same + [ref[perm]])
    return L, n_same + 1, lo, ce, al, re


def test_constructed_flip_follows_the_oracle(mods):
    """iqr 0 puts the threshold exactly on the identical cells' value; the extra cell holds the same entries in another file
    order, so only the rounding of its sum decides whether the reference excludes it.  Precondition, on the oracle alone: one
    permutation where it is excluded and one where it is not.  The device must decide as the oracle does in both."""
    rng = np.random.default_rng(3)
    want = {}
    for _ in range(200):
        perm = rng.permutation(400)
        L, N, lo, ce, al, re = _flip_coo(perm)
        o = mods["ob"].Oracle.from_coo(L, N, lo, ce, al, re)
        so = o.em_iteration(5.0)
        assert so.iqr == 0.0
        want.setdefault(bool(o.excluded()[-1]), perm)
        o.close()
        if len(want) == 2:
            break
    assert set(want) == {True, False}, "no permutation on one side of the threshold"
    for excluded, perm in want.items():
        L, N, lo, ce, al, re = _flip_coo(perm)
        g = mods["Cellector"](0)
        g.set_option("resolve_ties", 1)
        g.load_coo(L, N, lo, ce, al, re)
        o = mods["ob"].Oracle.from_coo(L, N, lo, ce, al, re)
        sg, so = g.em_iteration(5.0), o.em_iteration(5.0)
        assert (sg.median, sg.iqr, sg.threshold) == (so.median, so.iqr, so.threshold)
        assert bool(g.excluded()[-1]) == excluded
        assert np.array_equal(g.excluded(), o.excluded())
        assert _bits(g.cell_outputs()["normalized"]).tolist() == _bits(o.cell_outputs()["normalized"]).tolist()
        g.close(); o.close()


def test_identical_cells_summary_is_the_oracles(mods):
    L, N = 40, 50
    lo = np.repeat(np.arange(L, dtype=np.uint32), N)
    ce = np.tile(np.arange(N, dtype=np.uint32), L)
    al = np.ones(L * N, np.uint32)
    re = np.ones(L * N, np.uint32)
    g = mods["Cellector"](0)
    g.set_option("resolve_ties", 1)
    g.load_coo(L, N, lo, ce, al, re)
    o = mods["ob"].Oracle.from_coo(L, N, lo, ce, al, re)
    sg, so = g.em_iteration(5.0), o.em_iteration(5.0)
    assert _bits([sg.median, sg.iqr, sg.threshold]).tolist() == _bits([so.median, so.iqr, so.threshold]).tolist()
    assert (sg.n_excluded, sg.any_change) == (0, 0) and np.array_equal(g.excluded(), o.excluded())
    assert g.resolution().n_evaluated == N
    g.close(); o.close()


def test_cli_resolve_near_ties_prints_the_oracles_lines(host_bin, oracle_lib, tmp_path):
    L, N = 1500, 700
    coo, alt, ref, bc, gt, vcf = _write_inputs(str(tmp_path), L, N, 0.12, seed=4, minority=0.08)
    out = str(tmp_path / "out")
    base = [host_bin, "-a", alt, "-r", ref, "--output_directory", out, "--barcodes", bc]
    r = subprocess.run(base + ["--resolve_near_ties", "true"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "warning:" not in r.stderr
    lines = [ln for ln in r.stdout.splitlines() if not ln.startswith("filtering locus")]
    o = oracle_lib.Oracle.from_mtx(alt, ref, 4, 4)
    it = 0
    while True:
        s = o.em_iteration(5.0)
        assert lines[2 * it] == (f"detected {s.n_new_excluded} new anomylous cells and rescued {s.n_rescued} cells to the "
                                 f"majority in iteration {it + 1}")
        assert lines[2 * it + 1] == (f"median normalized log likelihood {rust_display(s.median)} with interquartile range "
                                     f"{rust_display(s.iqr)}, threshold {rust_display(s.threshold)}")
        it += 1
        if not s.any_change:
            break
    o.close()
    r = subprocess.run(base + ["--resolve_near_ties", "true", "--devices", "0,0"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "resolve_near_ties" in r.stderr


def test_refusals_and_the_default_path(mods):
    from cellector_amd import Cellector, CellectorError
    g = mods["Cellector"](0)
    with pytest.raises(CellectorError):
        g.set_option("resolve_ties", 3)
    g.close()
    m = Cellector(devices=[0, 0])
    with pytest.raises(CellectorError):
        m.set_option("resolve_ties", 1)
    m.close()
    # after an ingest without the option the cells' file order is gone: refused, not silently summed in another order
    lo, ce, al, re = mods["synth"].generate_coo(300, 200, 0.1, seed=2)
    g = mods["Cellector"](0)
    g.load_coo(300, 200, lo, ce, al, re)
    with pytest.raises(CellectorError):
        g.set_option("resolve_ties", 1)
    g.close()
    # resolve_ties = 0 is the path of a ctx where the option was never set, bit for bit
    lo, ce, al, re = mods["synth"].generate_coo(1500, 800, 0.1, seed=11, minority_fraction=0.08)
    ga, gb = mods["Cellector"](0), mods["Cellector"](0)
    gb.set_option("resolve_ties", 1)
    gb.set_option("resolve_ties", 0)
    for g in (ga, gb):
        g.load_coo(1500, 800, lo, ce, al, re)
    for _ in range(4):
        sa, sb = ga.em_iteration(5.0), gb.em_iteration(5.0)
        assert bytes(sa) == bytes(sb)
        ca, cb = ga.cell_outputs(), gb.cell_outputs()
        assert all(np.array_equal(_bits(ca[k]), _bits(cb[k])) for k in ca)
        assert np.array_equal(ga.excluded(), gb.excluded())
        assert gb.resolution().mode == 0 and gb.resolution().n_evaluated == 0
    ga.close(); gb.close()
