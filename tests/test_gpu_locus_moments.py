"""GPU: the locus moments — cellector_locus_moments, cellector_locus_total_counts, option locus_moments /
cellector_iter_locus_moments — on both engines (the kernels stream the by-cell CSR both keep).

Matrix A is tests/test_gpu_cell_pmfs.py's value matrix (1400 loci x 1500 cells, ~42k entries, min_alt = min_ref = 0): rows of 0, 1,
63, 64, 65, 129 and 2100 entries, totals 0..25 on both sides of the table's last slot 17, a 0/0 entry, a pair listed three times,
single entries of total 80, 300 and 65535 at loci 702..704; alpha / beta of test_gpu_tile_sweep._alpha_beta, the four masks of
test_gpu_cell_variance.case_a.  Matrix C (tests/locus_moments_reference.py, 40 x 200) is the smallest shape at which the far
list's segments can go wrong.  Matrix B is synth.generate_coo(2000, 1000, 0.10) with min_alt = min_ref = 4: the loop.

Flag sets: empty, all, random 10 %, one that holds the planted far cells (and, on A, the 2100-entry row), its complement.

Bounds (tests/locus_moments_reference.py; u = 2^-53; nothing fitted): per locus and class, B = the sum of the entries' b_expected
(b_variance), plus (m + 1) u (|S| + B) for the device's 17 products and m = 17 + (far entries of the class) additions — all
terms of a sum have one sign, so every partial sum is at most the whole — plus half an ulp of S.  Against the device's own
records (cell_pmfs' two columns, added here in longdouble) only the multiply-adds remain: (m + 1) u |S| + ulp(S) / 2.

Worst observed / bound ratios are printed (pytest -s).
"""
import numpy as np
import pytest

import locus_moments_reference as lm
import pmf_reference as pr
import test_gpu_cell_pmfs as P
import test_gpu_cell_variance as V
import test_gpu_tile_sweep as S
from test_gpu_cell_variance import case_a, coo_b  # noqa: F401  (matrix A with its masks; matrix B)
from test_gpu_parity import mods  # noqa: F401  (both engines)

pytestmark = pytest.mark.gpu

L1, N1 = P.L1, P.N1
LD = np.longdouble
FAR_CELLS_A = [P.MID[1], P.BIG[1], P.HUGE[1], 26]  # the cells of the totals 80, 300, 65535 and the 2100-entry row


def _flag_sets(n_cells, planted, seed):
    rng = np.random.default_rng(seed)
    pl = np.zeros(n_cells, np.uint8)
    pl[planted] = 1
    return {"empty": np.zeros(n_cells, np.uint8), "all": np.ones(n_cells, np.uint8),
            "random 10 %": (rng.random(n_cells) < 0.1).astype(np.uint8), "planted": pl, "complement": (1 - pl).astype(np.uint8)}


@pytest.fixture(scope="module")
def cases(case_a):
    """matrix A (the reference records come from case_a) and matrix C: entries in CSR order, masks, flag sets"""
    a = dict(name="A", L=L1, N=N1, coo=case_a["coo"], alpha=case_a["alpha"], beta=case_a["beta"], lo=case_a["lo"], ce=case_a["ce"],
             n=case_a["n"], rec=case_a["rec"], masks=case_a["masks"], flags=_flag_sets(N1, FAR_CELLS_A, 23))
    coo = lm.matrix_c()
    order = lm.csr_order(coo[0], coo[1])
    lo, ce, al, re = (x[order] for x in coo)
    alpha, beta = S._alpha_beta(lm.LC, 40)
    c = dict(name="C", L=lm.LC, N=lm.NC, coo=coo, alpha=alpha, beta=beta, lo=lo, ce=ce, n=al + re,
             rec=pr.records(alpha, beta, lo, al, re), masks={"none": None, "two loci": lm.matrix_c_mask(), "all": np.zeros(lm.LC, np.uint8)},
             flags=lm.matrix_c_flags())
    return dict(A=a, C=c)


def _load(mods, c, opts=()):
    return P._load(mods, c["coo"], c["L"], c["N"], opts)


def test_counts_exact(mods, cases):
    """locus_total_counts is the numpy histogram for every flag set and for None; slot 18 = the far entries; the pair listed
    three times counts 3; per locus the row sum is cells_min (cells_min + cells_maj) of the oracle's locus stats, all loci used"""
    for c in cases.values():
        g = _load(mods, c)
        tag = f"engine {mods['engine']} matrix {c['name']}"
        h_all = g.locus_total_counts()
        assert h_all.shape == (c["L"], 19) and h_all.dtype == np.uint32, tag
        assert np.array_equal(h_all, lm.histogram(c["L"], c["lo"], c["ce"], c["n"])), tag
        assert np.array_equal(h_all[:, 18], np.bincount(c["lo"][c["n"] > lm.SMALL], minlength=c["L"])), tag
        assert h_all[:, 18].sum() > 0 and h_all[:, 0].sum() > 0, tag
        ob = mods["ob"].Oracle.from_coo(c["L"], c["N"], *S._u32(c["coo"]), 0, 0)
        ones = np.ones(c["L"], np.uint8)
        for name, f in c["flags"].items():
            h = g.locus_total_counts(f)
            assert np.array_equal(h, lm.histogram(c["L"], c["lo"], c["ce"], c["n"], f)), (tag, name)
            st = ob.locus_stats(c["alpha"], c["beta"], ones, f)
            assert np.array_equal(h.sum(axis=1), st["cells_min"]), (tag, name)
            assert np.array_equal(h_all.sum(axis=1), st["cells_min"] + st["cells_maj"]), (tag, name)
        if c["name"] == "A":
            only = np.zeros(N1, np.uint8)
            only[P.TRIPLE[1]] = 1
            want = int(((c["lo"] == P.TRIPLE[0]) & (c["ce"] == P.TRIPLE[1])).sum())
            assert want >= 3 and g.locus_total_counts(only)[P.TRIPLE[0]].sum() == want, tag
        else:
            tw = np.zeros(lm.NC, np.uint8)
            tw[lm.C_TWICE[1]] = 1
            assert g.locus_total_counts(tw)[lm.C_TWICE[0], 18] == 2, tag
        ob.close()
        g.close()


def _worst(tag, what, diff, bound):
    ok = bound > 0
    r = float((diff[ok] / bound[ok]).max()) if ok.any() else 0.0
    print(f"  {tag}: {what} worst |device - reference| / bound = {r:.3f} (largest bound {bound.max():.2e})")
    return np.nonzero(diff > bound)[0]


def test_values(mods, cases):
    """the four vectors under every mask and flag set against the longdouble sums of pmf_reference.records, within
    B + (m + 1) u (|S| + B) + ulp(S) / 2 (module docstring); exact zeros at masked loci, under the all-masked mask and for a
    class without entries"""
    for c in cases.values():
        g = _load(mods, c)
        for mname, m in c["masks"].items():
            for fname, f in c["flags"].items():
                tag = f"engine {mods['engine']} matrix {c['name']} mask '{mname}' flags '{fname}'"
                got = g.locus_moments(c["alpha"], c["beta"], m, f)
                assert sorted(got) == sorted(lm.KEYS), tag
                for k in lm.KEYS:
                    assert got[k].shape == (c["L"],) and np.isfinite(got[k]).all(), (tag, k)
                if m is not None:
                    for k in lm.KEYS:
                        assert not got[k][m == 0].any(), (tag, k)
                if mname == "all":
                    continue
                ref = lm.sums(c["L"], c["lo"], c["ce"], c["n"], c["rec"], m, f)
                for k in lm.KEYS:
                    d = np.abs((got[k].astype(LD) - ref[k]).astype(np.float64))
                    bad = _worst(tag, k, d, ref["b_" + k])
                    assert bad.size == 0, (tag, k, bad[:5], got[k][bad[:5]], ref[k][bad[:5]], ref["b_" + k][bad[:5]])
                    assert not got[k][ref[k] == 0].any(), (tag, k)  # no entry of the class at a used locus: an exact zero
                assert (got["exp_min"] <= 0).all() and (got["exp_maj"] <= 0).all() and (got["var_min"] >= 0).all() and (got["var_maj"] >= 0).all(), tag
                if fname == "empty":
                    assert not got["exp_min"].any() and not got["var_min"].any(), tag
                if fname == "all":
                    assert not got["exp_maj"].any() and not got["var_maj"].any() and got["exp_min"].any(), tag
        g.close()


def test_agrees_with_the_records(mods, cases):
    """the device's own cell_pmfs columns over all cells, summed per (locus, class) in longdouble, against locus_moments within the
    multiply-adds alone; every distinct (locus, total) is one value across all its records — a wrong table index or a wrong
    class moves a value by far more"""
    c = cases["A"]
    g = _load(mods, c)
    cells = np.arange(N1)
    for mname in ("none", "random 30 %"):
        m = c["masks"][mname]
        recs = g.cell_pmfs(cells, c["alpha"], c["beta"], m)
        rows = np.repeat(cells, np.diff(recs["rec_ptr"].astype(np.int64)))
        lo = recs["locus_index"].astype(np.int64)
        n = recs["alt"].astype(np.int64) + recs["ref"].astype(np.int64)
        key = lo * (1 << 20) + n
        _, first, inv = np.unique(key, return_index=True, return_inverse=True)
        for col in ("expected_log_pmf", "expected_log_variance"):
            assert np.array_equal(recs[col], recs[col][first][inv]), (mname, col)
        for fname in ("random 10 %", "planted", "complement"):
            f = c["flags"][fname]
            tag = f"engine {mods['engine']} mask '{mname}' flags '{fname}'"
            got = g.locus_moments(c["alpha"], c["beta"], m, f)
            is_min = f[rows] != 0
            for cls, sel in (("min", is_min), ("maj", ~is_min)):
                far = np.bincount(lo[sel & (n > lm.SMALL)], minlength=L1)
                for what, col in (("exp", "expected_log_pmf"), ("var", "expected_log_variance")):
                    s_ld = np.zeros(L1, LD)
                    np.add.at(s_ld, lo[sel], recs[col][sel].astype(LD))
                    k = f"{what}_{cls}"
                    d = np.abs((got[k].astype(LD) - s_ld).astype(np.float64))
                    bad = _worst(tag, k + " against the device's records", d, lm.add_bound(far, s_ld))
                    assert bad.size == 0, (tag, k, bad[:5], got[k][bad[:5]], s_ld[bad[:5]])
                    assert np.array_equal(got[k] == 0.0, s_ld == 0), (tag, k)
    g.close()


def test_bits(mods, cases):
    """the four vectors are the same bits on engine 1 and engine 2 and under bank_order 0 and 1"""
    from cellector_amd import Cellector
    for c in cases.values():
        mk = [m for name, m in c["masks"].items() if name != "all"]
        fl = [c["flags"][k] for k in ("random 10 %", "planted")]
        g0, g1 = _load(mods, c, [("bank_order", 0)]), _load(mods, c, [("bank_order", 1)])
        other = Cellector(0)
        other.set_option("engine", 3 - mods["engine"])
        other.load_coo(c["L"], c["N"], *S._u32(c["coo"]), 0, 0)
        for m in mk:
            for f in fl:
                a = g0.locus_moments(c["alpha"], c["beta"], m, f)
                for h in (g1, other):
                    b = h.locus_moments(c["alpha"], c["beta"], m, f)
                    for k in lm.KEYS:
                        assert np.array_equal(a[k], b[k]), (c["name"], k)
                assert np.array_equal(g0.locus_total_counts(f), other.locus_total_counts(f))
        g0.close(); g1.close(); other.close()


def test_the_loop(mods, coo_b):
    """matrix B, three iterations with the option on: iter_locus_moments() is locus_moments() under the alpha / beta and mask
    taken before the iteration and the exclusion set taken after it, to the bit; cell outputs, locus outputs and summaries are
    those of a run with the option off, to the bit; "not formed" with the option off and after em_reset"""
    ffi = mods["ffi"]
    ga, gb = V._load_b(mods, coo_b), V._load_b(mods, coo_b, [("locus_moments", 1), ("timing", 1)])
    for it in range(3):
        a, b = gb.alpha_betas()
        used = gb.loci_mask()
        sa, sb = ga.em_iteration(5.0), gb.em_iteration(5.0)
        assert P._summary(sa) == P._summary(sb), it
        got = gb.iter_locus_moments()
        want = gb.locus_moments(a, b, used, gb.excluded())
        for k in lm.KEYS:
            assert np.array_equal(got[k], want[k]), (it, k)
        assert got["exp_maj"].any() and (it == 0 or gb.excluded().any())
        if gb.excluded().any():
            assert got["exp_min"].any() and got["var_min"].any(), it
        for x, y in ((ga.cell_outputs(), gb.cell_outputs()), (ga.locus_outputs(), gb.locus_outputs())):
            for k in x:
                assert np.array_equal(x[k], y[k]), (it, k)
        assert np.array_equal(ga.excluded(), gb.excluded()) and np.array_equal(ga.loci_mask(), gb.loci_mask()), it
        with pytest.raises(ffi.CellectorError) as e:
            ga.iter_locus_moments()
        assert e.value.status == 1 and "not formed" in str(e.value)
    assert gb.excluded().sum() > 0
    assert gb.kernel_time(ffi.K_LOCUS_MOM)[1] == 3 and ga.kernel_time(ffi.K_LOCUS_MOM)[1] == 0
    # set_excluded / set_loci_mask keep the last iteration's vectors; em_reset drops them until an iteration has finished
    gb.set_excluded(np.zeros(V.NB, np.uint8))
    again = gb.iter_locus_moments()
    for k in lm.KEYS:
        assert np.array_equal(again[k], got[k]), k
    gb.em_reset()
    with pytest.raises(ffi.CellectorError) as e:
        gb.iter_locus_moments()
    assert e.value.status == 1 and "not formed" in str(e.value)
    gb.set_option("locus_moments", 0)
    gb.em_iteration(5.0)
    with pytest.raises(ffi.CellectorError):
        gb.iter_locus_moments()
    gb.set_option("locus_moments", 1)
    gb.em_iteration(5.0)
    assert gb.iter_locus_moments()["exp_maj"].any()
    ga.close(); gb.close()


def test_refusals(mods, coo_b):
    from cellector_amd import Cellector
    ffi = mods["ffi"]

    def refused(call, *words):
        with pytest.raises(ffi.CellectorError) as e:
            call()
        assert e.value.status == 1 and all(w in str(e.value) for w in words), str(e.value)

    coo = S._u32(coo_b)
    # a multi-device ctx: the option, the three calls
    m = Cellector(devices=[0, 0])
    m.set_option("engine", mods["engine"])
    refused(lambda: m.set_option("locus_moments", 1), "single-device")
    m.set_option("locus_moments", 0)
    m.load_coo(V.LB, V.NB, *coo, 4, 4)
    L = m.dims().loci_used
    a, b = m.alpha_betas()
    refused(lambda: m.locus_moments(a, b, None, np.zeros(V.NB, np.uint8)), "single-device")
    refused(lambda: m.locus_total_counts(), "single-device")
    refused(lambda: m.iter_locus_moments(), "single-device")
    refused(lambda: m.set_option("locus_moments", 1), "single-device")
    assert m.em_iteration(5.0).n_new_excluded == 47  # usable afterwards
    m.close()
    # a cellector_set_shard range, whichever is set first
    g = mods["Cellector"](0)
    g.set_option("locus_moments", 1)
    refused(lambda: g.set_shard(100, 600), "locus_moments")
    g.set_option("locus_moments", 0)
    g.set_shard(100, 600)
    refused(lambda: g.set_option("locus_moments", 1), "set_shard")
    g.load_coo(V.LB, V.NB, *coo, 4, 4)
    assert g.n_local == 500
    ones = np.ones(g.dims().loci_used)  # (a shard without an exchange filters the loci by its own cells)
    refused(lambda: g.locus_moments(ones, ones, None, np.zeros(500, np.uint8)), "set_shard")
    refused(lambda: g.locus_total_counts(), "set_shard")
    refused(lambda: g.set_option("locus_moments", 1), "set_shard")
    assert len(g.cell_log_variances(ones, ones)) == 500  # usable afterwards
    g.close()
    g = mods["Cellector"](0)
    g.set_shard(0, 500)  # (a range from cell 0 is known to be one only once the matrix is: the calls and the loop refuse)
    g.set_option("locus_moments", 1)
    g.load_coo(V.LB, V.NB, *coo, 4, 4)
    refused(lambda: g.locus_total_counts(), "set_shard")
    g.em_begin()
    refused(lambda: g.em_threshold(5.0), "set_shard")
    g.close()
    # before a load; an iteration in flight; wrong lengths
    g = mods["Cellector"](0)
    refused(lambda: g.iter_locus_moments())
    refused(lambda: g.locus_total_counts())
    g.load_coo(V.LB, V.NB, *coo, 4, 4)
    f = np.zeros(V.NB, np.uint8)
    f[::7] = 1
    g.em_begin()
    refused(lambda: g.locus_moments(a, b, None, f), "in flight")
    g.em_threshold(5.0)
    refused(lambda: g.locus_moments(a, b, None, f), "in flight")
    refused(lambda: g.locus_total_counts(f), "in flight")
    refused(lambda: g.iter_locus_moments(), "in flight")
    g.em_finish()
    for call in (lambda: g.locus_moments(a[:-1], b, None, f), lambda: g.locus_moments(a, b, np.ones(L + 1, np.uint8), f),
                 lambda: g.locus_moments(a, b, None, f[:-1]), lambda: g.locus_total_counts(f[:-1])):
        with pytest.raises(ValueError):
            call()
    refused(lambda: g.set_option("locus_moments", 2), "locus_moments")
    got = g.locus_moments(a, b, None, f)  # usable afterwards
    assert got["exp_min"].any() and got["exp_maj"].any() and g.locus_total_counts(f).sum() > 0
    assert g.em_iteration(5.0).n_excluded == 47
    g.close()
