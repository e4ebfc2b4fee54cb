"""GPU: cellector_cell_pmfs (the reference's PMFData, main.rs:527-539, of listed cells) and cellector_posterior_alpha_betas, on
both engines (the by-cell CSR both keep), min_alt = min_ref = 0 so that every locus is used and locus_index is the file's locus.

Matrix of the value cases: 1400 loci (three chunks of the tiled layout, the last short) x 1500 cells (two cell blocks), about 40k
entries drawn like tests/test_gpu_tile_sweep.py's (SHALLOW totals: 0..25, i.e. both sides of DM_MOM_SMALL = 17, where the kernel
hands an entry to the whole wave), and planted: rows of 0, 1, 63, 64, 65, 129 and 2100 entries (the fill pass strides a row in
64-entry steps; 2100 > 1400 loci: 700 of its pairs are listed twice), one (locus, cell) pair listed three times, one 0/0 entry,
one entry each of total 80, 300 and 65535.  alpha, beta log-uniform in [1, 1e4] (test_gpu_tile_sweep._alpha_beta).

Bounds.  log_pmf: tile_reference.term_bound; expected_log_pmf: tile_reference.expected_bound; the variance: against the oracle at
1e-7 max(1, |v|) (its ln_gamma noise, the tolerance of every GPU-versus-oracle file here) and against tests/pmf_reference.py's
value within pmf_reference.variance_bound, derived there from the device's operation count (its module docstring; nothing is
fitted).  For the one entry of total 65535 the largest B_term over k, an ingredient of expected_bound and of the variance bound,
cannot be evaluated (65536 terms of 65535 factors): pmf_reference.term_bound_upper bounds it from above, and its reference
values come from mpmath (pmf_reference module docstring).  ln C's 1.5 ulp of tile_reference.ln_choose_bound is established up
to total 64 (tests/test_tile_reference.py); for the planted total of 80, (37, 43), tests/test_pmf_reference.py checks that pair.

The mask case compares per-cell sums of records with cell_log_likelihoods, whose reference (tile_reference.cell_reference) and
engine 1's cell pass (a log-space fold of n + 1 log-pmfs of n factors each) are both O(n^2) in a total: it runs on the same matrix
WITHOUT the total-65535 entry.

Worst observed / bound ratios are printed per case (pytest -s).
"""
import ctypes as C

import numpy as np
import pytest

import pmf_reference as pr
import test_gpu_tile_sweep as S
import tile_reference as tr
from test_gpu_parity import mods  # noqa: F401  (both engines)

pytestmark = pytest.mark.gpu

L1, N1 = 1400, 1500
PLANTED = {20: 0, 21: 1, 22: 63, 23: 64, 24: 65, 25: 129, 26: 2100}  # cell -> entries of its row
TRIPLE, ZERO, MID, BIG, HUGE = (700, 40), (701, 41), (702, 42), (703, 43), (704, N1 - 1)  # (locus, cell) of the single plants


def _case1_coo(huge=True):
    rng = np.random.default_rng(99)
    lo, ce, al, re = S._random_coo(99, L1, N1, 40_000)
    keep = ~np.isin(ce, list(PLANTED))
    lo, ce, al, re = lo[keep], ce[keep], al[keep], re[keep]
    add = [[], [], [], []]
    for cell, k in PLANTED.items():
        loci = np.concatenate([rng.permutation(L1)[:min(k, L1)], rng.permutation(L1)[:max(0, k - L1)]])
        tot = rng.choice(S.SHALLOW, k)
        a = (rng.random(k) * (tot + 1)).astype(np.int64)
        for i, v in enumerate((loci, np.full(k, cell), a, tot - a)):
            add[i].append(v)
    singles = [TRIPLE + (1, 0), TRIPLE + (0, 2), TRIPLE + (3, 1), ZERO + (0, 0), MID + (37, 43), BIG + (120, 180)]
    if huge:
        singles.append(HUGE + (40000, 25535))
    for l, c, a, r in singles:
        for i, v in enumerate((l, c, a, r)):
            add[i].append(np.array([v]))
    coo = [np.concatenate([x] + y).astype(np.int64) for x, y in zip((lo, ce, al, re), add)]
    perm = rng.permutation(len(coo[0]))  # (load order is arbitrary: the ingest sorts by locus, stably)
    perm = perm[np.argsort(coo[0][perm], kind="stable")]  # ... but keep it locus-major, so that "file order" inside a pair is defined here
    return [x[perm] for x in coo]


def _csr_order(coo):
    """the by-cell CSR's order: cell, then locus, repeated pairs in load order"""
    lo, ce = coo[0], coo[1]
    return np.lexsort((np.arange(len(lo)), lo, ce))


@pytest.fixture(scope="module")
def case1(oracle_lib):
    coo = _case1_coo()
    alpha, beta = S._alpha_beta(L1, 99)
    order = _csr_order(coo)
    lo, ce, al, re = (x[order] for x in coo)
    rp = np.concatenate([[0], np.cumsum(np.bincount(ce, minlength=N1))]).astype(np.uint64)
    assert [int(rp[c + 1] - rp[c]) for c in PLANTED] == list(PLANTED.values())
    rec = pr.records(alpha, beta, lo, al, re)
    # the oracle's variance (and expected term) per distinct (locus, total)
    key = lo * (1 << 20) + (al + re)
    uk, inv = np.unique(key, return_inverse=True)
    ov = np.array([oracle_lib.expected_log_pmf(int(k & 0xFFFFF), float(alpha[k >> 20]), float(beta[k >> 20])) for k in uk])
    return dict(coo=coo, alpha=alpha, beta=beta, lo=lo, ce=ce, al=al, re=re, rp=rp, rec=rec, o_e=ov[inv, 0], o_v=ov[inv, 1])


def _load(mods, coo, L=L1, N=N1, opts=()):
    g = mods["Cellector"](0)
    for k, v in opts:
        g.set_option(k, v)
    g.load_coo(L, N, *S._u32(coo), 0, 0)
    assert g.dims().loci_used == L
    return g


def _rows(rp, cells):
    """positions, in the all-cells record order, of the records of a cell list; and the list's rec_ptr"""
    cells = np.asarray(cells, np.int64)
    n = (rp[cells + 1] - rp[cells]).astype(np.int64)
    ptr = np.concatenate([[0], np.cumsum(n)]).astype(np.uint64)
    idx = np.concatenate([np.arange(int(rp[c]), int(rp[c + 1])) for c in cells] + [np.zeros(0, np.int64)]).astype(np.int64)
    return idx, ptr


def _lists():
    rng = np.random.default_rng(5)
    must = list(PLANTED) + [TRIPLE[1], ZERO[1], MID[1], BIG[1], N1 - 1, 0, 1023, 1024]
    subset = np.array(sorted(set(must) | set(rng.choice(N1, 200, replace=False).tolist())))
    rng.shuffle(subset)
    return {"all": np.arange(N1), "shuffled subset": subset, "repeat": np.array([26, 5, 26, N1 - 1, 5, 22]), "empty": np.zeros(0, np.int64)}


def _worst(tag, name, diff, bound):
    r = S._ratio(diff, bound)
    bad = np.nonzero(diff > bound)[0]
    print(f"  {tag}: {name} worst |device - reference| / bound = {r:.3f} (largest bound {bound.max() if len(bound) else 0:.2e})")
    return r, bad


def test_values(mods, case1):
    """every list: rec_ptr = the CSR row lengths, the integer columns = csr_rows unpacked entry for entry (and the order stated
    in the header: ascending locus, repeated pairs in load order), the three values within their bounds"""
    c = case1
    g = _load(mods, c["coo"])
    rp_dev, ent = g.csr_rows(0, N1)
    assert np.array_equal(rp_dev, c["rp"])
    assert np.array_equal(ent & np.uint64(0xFFFFFFFF), c["lo"].astype(np.uint64))
    assert np.array_equal((ent >> np.uint64(32)) & np.uint64(0xFFFF), c["al"].astype(np.uint64))
    assert np.array_equal(ent >> np.uint64(48), c["re"].astype(np.uint64))
    rec = c["rec"]
    for name, cells in _lists().items():
        tag = f"engine {mods['engine']} list '{name}'"
        idx, ptr = _rows(c["rp"], cells)
        got = g.cell_pmfs(cells, c["alpha"], c["beta"])
        assert np.array_equal(got["rec_ptr"], ptr), tag
        assert np.array_equal(got["locus_index"], (ent[idx] & np.uint64(0xFFFFFFFF)).astype(np.uint32)), tag
        assert np.array_equal(got["alt"], ((ent[idx] >> np.uint64(32)) & np.uint64(0xFFFF)).astype(np.uint32)), tag
        assert np.array_equal(got["ref"], (ent[idx] >> np.uint64(48)).astype(np.uint32)), tag
        if name == "empty":
            assert len(got["rec_ptr"]) == 1 and all(len(got[k]) == 0 for k in got if k != "rec_ptr")
            continue
        for k in ("log_pmf", "expected_log_pmf", "expected_log_variance"):
            assert np.isfinite(got[k]).all(), (tag, k)
        n = (c["al"] + c["re"])[idx]
        zero = n == 0  # the 0/0 entry (and SHALLOW's zero totals): 0, 0, 0
        assert zero.any() and not got["log_pmf"][zero].any() and not got["expected_log_pmf"][zero].any() \
            and not got["expected_log_variance"][zero].any()
        for col, want, bound in (("log_pmf", rec["log_pmf"], rec["b_log_pmf"]), ("expected_log_pmf", rec["expected"], rec["b_expected"]),
                                 ("expected_log_variance", rec["variance"], rec["b_variance"])):
            d = np.abs(got[col] - want[idx])
            _, bad = _worst(tag, col, d, bound[idx])
            assert bad.size == 0, (f"{tag}: {col} beyond its bound at {bad.size} of {len(d)} records, first {bad[:5]}: device "
                                   f"{got[col][bad[:5]]}, reference {want[idx][bad[:5]]}, bound {bound[idx][bad[:5]]}, totals {n[bad[:5]]}")
        # the oracle's values at its own noise
        for col, want in (("expected_log_pmf", c["o_e"]), ("expected_log_variance", c["o_v"])):
            w = want[idx]
            d = np.abs(got[col] - w) / np.maximum(1.0, np.abs(w))
            print(f"  {tag}: {col} against the oracle, worst relative {d.max():.2e} (tolerance 1e-7)")
            assert (d <= 1e-7).all(), (tag, col, np.nonzero(d > 1e-7)[0][:5])
        # a column that is not asked for is not needed by the others
        if name == "repeat":
            rp2 = np.zeros(len(cells) + 1, np.uint64)
            cc = np.ascontiguousarray(cells, np.uint32)
            v = np.zeros(int(ptr[-1]), np.float64)
            g._ck(g._lib.cellector_cell_pmfs(g.h, c["alpha"].ctypes.data, c["beta"].ctypes.data, None, cc.ctypes.data, len(cc),
                                             rp2.ctypes.data, len(v), None, None, None, None, None, v.ctypes.data))
            assert np.array_equal(rp2, ptr) and np.array_equal(v, got["expected_log_variance"])
    g.close()


@pytest.fixture(scope="module")
def case2():
    coo = _case1_coo(huge=False)
    alpha, beta = S._alpha_beta(L1, 99)
    rng = np.random.default_rng(17)
    chunk = np.ones(L1, np.uint8)
    chunk[639:1278] = 0
    masks = {"none": None, "random 30 %": (rng.random(L1) >= 0.3).astype(np.uint8), "loci 639..1277": chunk, "all": np.zeros(L1, np.uint8)}
    refs = {k: tr.cell_reference(N1, *coo, alpha, beta, mask=m) for k, m in masks.items()}
    rp = np.concatenate([[0], np.cumsum(np.bincount(coo[1], minlength=N1))]).astype(np.uint64)
    return dict(coo=coo, alpha=alpha, beta=beta, masks=masks, refs=refs, rp=rp)


def test_mask(mods, case2):
    """no record at a masked locus; the counts are cell_log_likelihoods' loci_used under the same mask, exactly; the per-cell sums of
    log_pmf and expected_log_pmf (added here in longdouble) are that call's ll / expected_ll within tile_reference.cell_bound"""
    c = case2
    g = _load(mods, c["coo"])
    G = S._n_partials(g.engine_info().chunk_groups, L1, ()) if mods["engine"] == 2 else 6  # engine 1: a wave's six shuffle steps
    cells = np.arange(N1)
    for name, m in c["masks"].items():
        tag = f"engine {mods['engine']} mask '{name}'"
        got = g.cell_pmfs(cells, c["alpha"], c["beta"], m)
        ll, ell, nl = g.cell_log_likelihoods(c["alpha"], c["beta"], m)
        cnt = np.diff(got["rec_ptr"].astype(np.int64))
        assert np.array_equal(cnt.astype(np.float64), nl), tag
        assert np.array_equal(cnt, c["refs"][name]["count"]), tag
        if m is not None:
            assert (m[got["locus_index"]] != 0).all(), tag
        if name == "all":
            assert got["rec_ptr"][-1] == 0 and not ll.any() and not nl.any()
            continue
        row = np.repeat(cells, cnt)
        s_lp = np.zeros(N1, np.longdouble)
        s_e = np.zeros(N1, np.longdouble)
        np.add.at(s_lp, row, got["log_pmf"].astype(np.longdouble))
        np.add.at(s_e, row, got["expected_log_pmf"].astype(np.longdouble))
        b_ll, b_ell = tr.cell_bound(c["refs"][name], G)
        for what, s, dev, b in (("sum log_pmf", s_lp, ll, b_ll), ("sum expected_log_pmf", s_e, ell, b_ell)):
            d = np.abs((s - dev.astype(np.longdouble)).astype(np.float64))
            _, bad = _worst(tag, what + " against cell_log_likelihoods", d, b)
            assert bad.size == 0, (tag, what, bad[:5], d[bad[:5]], b[bad[:5]])
    g.close()


CFG1 = (2000, 1000, 0.10)


@pytest.fixture(scope="module")
def cfg1_coo():
    from cellector_amd import synth
    L, N, d = CFG1
    return [np.asarray(x, np.int64) for x in synth.generate_coo(L, N, d)]


def test_records_give_the_locus_pass(mods, cfg1_coo):
    """get_locus_log_likelihoods (main.rs:392-408) is a per-locus reduction of all_pmfs split by the exclusion set: the records of
    ALL cells under the alpha / beta / mask of an iteration at the fixed point, reduced here, are that iteration's locus outputs"""
    L, N, _ = CFG1
    g = _load(mods, cfg1_coo, L, N)
    sums = g.run()
    assert not sums[-1].any_change and len(sums) >= 2
    a, b = g.alpha_betas()
    used = g.loci_mask()
    s = g.em_iteration(5.0)
    assert not s.any_change and s.n_loci_filtered == 0
    lo = g.locus_outputs()
    exc = g.excluded() != 0
    assert exc.any()
    got = g.cell_pmfs(np.arange(N), a, b, used)
    cell = np.repeat(np.arange(N), np.diff(got["rec_ptr"].astype(np.int64)))
    mi = exc[cell]
    li = got["locus_index"].astype(np.int64)
    cnt = lambda sel, w=None: np.bincount(li[sel], weights=None if w is None else w[sel].astype(np.float64), minlength=L)
    assert np.array_equal(cnt(mi), lo["cells_min"]) and np.array_equal(cnt(~mi), lo["cells_maj"])
    for k, sel, w in (("alt_min", mi, got["alt"]), ("ref_min", mi, got["ref"]), ("alt_maj", ~mi, got["alt"]), ("ref_maj", ~mi, got["ref"])):
        assert np.array_equal(cnt(sel, w), lo[k].astype(np.float64)), k
    for k, sel in (("contrib_min", mi), ("contrib_maj", ~mi)):
        v = cnt(sel, got["log_pmf"])
        d = np.abs(v - lo[k]) / np.maximum(1.0, np.abs(lo[k]))
        print(f"  engine {mods['engine']}: {k} from the records, worst relative {d.max():.2e} (tolerance 1e-9)")
        assert (d <= 1e-9).all(), (k, np.nonzero(d > 1e-9)[0][:5])
    g.close()


def _summary(s):
    return (s.any_change, s.n_new_excluded, s.n_rescued, s.n_excluded, s.n_loci_filtered, s.median, s.iqr, s.threshold, s.n_near_threshold)


def test_nothing_is_disturbed(mods, cfg1_coo):
    """two ctxs run the same five iterations; one calls cell_pmfs and posterior_alpha_betas between every two: same bits"""
    L, N, _ = CFG1
    ga, gb = _load(mods, cfg1_coo, L, N), _load(mods, cfg1_coo, L, N)
    cells = np.array([0, 999, 17, 17, 512])
    for it in range(5):
        sa, sb = ga.em_iteration(5.0), gb.em_iteration(5.0)
        assert _summary(sa) == _summary(sb), it
        ca, cb = ga.cell_outputs(), gb.cell_outputs()
        for k in ca:
            assert np.array_equal(ca[k], cb[k]), (it, k)
        assert np.array_equal(ga.excluded(), gb.excluded()), it
        r = gb.cell_pmfs(cells)
        assert r["rec_ptr"][-1] == len(r["log_pmf"]) > 0
        for w in (0, 1, 2):
            gb.posterior_alpha_betas(w)
        gb.cell_pmfs(np.arange(N), *gb.posterior_alpha_betas(1), np.ones(L, np.uint8))
    pa, pb = ga.posteriors(), gb.posteriors()
    for k in pa:
        assert np.array_equal(pa[k], pb[k]), k
    ga.close(); gb.close()


def test_sharded(mods, case1):
    """three logical shards on one device: a list that crosses both shard borders in both directions gives the single-device call's
    arrays to the bit, in list order; posterior_alpha_betas is shard 0's, the same"""
    from cellector_amd import Cellector
    c = case1
    g = _load(mods, c["coo"])
    m = Cellector(devices=[0, 0, 0])
    m.set_option("engine", mods["engine"])
    m.load_coo(L1, N1, *S._u32(c["coo"]), 0, 0)
    b = [int(x) for x in m.partition()]
    assert len(b) == 4 and 0 < b[1] < b[2] < N1
    cells = np.array([b[1] - 1, b[1], b[2], b[2] - 1, b[1] + 1, b[1] - 2, N1 - 1, 0, 26, b[2] + 3, 26, b[1]])
    mask = (np.random.default_rng(3).random(L1) >= 0.2).astype(np.uint8)
    for mk in (None, mask):
        one, many = g.cell_pmfs(cells, c["alpha"], c["beta"], mk), m.cell_pmfs(cells, c["alpha"], c["beta"], mk)
        for k in one:
            assert np.array_equal(one[k], many[k]), k
        assert one["rec_ptr"][-1] > 2100
    empty = m.cell_pmfs(np.zeros(0, np.int64), c["alpha"], c["beta"])
    assert list(empty["rec_ptr"]) == [0]
    # (an exclusion set placed, not iterated to: engine 1's cell pass folds the total-65535 entry's 65536 log-pmfs one by one)
    flags = (np.random.default_rng(8).random(N1) < 0.1).astype(np.uint8)
    g.set_excluded(flags); m.set_excluded(flags)
    assert np.array_equal(g.excluded(), m.excluded()) and g.excluded().sum() == flags.sum() > 0
    for w in (0, 1, 2):
        for x, y in zip(g.posterior_alpha_betas(w), m.posterior_alpha_betas(w)):
            assert np.array_equal(x, y), w
    with pytest.raises(mods["ffi"].CellectorError) as e:
        m.cell_pmfs([N1], c["alpha"], c["beta"])
    assert e.value.status == 1 and str(N1) in str(e.value)
    g.close(); m.close()


def test_refusals(mods, case2):
    c = case2  # (without the total-65535 entry: the em_begin below is engine 1's cell pass as well)
    ffi = mods["ffi"]
    g = mods["Cellector"](0)
    with pytest.raises(ffi.CellectorError) as e:  # before a load
        g.cell_pmfs([0], np.ones(4), np.ones(4))
    assert e.value.status == 1
    with pytest.raises(ffi.CellectorError) as e:
        g.posterior_alpha_betas(0)
    assert e.value.status == 1
    g.close()
    g = _load(mods, c["coo"])
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    alpha, beta = c["alpha"], c["beta"]
    # id == N: EINVAL, the message names it, nothing was written
    cells = np.array([3, N1, 5], np.uint32)
    rp = np.full(4, 12345, np.uint64)
    cols_u = [np.full(8, 777, np.uint32) for _ in range(3)]
    cols_f = [np.full(8, -7.5) for _ in range(3)]
    st = g._lib.cellector_cell_pmfs(g.h, p(alpha), p(beta), None, p(cells), 3, p(rp), 8, *[p(x) for x in cols_u + cols_f])
    assert st == 1 and str(N1) in g._lib.cellector_last_error(g.h).decode()
    assert (rp == 12345).all() and all((x == 777).all() for x in cols_u) and all((x == -7.5).all() for x in cols_f)
    # capacity one short: EINVAL, rec_ptr correct
    cells = np.array([26, 22, 21], np.uint32)
    _, want = _rows(c["rp"], cells)
    rp = np.zeros(4, np.uint64)
    n = int(want[-1])
    lp = np.zeros(n, np.float64)
    st = g._lib.cellector_cell_pmfs(g.h, p(alpha), p(beta), None, p(cells), 3, p(rp), n - 1, None, None, None, p(lp), None, None)
    assert st == 1 and np.array_equal(rp, want)
    st = g._lib.cellector_cell_pmfs(g.h, p(alpha), p(beta), None, p(cells), 3, p(rp), n, None, None, None, p(lp), None, None)
    assert st == 0 and np.array_equal(lp, g.cell_pmfs(cells, alpha, beta)["log_pmf"]) and lp.any()
    with pytest.raises(ffi.CellectorError):
        g.posterior_alpha_betas(3)
    # between em_begin and em_finish
    g.em_begin()
    for call in (lambda: g.cell_pmfs([0], alpha, beta), lambda: g.posterior_alpha_betas(0)):
        with pytest.raises(ffi.CellectorError) as e:
            call()
        assert e.value.status == 1 and "in flight" in str(e.value)
    g.em_threshold(5.0)
    with pytest.raises(ffi.CellectorError):
        g.cell_pmfs([0], alpha, beta)
    g.em_finish()
    assert g.cell_pmfs([0], alpha, beta)["rec_ptr"][-1] == c["rp"][1]
    g.close()


def test_posterior_alpha_betas(mods, cfg1_coo):
    """the three pairs to the bit against numpy in the reference's operation order (main.rs:239-254; the counts are whole numbers in
    f64 and the library is built with -ffp-contract=off: the same operations give the same bits); the cell pass under the minority
    and the majority pair against posteriors()' sums: each within tile_reference.cell_bound of the reference"""
    import test_gpu_fullsize as F
    L, N, _ = CFG1
    g = _load(mods, cfg1_coo, L, N)
    g.run()
    lc = g.locus_counts()
    a_em, b_em = g.alpha_betas()
    n_exc = int((g.excluded() != 0).sum())
    alt_min, ref_min = (lc[:, 1] + 1.0) - a_em, (lc[:, 0] + 1.0) - b_em  # (whole numbers: exact)
    want = F._posterior_alpha_betas(lc, alt_min, ref_min, n_exc, N)[:3]
    got = [g.posterior_alpha_betas(w) for w in (0, 1, 2)]
    for w in range(3):
        assert np.array_equal(got[w][0], want[w][0]) and np.array_equal(got[w][1], want[w][1]), w
    post = g.posteriors()
    G = S._n_partials(g.engine_info().chunk_groups, L, ()) if mods["engine"] == 2 else 6
    for w, name in ((0, "ll_minority"), (1, "ll_majority")):
        ref = tr.cell_reference(N, *cfg1_coo, *got[w])
        bound = tr.cell_bound(ref, G)[0] + 0.5 * np.spacing(np.abs(ref["ll"]))
        for what, v in (("cell_log_likelihoods", g.cell_log_likelihoods(*got[w])[0]), ("posteriors", post[name])):
            d = np.abs(v - ref["ll"])
            _, bad = _worst(f"engine {mods['engine']} {name}", what, d, bound)
            assert bad.size == 0, (name, what, bad[:5])
    g.close()
