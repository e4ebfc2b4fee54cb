"""GPU: expected_log_variances, the fourth per-cell vector of get_cell_log_likelihoods (main.rs:541-591, :587) —
cellector_cell_log_variances, option cell_variance / cellector_iter_cell_variances — and option normalization = 1, the z-score of
main.rs:317-318, on both engines (the pass runs over the by-cell CSR both keep).

Matrix A is tests/test_gpu_cell_pmfs.py's value matrix (1400 loci x 1500 cells, ~42k entries, min_alt = min_ref = 0): rows of 0, 1,
63, 64, 65, 129 and 2100 entries (the row pass strides a row in 64-entry steps, four steps at a time), totals 0..25 on both sides
of the table's last slot 17, a 0/0 entry, a pair listed three times, single entries of total 80, 300 and 65535 at loci 702..704
for the whole-wave path.  Matrix B is synth.generate_coo(2000, 1000, 0.10) with min_alt = min_ref = 4.

Bounds (u = 2^-53; nothing fitted).  A cell's value is a sum of its entries' variances, each within pmf_reference's b_variance of
the reference (which includes half an ulp of the reference's rounding to double), so B = the sum of the row's b_variance over the
unmasked entries.  The device's own additions on a row of k entries (masked ones included: they add the table's zero): a lane adds
at most ceil(k / 64) terms, then wave_sum's six steps; every term is >= 0, so every partial sum is at most the whole, i.e. at most
V + B, and each addition errs by at most u (V + B).  Plus half an ulp of V for the rounding of the longdouble reference sum to
double:

    |device - reference| <= B + (ceil(k / 64) + 6) u (V + B) + ulp(V) / 2.

test_agrees_with_the_records compares with the DEVICE's own records (cellector_cell_pmfs' column, added here in longdouble): the
table holds those bits, so only the additions remain: (ceil(k / 64) + 6) u S + ulp(S) / 2 with S the records' sum.

Worst observed / bound ratios are printed (pytest -s).
"""
import math

import numpy as np
import pytest

import pmf_reference as pr
import test_gpu_cell_pmfs as P
import test_gpu_tile_sweep as S
from test_gpu_parity import mods  # noqa: F401  (both engines)

pytestmark = pytest.mark.gpu

L1, N1 = P.L1, P.N1
U = 2.0 ** -53
LB, NB, DB = 2000, 1000, 0.10  # matrix B
LD = np.longdouble


def _row_sums(n_rows, rows, values):
    s = np.zeros(n_rows, LD)
    np.add.at(s, rows, np.asarray(values).astype(LD))
    return s


def _add_bound(k, total):
    """the device's additions on rows of k entries whose partial sums are at most `total`, plus the rounding of a longdouble sum"""
    return (np.ceil(k / 64.0) + 6.0) * U * total


@pytest.fixture(scope="module")
def case_a(oracle_lib):
    coo = P._case1_coo()
    alpha, beta = S._alpha_beta(L1, 99)
    order = P._csr_order(coo)
    lo, ce, al, re = (x[order] for x in coo)
    k = np.bincount(ce, minlength=N1).astype(np.float64)
    assert [int(k[c]) for c in P.PLANTED] == list(P.PLANTED.values())
    n = al + re
    assert n.min() == 0 and (n == 17).any() and (n == 18).any() and {80, 300, 65535} <= set(n.tolist())
    rec = pr.records(alpha, beta, lo, al, re)
    key = lo * (1 << 20) + n
    uk, inv = np.unique(key, return_inverse=True)
    o_v = np.array([oracle_lib.expected_log_pmf(int(q & 0xFFFFF), float(alpha[q >> 20]), float(beta[q >> 20]))[1] for q in uk])[inv]
    rng = np.random.default_rng(17)
    chunk = np.ones(L1, np.uint8)
    chunk[639:1278] = 0  # (covers loci 702..704: the three entries above the table must add nothing)
    masks = {"none": None, "random 30 %": (rng.random(L1) >= 0.3).astype(np.uint8), "loci 639..1277": chunk, "all": np.zeros(L1, np.uint8)}
    return dict(coo=coo, alpha=alpha, beta=beta, lo=lo, ce=ce, n=n, k=k, rec=rec, o_v=o_v, masks=masks)


def _worst(tag, what, diff, bound):
    ok = bound > 0
    r = float((diff[ok] / bound[ok]).max()) if ok.any() else 0.0
    print(f"  {tag}: {what} worst |device - reference| / bound = {r:.3f} (largest bound {bound.max():.2e})")
    return np.nonzero(diff > bound)[0]


def test_values(mods, case_a):
    """cell_log_variances under four masks against the longdouble row sums of pmf_reference.records' variance, within
    B + (ceil(k / 64) + 6) u (V + B) + ulp(V) / 2 (module docstring); exact zeros for the all-masked mask and the empty row"""
    c = case_a
    g = P._load(mods, c["coo"])
    for name, m in c["masks"].items():
        tag = f"engine {mods['engine']} mask '{name}'"
        got = g.cell_log_variances(c["alpha"], c["beta"], m)
        assert got.shape == (N1,) and np.isfinite(got).all(), tag
        assert got[20] == 0.0 and c["k"][20] == 0, tag  # the empty row
        if name == "all":
            assert not got.any(), tag
            continue
        keep = np.ones(len(c["lo"]), bool) if m is None else m[c["lo"]] != 0
        v_ld = _row_sums(N1, c["ce"][keep], c["rec"]["variance"][keep])
        v = v_ld.astype(np.float64)
        b = _row_sums(N1, c["ce"][keep], c["rec"]["b_variance"][keep]).astype(np.float64)
        bound = b + _add_bound(c["k"], v + b) + 0.5 * np.spacing(v)
        d = np.abs((got.astype(LD) - v_ld).astype(np.float64))
        bad = _worst(tag, "expected_log_variance", d, bound)
        assert bad.size == 0, (tag, bad[:5], got[bad[:5]], v[bad[:5]], bound[bad[:5]], c["k"][bad[:5]])
        assert (got > 0).sum() > N1 // 2, tag
    # the three entries above the table at masked loci add nothing: their rows under the chunk mask hold table terms only
    chunk = g.cell_log_variances(c["alpha"], c["beta"], c["masks"]["loci 639..1277"])
    none = g.cell_log_variances(c["alpha"], c["beta"], None)
    for cell in (P.MID[1], P.BIG[1], P.HUGE[1]):
        assert chunk[cell] < none[cell], cell
    g.close()


def test_agrees_with_the_records(mods, case_a):
    """per-row longdouble sums of the device's own cell_pmfs()["expected_log_variance"] against cell_log_variances, within the
    additions alone: (ceil(k / 64) + 6) u S + ulp(S) / 2 — a wrong table index or stride moves a value by far more"""
    c = case_a
    g = P._load(mods, c["coo"])
    cells = np.arange(N1)
    for name in ("none", "random 30 %"):
        m = c["masks"][name]
        tag = f"engine {mods['engine']} mask '{name}'"
        recs = g.cell_pmfs(cells, c["alpha"], c["beta"], m)
        rows = np.repeat(cells, np.diff(recs["rec_ptr"].astype(np.int64)))
        s_ld = _row_sums(N1, rows, recs["expected_log_variance"])
        s = s_ld.astype(np.float64)
        got = g.cell_log_variances(c["alpha"], c["beta"], m)
        bound = _add_bound(c["k"], s) + 0.5 * np.spacing(s)
        d = np.abs((got.astype(LD) - s_ld).astype(np.float64))
        bad = _worst(tag, "against the device's records", d, bound)
        assert bad.size == 0, (tag, bad[:5], got[bad[:5]], s[bad[:5]], bound[bad[:5]])
        assert np.array_equal(got == 0.0, s == 0.0), tag
    g.close()


def test_oracle_cross_check(mods, case_a):
    """against the oracle's variance per distinct (locus, total), summed per row: relative 1e-7 max(1, |v|)"""
    c = case_a
    g = P._load(mods, c["coo"])
    got = g.cell_log_variances(c["alpha"], c["beta"], None)
    want = _row_sums(N1, c["ce"], c["o_v"]).astype(np.float64)
    d = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"  engine {mods['engine']}: expected_log_variance against the oracle, worst relative {d.max():.2e} (tolerance 1e-7)")
    assert (d <= 1e-7).all(), np.nonzero(d > 1e-7)[0][:5]
    g.close()


# ---- matrix B: the loop ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def coo_b():
    from cellector_amd import synth
    return [np.asarray(x, np.int64) for x in synth.generate_coo(LB, NB, DB)]


def _r8(keys, mult=5.0):
    """median, iqr, threshold of statrs' Data (R-8 quartiles), the numpy restatement tests/test_gpu_fullsize.py uses"""
    srt = np.sort(keys)
    n = len(srt)
    k = n // 2
    med = srt[k] if n % 2 else (srt[k - 1] + srt[k]) / 2.0
    h1, h3 = (n + 1.0 / 3.0) * 0.25 + 1.0 / 3.0, (n + 1.0 / 3.0) * 0.75 + 1.0 / 3.0
    q1 = srt[int(h1) - 1] + (h1 - int(h1)) * (srt[int(h1)] - srt[int(h1) - 1])
    q3 = srt[int(h3) - 1] + (h3 - int(h3)) * (srt[int(h3)] - srt[int(h3) - 1])
    return med, q3 - q1, q1 - mult * (q3 - q1)


_lgamma = np.vectorize(math.lgamma, otypes=[np.float64])


def _restate_zscore_loop(coo, n_loci, n_cells, min_alt, min_ref, mult, max_iter=6):
    """The reference's loop (main.rs:36-50, :308-347) with the z-score of main.rs:317-318 as the key, in double precision numpy:
    per iteration (threshold, new exclusion flags, keys)."""
    lo, ce, al, re = coo
    used = (np.bincount(lo[re > 0], minlength=n_loci) >= min_ref) & (np.bincount(lo[al > 0], minlength=n_loci) >= min_alt)
    e_used = used[lo]  # load_data.rs:254-280: only entries at used loci are kept
    lo, ce, al, re = lo[e_used], ce[e_used], al[e_used], re[e_used]
    n = al + re
    s_alt = np.bincount(lo, weights=al, minlength=n_loci)
    s_ref = np.bincount(lo, weights=re, minlength=n_loci)
    mask = np.ones(n_loci, bool)
    excluded = np.zeros(n_cells, bool)
    out = []
    for _ in range(max_iter):
        x = excluded[ce]
        alpha = (s_alt + 1.0) - np.bincount(lo[x], weights=al[x], minlength=n_loci)  # main.rs:598-611
        beta = (s_ref + 1.0) - np.bincount(lo[x], weights=re[x], minlength=n_loci)
        lp, ex, va = np.zeros(len(lo)), np.zeros(len(lo)), np.zeros(len(lo))
        for tot in np.unique(n):  # per total: the tot + 1 log-pmfs of every entry with it (stats.rs:8-33, :41-53)
            sel = np.nonzero(n == tot)[0]
            a_, b_ = alpha[lo[sel]][:, None], beta[lo[sel]][:, None]
            ks = np.arange(tot + 1, dtype=np.float64)[None, :]
            t = (_lgamma(tot + 1.0) - _lgamma(ks + 1.0) - _lgamma(tot - ks + 1.0)) + (_lgamma(ks + a_) + _lgamma(tot - ks + b_)
                 - _lgamma(tot + a_ + b_)) - (_lgamma(a_) + _lgamma(b_) - _lgamma(a_ + b_))
            e = np.log(np.exp(2.0 * t).sum(axis=1))
            lp[sel] = t[np.arange(len(sel)), al[sel]]
            ex[sel] = e
            va[sel] = (np.exp(t) * (t - e[:, None]) ** 2).sum(axis=1)
        live = mask[lo]
        ll = np.bincount(ce[live], weights=lp[live], minlength=n_cells)
        ell = np.bincount(ce[live], weights=ex[live], minlength=n_cells)
        var = np.bincount(ce[live], weights=va[live], minlength=n_cells)
        cnt = np.bincount(ce[live], minlength=n_cells)
        ok = (cnt > 0) & (var > 0)
        z = np.where(ok, (ll - ell) / np.sqrt(np.where(ok, var, 1.0)), 0.0)
        med, iqr, thr = _r8(z, mult)
        new = z < thr
        out.append(dict(threshold=thr, median=med, iqr=iqr, excluded=new, keys=z, n_new=int((new & ~excluded).sum()),
                        n_rescued=int((excluded & ~new).sum())))
        mi = live & new[ce]  # main.rs:368-451: the -80 filter on the new minority's per-cell contribution
        c_min = np.bincount(lo[mi], weights=lp[mi], minlength=n_loci)
        n_min = np.bincount(lo[mi], minlength=n_loci)
        mask = mask & ~((n_min > 0) & (c_min / np.maximum(n_min, 1) < -80.0))
        changed = out[-1]["n_new"] > 0 or out[-1]["n_rescued"] > 0
        excluded = new
        if not changed:
            break
    return out


def _load_b(mods, coo, opts=()):
    g = mods["Cellector"](0)
    for k, v in opts:
        g.set_option(k, v)
    g.load_coo(LB, NB, *S._u32(coo), 4, 4)
    return g


def test_zscore_iteration(mods, coo_b):
    """option normalization = 1, iteration by iteration until no change: the keys are (ll - ell) / sqrt(var) of the device's own
    columns within 4 ulp (0 where loci_used or var is 0), the summary is the R-8 statistics of those keys exactly, the flags are
    keys < threshold exactly, cell_variances() is cell_log_variances under the iteration's alpha / beta / mask to the bit, and the
    trajectory is the double-precision numpy restatement's: 47 cells excluded in iteration 1, no change in iteration 2, thresholds
    within 1e-6 relative (-4.5167, -7.4088), and, no cell of the restatement lying within 1e-6 max(1, |threshold|) of a threshold,
    the same flags for every cell"""
    want = _restate_zscore_loop(coo_b, LB, NB, 4, 4, 5.0)
    assert len(want) == 2 and (want[0]["n_new"], want[0]["n_rescued"]) == (47, 0) and (want[1]["n_new"], want[1]["n_rescued"]) == (0, 0)
    assert abs(want[0]["threshold"] + 4.5167) < 1e-4 and abs(want[1]["threshold"] + 7.4088) < 1e-4
    for w in want:  # the condition under which every cell's flag can be compared
        assert np.abs(w["keys"] - w["threshold"]).min() > 1e-6 * max(1.0, abs(w["threshold"]))
    g = _load_b(mods, coo_b, [("normalization", 1)])
    for it in range(len(want) + 1):
        a, b = g.alpha_betas()
        used = g.loci_mask()
        s = g.em_iteration(5.0)
        co = g.cell_outputs()
        var = g.cell_variances()
        ok = (co["loci_used"] > 0) & (var > 0)
        z = np.where(ok, (co["ll"] - co["expected_ll"]) / np.sqrt(np.where(ok, var, 1.0)), 0.0)
        ulps = np.abs(co["normalized"] - z) / np.spacing(np.abs(z))
        print(f"  engine {mods['engine']} iteration {it + 1}: keys against numpy's quotient, worst {ulps.max():.2f} ulp; threshold {s.threshold!r}")
        assert (ulps <= 4.0).all() and not co["normalized"][~ok].any(), it
        assert (s.median, s.iqr, s.threshold) == _r8(co["normalized"]), it
        assert np.array_equal(g.excluded(), (co["normalized"] < s.threshold).astype(np.uint8)), it
        assert np.array_equal(var, g.cell_log_variances(a, b, used)), it
        w = want[it]
        assert (s.n_new_excluded, s.n_rescued) == (w["n_new"], w["n_rescued"]), it
        assert abs(s.threshold - w["threshold"]) <= 1e-6 * abs(w["threshold"]), (it, s.threshold, w["threshold"])
        assert np.array_equal(g.excluded() != 0, w["excluded"]), it
        if not s.any_change:
            break
    assert it == 1 and not s.any_change and s.n_excluded == 47
    g.close()


def test_default_is_not_disturbed(mods, coo_b):
    """two ctxs run the same five iterations, one with cell_variance = 1 (normalization 0) and a cell_log_variances call between
    every two: summaries, cell outputs, flags and posteriors are the same bits; the plain ctx refuses cell_variances()"""
    ga, gb = _load_b(mods, coo_b), _load_b(mods, coo_b, [("cell_variance", 1)])
    ones = np.ones(ga.dims().loci_used, np.uint8)
    for it in range(5):
        a, b = gb.alpha_betas()
        used = gb.loci_mask()
        sa, sb = ga.em_iteration(5.0), gb.em_iteration(5.0)
        assert P._summary(sa) == P._summary(sb), it
        ca, cb = ga.cell_outputs(), gb.cell_outputs()
        assert sorted(ca) == ["expected_ll", "ll", "loci_used", "normalized"]
        for k in ca:
            assert np.array_equal(ca[k], cb[k]), (it, k)
        assert np.array_equal(ga.excluded(), gb.excluded()), it
        var = gb.cell_variances()
        assert (var > 0).all() and np.array_equal(var, gb.cell_log_variances(a, b, used)), it
        gb.cell_log_variances(*gb.posterior_alpha_betas(1), ones)
        with pytest.raises(mods["ffi"].CellectorError) as e:
            ga.cell_variances()
        assert e.value.status == 1 and "not formed" in str(e.value)
    pa, pb = ga.posteriors(), gb.posteriors()
    for k in pa:
        assert np.array_equal(pa[k], pb[k]), k
    gb.em_reset()  # ... and after a reset until an iteration has finished
    with pytest.raises(mods["ffi"].CellectorError) as e:
        gb.cell_variances()
    assert e.value.status == 1
    gb.em_iteration(5.0)
    assert (gb.cell_variances() > 0).all()
    ga.close(); gb.close()


def test_sharded(mods, case_a, coo_b):
    """three logical shards on one device against one device: cell_log_variances on matrix A to the bit; on matrix B with
    bank_order 0 and normalization 1 the iteration summaries, cell_variances() and excluded() to the bit"""
    from cellector_amd import Cellector
    c = case_a
    g = P._load(mods, c["coo"])
    m = Cellector(devices=[0, 0, 0])
    m.set_option("engine", mods["engine"])
    m.load_coo(L1, N1, *S._u32(c["coo"]), 0, 0)
    assert len(m.partition()) == 4
    for mk in (None, c["masks"]["random 30 %"]):
        assert np.array_equal(g.cell_log_variances(c["alpha"], c["beta"], mk), m.cell_log_variances(c["alpha"], c["beta"], mk))
    g.close(); m.close()
    g = _load_b(mods, coo_b, [("bank_order", 0), ("normalization", 1)])
    m = Cellector(devices=[0, 0, 0])
    for k, v in (("engine", mods["engine"]), ("bank_order", 0), ("normalization", 1)):
        m.set_option(k, v)
    m.load_coo(LB, NB, *S._u32(coo_b), 4, 4)
    for it in range(3):
        sg, sm = g.em_iteration(5.0), m.em_iteration(5.0)
        assert P._summary(sg) == P._summary(sm), it
        assert np.array_equal(g.cell_variances(), m.cell_variances()), it
        assert np.array_equal(g.excluded(), m.excluded()), it
        assert np.array_equal(g.cell_outputs()["normalized"], m.cell_outputs()["normalized"]), it
    assert sg.n_excluded == 47
    g.close(); m.close()


def test_refusals(mods, coo_b):
    ffi = mods["ffi"]
    g = mods["Cellector"](0)
    for call in (lambda: g.cell_log_variances(np.ones(4), np.ones(4)), lambda: g.cell_variances()):  # before a load
        with pytest.raises(ffi.CellectorError) as e:
            call()
        assert e.value.status == 1
    g.close()
    g = _load_b(mods, coo_b)
    a, b = g.alpha_betas()
    g.em_begin()
    with pytest.raises(ffi.CellectorError) as e:  # between em_begin and em_finish
        g.cell_log_variances(a, b)
    assert e.value.status == 1 and "in flight" in str(e.value)
    g.em_threshold(5.0)
    with pytest.raises(ffi.CellectorError) as e:
        g.cell_log_variances(a, b)
    assert e.value.status == 1 and "in flight" in str(e.value)
    g.em_finish()
    assert (g.cell_log_variances(a, b) > 0).all()

    def refused(key, value, *names):
        with pytest.raises(ffi.CellectorError) as e:
            g.set_option(key, value)
        assert e.value.status == 1 and all(n in str(e.value) for n in names), str(e.value)

    refused("normalization", 2, "normalization")
    refused("normalization", -1, "normalization")
    # against resolve_ties, both orders (resolve_ties 1 after this ingest is refused for its own reason: set on a fresh ctx)
    g.close()
    g = mods["Cellector"](0)
    g.set_option("resolve_ties", 1)
    refused("normalization", 1, "normalization", "resolve_ties")
    g.set_option("resolve_ties", 0)
    g.set_option("normalization", 1)
    refused("resolve_ties", 1, "normalization", "resolve_ties")
    g.set_option("resolve_posteriors", 1)  # independent
    g.set_option("resolve_posteriors", 0)
    # against compute_expected, both orders
    refused("compute_expected", 0, "normalization", "compute_expected")
    g.set_option("normalization", 0)
    g.set_option("compute_expected", 0)
    refused("normalization", 1, "normalization", "compute_expected")
    g.set_option("compute_expected", 1)
    # the ctx is usable afterwards: the z-score loop
    g.set_option("normalization", 1)
    g.load_coo(LB, NB, *S._u32(coo_b), 4, 4)
    s = g.em_iteration(5.0)
    assert s.n_new_excluded == 47 and (g.cell_variances() > 0).all()
    g.close()
