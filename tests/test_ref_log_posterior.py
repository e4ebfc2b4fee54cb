"""CPU checks behind option resolve_posteriors: ref_log.h and assign_host.h compiled as plain C++ on the host.

The posterior phase's alpha/beta are NOT integers (main.rs:245-253 scales the majority tallies by the minority fraction), unlike
the EM loop's, so ref_log_bb_pmf is compared with the oracle's orc_log_beta_binomial_pmf bit for bit on such arguments; and the
last steps cellector_assign runs on the host (assign_host.h: main.rs:266-278 and the rule of main.rs:145-169) are compared with
the oracle's on random LL triples.  Zero mismatches are expected; a mismatch names its arguments.
"""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cellector_amd", "csrc")

DRIVER = r"""
#include <cmath>
#include <cstdint>
#include "ref_log.h"
#include "assign_host.h"

static double g_lf[171];
static bool g_lf_ready = false;
static void lf_init()
{
    // the library's ln-factorial table: statrs' FCACHE running product, the host's log (ctx_core.cpp)
    if (g_lf_ready) return;
    double f = 1.0;
    g_lf[0] = std::log(1.0);
    for (int i = 1; i < 171; i++) { f *= (double)i; g_lf[i] = std::log(f); }
    g_lf_ready = true;
}

extern "C" void log_bb_pmf_batch(const uint32_t *a, const uint32_t *r, const double *alpha, const double *beta, int64_t n,
                                 double *out)
{
    lf_init();
    for (int64_t i = 0; i < n; i++) out[i] = ref_log_bb_pmf(g_lf, alpha[i], beta[i], a[i], r[i]);
}

extern "C" void assign_batch(const double *ll3 /*[3][n] min | maj | dbl*/, int64_t n, double lp_min, double lp_maj, double lp_dbl,
                             const uint32_t *n_entries, double threshold, uint64_t min_loci, double *posterior, double *doublet,
                             uint8_t *label, uint64_t *qual)
{
    for (int64_t i = 0; i < n; i++) {
        assign_posterior(ll3[i], ll3[n + i], ll3[2 * n + i], lp_min, lp_maj, lp_dbl, &posterior[i], &doublet[i]);
        label[i] = assign_label(posterior[i], doublet[i], n_entries[i], threshold, min_loci);
        qual[i] = assign_qual(posterior[i]);
    }
}
"""


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    if not cxx:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("ref_log_posterior")
    src, so = d / "driver.cpp", d / "libdrv.so"
    src.write_text(DRIVER)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fno-fast-math", "-ffp-contract=off", "-fPIC", "-shared",
                           "-I", CSRC, str(src), "-o", str(so), "-lm"])
    L = C.CDLL(str(so))
    vp, i64, d_ = C.c_void_p, C.c_int64, C.c_double
    L.log_bb_pmf_batch.restype = None
    L.log_bb_pmf_batch.argtypes = [vp, vp, vp, vp, i64, vp]
    L.assign_batch.restype = None
    L.assign_batch.argtypes = [vp, i64, d_, d_, d_, vp, d_, C.c_uint64, vp, vp, vp, vp]
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_ref_log_bb_pmf_equals_oracle_on_posterior_phase_alpha_beta(drv, oracle_lib):
    """alpha, beta formed as calculate_posteriors forms them: (A - 1) mf + 1 (majority set) and (A - 1) mf + (B - 1) + 1
    (doublet set) for integer A, B in 1 .. 2e6 and mf in [0.0005, 0.35]."""
    L = oracle_lib.lib()
    rng = np.random.default_rng(20261016)
    n = 100_000

    def tallies():
        return np.floor(np.exp(rng.uniform(0.0, np.log(2e6), n))).astype(np.float64)

    mf = rng.uniform(0.0005, 0.35, n)
    a_maj, b_maj, a_min, b_min = tallies(), tallies(), tallies(), tallies()
    dbl = np.arange(n) % 2 == 1
    al = np.where(dbl, (a_maj - 1.0) * mf + (a_min - 1.0) + 1.0, (a_maj - 1.0) * mf + 1.0)
    be = np.where(dbl, (b_maj - 1.0) * mf + (b_min - 1.0) + 1.0, (b_maj - 1.0) * mf + 1.0)
    assert al.min() >= 1.0 and be.min() >= 1.0 and np.mean(al != np.round(al)) > 0.9
    a = rng.integers(0, 41, n).astype(np.uint32)
    r = rng.integers(0, 41, n).astype(np.uint32)
    a[:300] = rng.integers(100, 65536, 300)  # a few deep counts: ln C beyond the factorial table
    r[150:450] = rng.integers(100, 65536, 300)
    a[450], r[450], a[451], r[451] = 65535, 65535, 0, 0
    got = np.empty(n)
    drv.log_bb_pmf_batch(_p(a), _p(r), _p(al), _p(be), n, _p(got))
    f, lnb = L.orc_log_beta_binomial_pmf, L.orc_ln_binomial
    want = np.array([f(float(x), float(y), p, q, lnb(int(x) + int(y), int(x))) for x, y, p, q in zip(a, r, al, be)])
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    assert bad.size == 0, "%d mismatches; ref_log_bb_pmf != oracle at (a, r, alpha, beta) = %s" % (bad.size, [
        (int(a[i]), int(r[i]), float(al[i]).hex(), float(be[i]).hex()) for i in bad[:8]])


def _oracle_chain(L, s_min, s_maj, s_dbl, lp_min, lp_maj, lp_dbl):
    """orc_posteriors' last loop (main.rs:266-278) for one cell, with the oracle's logsumexp and the C library's exp."""
    log_num = lp_min + s_min
    log_den = L.orc_logsumexp(log_num, lp_maj + s_maj)
    log_dbl = lp_dbl + s_dbl
    log_den = L.orc_logsumexp(log_den, log_dbl)
    return math.exp(log_num - log_den), math.exp(log_dbl - log_den)


def test_host_chain_and_rule_equal_the_oracles(drv, oracle_lib):
    """Three LLs in -> posterior, doublet posterior, label and qual: assign_host.h against the oracle on 1e5 triples, with
    saturated cells (1 - post == 0: qual 255, no NaN), cells between, and thresholds within an ulp of a cell's posterior."""
    from cellector_amd import synth
    L = oracle_lib.lib()
    N = 2000
    lo, ce, al, re = synth.generate_coo(300, N, 0.15, seed=3, minority_fraction=0.3)
    o = oracle_lib.Oracle.from_coo(300, N, lo, ce, al, re)
    o.em_iteration(5.0)
    ent = o.entries_per_cell()
    assert ent.min() < 30 < ent.max()
    rng = np.random.default_rng(5)
    mf = 0.07
    lp_min, lp_maj, lp_dbl = math.log(mf), math.log(1.0 - mf), math.log(N / 1000.0 / 100.0 * max(mf, 0.1))
    seen = set()
    for batch in range(50):
        base = -rng.uniform(1.0, 3000.0, N)
        # differences from 1e-3 to 60 nats either way: posteriors from saturated to the middle
        gap = lambda: rng.choice([-1.0, 1.0], N) * np.exp(rng.uniform(np.log(1e-3), np.log(60.0), N))  # noqa: E731
        ll3 = np.ascontiguousarray(np.stack([base, base + gap(), base + gap() - rng.uniform(0.0, 30.0, N)]))
        if batch == 0:
            ll3[:, :4] = [[-10.0, -2000.0, -100.0, 0.0], [-2000.0, -10.0, -100.0, 0.0], [-3000.0, -3000.0, -10.0, 0.0]]
        want_p = np.empty(N)
        want_d = np.empty(N)
        for i in range(N):
            want_p[i], want_d[i] = _oracle_chain(L, ll3[0, i], ll3[1, i], ll3[2, i], lp_min, lp_maj, lp_dbl)
        mid = np.flatnonzero((want_p > 0.5) & (want_p < 1.0))
        T = 0.999
        if batch % 3 == 1 and mid.size:
            T = float(want_p[mid[0]])
        elif batch % 3 == 2 and mid.size:
            T = float(np.nextafter(want_p[mid[-1]], 0.0))
        p, d = np.empty(N), np.empty(N)
        lab, q = np.empty(N, np.uint8), np.empty(N, np.uint64)
        drv.assign_batch(_p(ll3), N, lp_min, lp_maj, lp_dbl, _p(ent), T, 30, _p(p), _p(d), _p(lab), _p(q))
        assert np.array_equal(p.view(np.uint64), want_p.view(np.uint64)), batch
        assert np.array_equal(d.view(np.uint64), want_d.view(np.uint64)), batch
        wl, _, wq = o.assignments(want_p, want_d, T, 30)
        assert np.array_equal(lab, wl) and np.array_equal(q, wq), batch
        assert not np.isnan(p).any() and q.max() <= 255
        seen |= set(np.unique(lab).tolist())
        if batch == 0:
            assert p[0] == 1.0 and q[0] == 255 and p[1] == 0.0 and q[1] == 255 and d[2] > 0.5
    assert seen == {0, 1, 2, 3}
    o.close()
