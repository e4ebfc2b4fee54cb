"""ref_log.h compiled as plain C++ on the host (CPU): ref_log bit for bit against the C library's log, and ref_log_bb_pmf
against the CPU oracle's orc_log_beta_binomial_pmf (the reference's arithmetic with the C library's log).

Option resolve_ties evaluates the cells next to an order statistic or the threshold with these functions on the device and
promises the reference's bits; that holds where ref_log equals the C library's log.  Zero mismatches are expected; a
mismatch names its argument.
"""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cellector_amd", "csrc")
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "math_kat.json")))

DRIVER = r"""
#include <cmath>
#include <cstdint>
#include <cstring>
#include "ref_log.h"

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

extern "C" int64_t ref_log_mismatches(const double *x, int64_t n, double *bad, int64_t max_bad)
{
    int64_t nb = 0;
    for (int64_t i = 0; i < n; i++) {
        const double a = ref_log(x[i]), b = std::log(x[i]);
        if (std::memcmp(&a, &b, 8) != 0) {
            if (nb < max_bad) bad[nb] = x[i];
            nb++;
        }
    }
    return nb;
}

// the two arguments statrs' Lanczos ln_gamma passes to log for each x (x >= 0.5)
extern "C" void lanczos_log_args(const double *x, int64_t n, double *out /*[2n]*/)
{
    const double dk[11] = {2.48574089138753565546e-5,  1.05142378581721974210,    -3.45687097222016235469,
                           4.51227709466894823700,     -2.98285225323576655721,   1.05639711577126713077,
                           -1.95428773191645869583e-1, 1.70970543404441224307e-2, -5.71926117404305781283e-4,
                           4.63399473359905636708e-6,  -2.71994908488607703910e-9};
    for (int64_t j = 0; j < n; j++) {
        double s = dk[0];
        for (int i = 1; i <= 10; i++) s += dk[i] / (x[j] + (double)i - 1.0);
        out[2 * j] = s;
        out[2 * j + 1] = (x[j] - 0.5 + 10.900511) / 2.71828182845904523536028747135266250;
    }
}

extern "C" void log_bb_pmf_batch(const uint32_t *a, const uint32_t *r, const double *alpha, const double *beta, int64_t n,
                                 double *out)
{
    lf_init();
    for (int64_t i = 0; i < n; i++) out[i] = ref_log_bb_pmf(g_lf, alpha[i], beta[i], a[i], r[i]);
}
"""


@pytest.fixture(scope="module")
def rl(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    if not cxx:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("ref_log")
    src, so = d / "driver.cpp", d / "libreflog.so"
    src.write_text(DRIVER)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fno-fast-math", "-ffp-contract=off", "-fPIC", "-shared",
                           "-I", CSRC, str(src), "-o", str(so), "-lm"])
    L = C.CDLL(str(so))
    vp, i64 = C.c_void_p, C.c_int64
    L.ref_log_mismatches.restype = i64
    L.ref_log_mismatches.argtypes = [vp, i64, vp, i64]
    L.lanczos_log_args.restype = None
    L.lanczos_log_args.argtypes = [vp, i64, vp]
    L.log_bb_pmf_batch.restype = None
    L.log_bb_pmf_batch.argtypes = [vp, vp, vp, vp, i64, vp]
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _mismatches(rl, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    assert np.all(np.isfinite(x)) and np.all(x >= np.finfo(np.float64).tiny)
    bad = np.zeros(16)
    nb = rl.ref_log_mismatches(_p(x), x.size, _p(bad), bad.size)
    return nb, [float(v).hex() for v in bad[:min(nb, 16)]]


def _lanczos_args(rl, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty(2 * x.size)
    rl.lanczos_log_args(_p(x), x.size, _p(out))
    return out


def test_ref_log_equals_libm_log_bit_for_bit(rl):
    rng = np.random.default_rng(20261016)
    sets = {}
    # random doubles over the whole normal range: random exponent field 1..2046, random mantissa
    bits = (rng.integers(1, 2047, 4_000_000, dtype=np.uint64) << np.uint64(52)) | rng.integers(0, 1 << 52, 4_000_000,
                                                                                              dtype=np.uint64)
    sets["random exponents"] = bits.view(np.float64)
    # 1 +- 2^-k and their neighbours, and a dense cloud around 1 (the cancellation-prone range)
    k = np.arange(1, 60, dtype=np.float64)
    near = np.concatenate([1.0 + 2.0 ** -k, 1.0 - 2.0 ** -k])
    near = np.concatenate([np.nextafter(near, 0.0), near, np.nextafter(near, 2.0)])
    one = np.float64(1.0)
    steps = np.arange(1, 200_001, dtype=np.float64)
    sets["1 +- 2^-k"] = np.concatenate([near, one + steps * 2.0 ** -52, one - steps * 2.0 ** -53,
                                        rng.uniform(0.98, 1.02, 1_000_000)])
    # what the Lanczos ln_gamma passes to log for x = count + alpha, alpha and beta over 1 .. 2e6 (and their sum)
    n = 600_000
    al = np.exp(rng.uniform(0.0, np.log(2e6), n))
    be = np.exp(rng.uniform(0.0, np.log(2e6), n))
    al[: n // 4] = np.round(al[: n // 4])  # integer alpha / beta (tallies + 1) as in a real run
    be[: n // 4] = np.round(be[: n // 4])
    a = rng.integers(0, 40, n).astype(np.float64)
    r = rng.integers(0, 40, n).astype(np.float64)
    xs = np.concatenate([al, be, al + be, a + al, r + be, (a + al) + (r + be)])
    sets["Lanczos arguments"] = _lanczos_args(rl, xs)
    total = 0
    report = {}
    for name, x in sets.items():
        nb, bad = _mismatches(rl, x)
        total += x.size
        if nb:
            report[name] = (nb, bad)
    assert total >= 10_000_000
    assert not report, f"ref_log differs from the C library's log on: {report}"


def test_ref_log_bb_pmf_equals_oracle(rl, oracle_lib):
    L = oracle_lib.lib()
    rng = np.random.default_rng(7)
    n = 100_000
    a = rng.integers(0, 30, n).astype(np.uint32)
    r = rng.integers(0, 30, n).astype(np.uint32)
    a[:500] = rng.integers(100, 400, 500)  # ln C beyond the factorial table (ln_gamma(n + 1))
    al = np.exp(rng.uniform(0.0, np.log(2e6), n))
    be = np.exp(rng.uniform(0.0, np.log(2e6), n))
    al[: n // 2] = np.round(al[: n // 2])
    be[: n // 2] = np.round(be[: n // 2])
    # the golden rows (known-answer arguments and the reference-style anchors)
    rows = [(g["alt"], g["ref"], g["alpha"], g["beta"]) for g in GOLD["log_beta_binomial_pmf"]]
    rows += [(x[0], x[1], x[2], x[3]) for x in GOLD["reference_style"]["log_beta_binomial_pmf"]]
    a = np.concatenate([a, np.array([x[0] for x in rows], np.uint32)])
    r = np.concatenate([r, np.array([x[1] for x in rows], np.uint32)])
    al = np.concatenate([al, np.array([x[2] for x in rows], np.float64)])
    be = np.concatenate([be, np.array([x[3] for x in rows], np.float64)])
    got = np.empty(a.size)
    rl.log_bb_pmf_batch(_p(a), _p(r), _p(al), _p(be), a.size, _p(got))
    f = L.orc_log_beta_binomial_pmf
    lnb = L.orc_ln_binomial
    want = np.array([f(float(x), float(y), p, q, lnb(int(x) + int(y), int(x))) for x, y, p, q in zip(a, r, al, be)])
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    assert bad.size == 0, "ref_log_bb_pmf != oracle at (a, r, alpha, beta) = %s" % [
        (int(a[i]), int(r[i]), float(al[i]).hex(), float(be[i]).hex()) for i in bad[:8]]
    # the reference-style anchors are recorded values: bit for bit
    for x in GOLD["reference_style"]["log_beta_binomial_pmf"]:
        j = a.size - len(GOLD["reference_style"]["log_beta_binomial_pmf"]) + GOLD["reference_style"]["log_beta_binomial_pmf"].index(x)
        assert got[j] == x[4]
