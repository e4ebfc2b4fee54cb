"""tests/pmf_reference.py — the reference the GPU tests of cellector_cell_pmfs compare with — held to mpmath at 50 digits
(tile_reference._mp) within its own stated accuracy, and to the oracle's per-term functions at the tolerance every comparison
with the oracle uses here (1e-7 max(1, |v|): its ln_gamma cancellation noise).  No GPU.

Grid: totals 0, 1, 4, 5, 8, 9, 17, 18, 25, 80, 300 (either side of the device's two forms, DM_MOM_SMALL = 17, the table edge
T_K = 4 and DM_CHUNK = 8), alpha and beta log-uniform in [1, 1e4]; and (3e4, 1.5, total 80), where pmf(0) ~ 1e-238 and its square
underflows a double: the log-space forms must stay finite there."""
import math

import numpy as np
import pytest

import pmf_reference as pr
import tile_reference as tr

TOTALS = [0, 1, 4, 5, 8, 9, 17, 18, 25, 80, 300]
UNDERFLOW = (3e4, 1.5, 80)
# the (alt, ref) pairs of totals 65..170 that tests/test_gpu_cell_pmfs.py plants: tile_reference.ln_choose_bound's 1.5 ulp is
# established up to 64 only (tests/test_tile_reference.py), so it is checked for exactly these pairs below
PLANTED_MID = [(37, 43)]


def _grid(per_total=5):
    rng = np.random.default_rng(2024)
    keys = [(float(10.0 ** rng.uniform(0, 4)), float(10.0 ** rng.uniform(0, 4)), n) for n in TOTALS for _ in range(per_total)]
    return keys + [UNDERFLOW]


@pytest.fixture(scope="module")
def grid():
    keys = _grid()
    al, be, n = (np.array(x) for x in zip(*keys))
    return keys, pr.moments(al, be, n.astype(np.int64))


def test_moments_against_mpmath(grid):
    keys, m = grid
    worst = 0.0
    for i, (al, be, n) in enumerate(keys):
        e, v = pr.moments_mp(al, be, n)
        de = abs(float(tr._mp().mpf(float(m["e"][i])) - e))
        dv = abs(float(tr._mp().mpf(float(m["v"][i])) - v))
        # (compared as doubles: half an ulp for the conversion on top of the reference's own error)
        be_, bv_ = m["de"][i] + 0.5 * np.spacing(abs(float(e))), m["dv"][i] + 0.5 * np.spacing(abs(float(v)))
        assert de <= be_ and dv <= bv_, (al, be, n, de, be_, dv, bv_)
        worst = max(worst, de / be_ if be_ else 0.0, dv / bv_ if bv_ else 0.0)
        assert math.isfinite(float(m["e"][i])) and math.isfinite(float(m["v"][i])) and float(m["v"][i]) >= 0.0
    print(f"  worst |reference - mpmath| / stated accuracy = {worst:.3f}")


def test_zero_total_is_exactly_zero(grid):
    keys, m = grid
    for i, (_, _, n) in enumerate(keys):
        if n == 0:
            assert m["e"][i] == 0 and m["v"][i] == 0


def test_the_recurrence_table_equals_the_product_form():
    """log_pmfs_mp (loggamma + the log of the ratio recurrence: the totals beyond LD_MAX) against term_mp (products)"""
    mp = tr._mp()
    for al, be, n in [(12.5, 431.0, 40), UNDERFLOW, (7.25e3, 9.5e3, 300)]:
        t = pr.log_pmfs_mp(al, be, n)
        for k in (0, 1, n // 2, n - 1, n):
            assert abs(t[k] - tr.term_mp(al, be, k, n - k)) < mp.mpf(10) ** -40, (al, be, n, k)


def test_moments_against_the_oracle(grid, oracle_lib):
    keys, m = grid
    for i, (al, be, n) in enumerate(keys):
        e, v = oracle_lib.expected_log_pmf(int(n), al, be)
        assert abs(e - float(m["e"][i])) <= 1e-7 * max(1.0, abs(e)), (al, be, n, e, float(m["e"][i]))
        assert abs(v - float(m["v"][i])) <= 1e-7 * max(1.0, abs(v)), (al, be, n, v, float(m["v"][i]))


def test_records_against_the_oracle_and_mpmath(oracle_lib):
    """records(): the per-entry lookup (distinct keys, per-locus alpha / beta) gives each entry its own key's values"""
    L_ = oracle_lib.lib()
    keys = _grid(per_total=2)
    alpha = np.array([k[0] for k in keys])
    beta = np.array([k[1] for k in keys])
    rng = np.random.default_rng(7)
    locus = np.concatenate([np.arange(len(keys)), np.arange(len(keys))])
    n = np.array([k[2] for k in keys] * 2)
    alt = (rng.random(len(n)) * (n + 1)).astype(np.int64)
    rec = pr.records(alpha, beta, locus, alt, n - alt)
    for i in range(len(n)):
        al, be = float(alpha[locus[i]]), float(beta[locus[i]])
        a, r = int(alt[i]), int(n[i] - alt[i])
        want = float(tr.term_mp(al, be, a, r))
        assert abs(rec["log_pmf"][i] - want) <= np.spacing(abs(want)), (al, be, a, r)
        o = L_.orc_log_beta_binomial_pmf(float(a), float(r), al, be, L_.orc_ln_binomial(a + r, a))
        assert abs(rec["log_pmf"][i] - o) <= 1e-7 * max(1.0, abs(o))
        e, v = oracle_lib.expected_log_pmf(a + r, al, be)
        assert abs(rec["expected"][i] - e) <= 1e-7 * max(1.0, abs(e)) and abs(rec["variance"][i] - v) <= 1e-7 * max(1.0, abs(v))
        assert rec["b_log_pmf"][i] >= 0 and rec["b_expected"][i] > 0 and rec["b_variance"][i] >= 0


def test_term_bound_upper_is_an_upper_bound():
    for al, be, n in [(12.5, 431.0, 40), (1.0, 9.9e3, 300), (7.25e3, 1.0, 300), (3e4, 1.5, 80)]:
        ks = np.arange(n + 1)
        _, lu, _ = tr.term_values(np.full(n + 1, al), np.full(n + 1, be), ks, n - ks)
        assert tr.term_bound(np.full(n + 1, n), ks, lu).max() <= pr.term_bound_upper(al, be, n)


def test_ln_choose_bound_holds_for_the_planted_mid_totals():
    """ln C(n, a) = lf[n] - lf[a] - lf[n - a] with the table's values (ln of the factorial in double, host arithmetic as on the
    device: csrc/ctx_core.cpp uploads the host libm's logs) against mpmath, for the planted pairs of totals 65..170"""
    mp = tr._mp()
    for a, r in PLANTED_MID:
        n = a + r
        lf = lambda x: math.log(float(math.factorial(x)))
        got = lf(n) - lf(a) - lf(r)
        assert abs(mp.mpf(got) - mp.log(mp.binomial(n, a))) <= tr.ln_choose_bound(n, a), (a, r)
