"""tests/locus_moments_reference.py against the oracle, on matrix C (no GPU): the per-key expected term and variance its sums are
built from agree with oracle_lib.expected_log_pmf within relative 1e-7 max(1, |x|) (the oracle's ln_gamma noise, the tolerance
of every comparison with the oracle here), the histogram's rows sum to the entry counts, and the sums are the plain per-class
sums of the records."""
import numpy as np
import pytest

import locus_moments_reference as lm
import pmf_reference as pr
import test_gpu_tile_sweep as S


@pytest.fixture(scope="module")
def case_c():
    coo = lm.matrix_c()
    order = lm.csr_order(coo[0], coo[1])
    lo, ce, al, re = (x[order] for x in coo)
    alpha, beta = S._alpha_beta(lm.LC, 40)
    return dict(lo=lo, ce=ce, al=al, re=re, n=al + re, alpha=alpha, beta=beta, rec=pr.records(alpha, beta, lo, al, re))


def test_matrix_c_has_what_it_is_for(case_c):
    c = case_c
    far = c["n"] > lm.SMALL
    assert sorted(zip(c["lo"][far].tolist(), c["ce"][far].tolist(), c["n"][far].tolist())) == sorted(lm.C_FAR)
    at = lambda l: np.nonzero(c["lo"] == l)[0]
    assert far[at(0)].any() and far[at(lm.LC - 1)].any()                       # the first and the last locus
    four = at(lm.C_FOUR[0])
    assert [(int(c["ce"][i]), int(c["n"][i])) for i in four if far[i]] == list(lm.C_FOUR[1])
    small_cells = c["ce"][four][~far[four]]
    assert small_cells.min() < 3 and ((small_cells > 3) & (small_cells < 70)).any() and (small_cells == 70).any() and \
        ((small_cells > 71) & (small_cells < 199)).any()                       # interleaved with the far cells
    assert far[at(lm.C_FAR_ONLY)].all() and len(at(lm.C_FAR_ONLY)) == 2        # far entries only
    assert (~far[at(21)]).all() and len(at(21)) > 0                            # none
    assert far[at(lm.C_MASKED)].any() and lm.matrix_c_mask()[lm.C_MASKED] == 0  # a far entry at a masked locus
    tw = np.nonzero((c["lo"] == lm.C_TWICE[0]) & (c["ce"] == lm.C_TWICE[1]) & far)[0]
    assert len(tw) == 2 and sorted(c["n"][tw].tolist()) == sorted(lm.C_TWICE[2])
    assert len(np.unique(c["lo"])) == lm.LC and c["n"].min() == 0 and (c["n"] == 17).any() and (c["n"] == 18).any()


def test_per_key_values_against_the_oracle(case_c, oracle_lib):
    c = case_c
    key = c["lo"] * (1 << 20) + c["n"]
    uk, first = np.unique(key, return_index=True)
    ov = np.array([oracle_lib.expected_log_pmf(int(k & 0xFFFFF), float(c["alpha"][k >> 20]), float(c["beta"][k >> 20])) for k in uk])
    for col, want in (("expected", ov[:, 0]), ("variance", ov[:, 1])):
        got = c["rec"][col][first]
        d = np.abs(got - want) / np.maximum(1.0, np.abs(want))
        print(f"  {col}: {len(uk)} keys against the oracle, worst relative {d.max():.2e} (tolerance 1e-7)")
        assert (d <= 1e-7).all(), (col, uk[d > 1e-7][:5])
    assert (c["rec"]["expected"] <= 0).all() and (c["rec"]["variance"] >= 0).all()  # one sign per sum: the bound relies on it


def test_histogram_and_sums(case_c):
    c = case_c
    per_locus = np.bincount(c["lo"], minlength=lm.LC)
    h_all = lm.histogram(lm.LC, c["lo"], c["ce"], c["n"])
    assert h_all.shape == (lm.LC, 19) and h_all.dtype == np.uint32 and np.array_equal(h_all.sum(axis=1), per_locus)
    assert np.array_equal(h_all[:, 18], np.bincount([l for l, _, _ in lm.C_FAR], minlength=lm.LC))
    mask = lm.matrix_c_mask()
    for name, f in lm.matrix_c_flags().items():
        h = lm.histogram(lm.LC, c["lo"], c["ce"], c["n"], f)
        assert np.array_equal(h.sum(axis=1), np.bincount(c["lo"][f[c["ce"]] != 0], minlength=lm.LC)), name
        assert (h <= h_all).all(), name
        r = lm.sums(lm.LC, c["lo"], c["ce"], c["n"], c["rec"], mask, f)
        for k in lm.KEYS:
            assert not r[k][mask == 0].any(), (name, k)
        # min + maj = the sum over all live entries, whatever the flags
        live = mask[c["lo"]] != 0
        tot = np.zeros(lm.LC, lm.LD)
        np.add.at(tot, c["lo"][live], c["rec"]["expected"][live].astype(lm.LD))
        assert np.allclose((r["exp_min"] + r["exp_maj"]).astype(np.float64), tot.astype(np.float64), rtol=1e-15, atol=0), name
        assert (r["exp_min"] <= 0).all() and (r["var_maj"] >= 0).all() and (r["b_exp_min"] >= 0).all(), name
        if name == "empty":
            assert not r["exp_min"].any() and not r["var_min"].any() and not r["far_min"].any()
        if name == "planted":
            assert r["far_min"].sum() == len(lm.C_FAR) - 1 and r["far_maj"].sum() == 0  # (the masked locus' far entry is not counted)
