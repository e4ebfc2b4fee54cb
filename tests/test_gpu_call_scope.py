"""GPU: the refusal paths of the whole-matrix model calls, in the order a caller meets them.

Every call below opens with the same three steps: the scope of a whole-matrix call (one device, no communicator, all cells), then
"no matrix loaded", then "<call>: iteration in flight".  The first failing step decides the message.  Each call is made with minimal
VALID arguments for the ctx at hand, so nothing but the step under test can refuse it:
  1. a fresh ctx, nothing loaded                 -> EINVAL, "no matrix loaded"
  2. between em_begin() and em_finish()          -> EINVAL, "<call>: iteration in flight"
  3. a ctx loaded after set_shard(0, 24) of 48   -> EINVAL, "... holds all cells ..."
and the donor-count pins: donor_posteriors with 0 and 65 donors names the range 1..64; donor_moment_tables and
pair_fraction_tables, which take no donors at all, succeed on default parameters.

The matrix is load_synthetic's 64 loci x 48 cells; every case is a refused call (an argument error before any launch) or one table.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L_, N_ = 64, 48
EINVAL = 1  # CELLECTOR_EINVAL (include/cellector_ffi.h)
K_, D_, G_ = 2, 2, 4


def _shape(g):
    """(total loci, used loci, local cells) as the wrappers of ffi.Cellector size their arguments: all 0 before a load"""
    d = g.dims()
    return d.total_loci, d.loci_used, (g.n_local if d.total_cells else 0)


def _labels(g):
    return np.arange(_shape(g)[2], dtype=np.uint8) % K_


def _gt(g):
    return np.zeros((D_, _shape(g)[0]), np.uint8)


def _gp(g):
    gp = np.zeros((D_, _shape(g)[0], 3), np.float32)
    gp[:, :, 0] = 1.0
    return gp


def _assign(g):
    return np.arange(_shape(g)[2], dtype=np.uint8) % D_


def _ab(g):
    return np.ones(_shape(g)[1]), np.ones(_shape(g)[1])


def _locus_moments(g):
    """cellector_locus_moments itself: the wrapper sizes flags by n_local, which means nothing before a load"""
    from cellector_amd.ffi import _p
    (alpha, beta), flags = _ab(g), np.zeros(_shape(g)[2], np.uint8)
    out = [np.zeros(_shape(g)[1]) for _ in range(4)]
    g._ck(g._lib.cellector_locus_moments(g.h, _p(alpha), _p(beta), None, _p(flags), *[_p(a) for a in out]))


RHO = np.array([0.0, 0.1, 0.2, 0.3])

# every public call that runs the three-step preamble, by the name its messages carry
CALLS = {
    "locus_moments": _locus_moments,
    "locus_total_counts": lambda g: g.locus_total_counts(),
    "iter_locus_moments": lambda g: g.iter_locus_moments(),
    "class_tallies": lambda g: g.class_tallies(_labels(g), K_),
    "class_alpha_betas": lambda g: g.class_alpha_betas(_labels(g), K_),
    "class_posteriors": lambda g: g.class_posteriors(_labels(g), K_),
    "refine_classes": lambda g: g.refine_classes(_labels(g), K_, max_iter=1),
    "class_pair_alpha_betas": lambda g: g.class_pair_alpha_betas(_labels(g), K_),
    "class_doublets": lambda g: g.class_doublets(_labels(g), K_),
    "refine_class_doublets": lambda g: g.refine_class_doublets(_labels(g), K_, max_iter=1),
    "class_genotypes": lambda g: g.class_genotypes(_labels(g), K_),
    "cluster": lambda g: g.cluster(K_, n_restarts=1),
    "cluster_m_step": lambda g: g.cluster_m_step(np.ones((_shape(g)[2], K_))),
    "cluster_e_step": lambda g: g.cluster_e_step(np.zeros((_shape(g)[1], K_, 2)), K_),
    "donor_tables": lambda g: g.donor_tables(_gt(g)),
    "donor_posteriors": lambda g: g.donor_posteriors(_gt(g)),
    "match_donors": lambda g: g.match_donors(_labels(g), K_, _gt(g)),
    "donor_moment_tables": lambda g: g.donor_moment_tables(),
    "donor_fit": lambda g: g.donor_fit(_gt(g)),
    "donor_posteriors_gp": lambda g: g.donor_posteriors_gp(_gp(g)),
    "donor_weights": lambda g: g.donor_weights(_gp(g)),
    "match_donors_gp": lambda g: g.match_donors_gp(_labels(g), K_, _gp(g)),
    "ambient_tables": lambda g: g.ambient_tables(RHO),
    "ambient_profile": lambda g: g.ambient_profile(_gt(g), _assign(g), RHO),
    "estimate_ambient": lambda g: g.estimate_ambient(_gt(g), _assign(g)),
    "pair_fraction_tables": lambda g: g.pair_fraction_tables(),
    "donor_pair_fractions": lambda g: g.donor_pair_fractions(_gt(g), _assign(g), (_assign(g) + 1) % D_),
    "donor_genotypes": lambda g: g.donor_genotypes(_assign(g), n_donors=D_),
}
EACH = pytest.mark.parametrize("name", list(CALLS))

# the sites that write the preamble out, and the calls that reach it through a shared check
PREAMBLE_SITES = ["locus_moments", "locus_total_counts", "iter_locus_moments", "donor_moment_tables", "pair_fraction_tables",
                  "donor_genotypes"]
THROUGH_CLASS_CHECK = ["class_tallies", "class_alpha_betas", "class_posteriors", "refine_classes", "class_pair_alpha_betas",
                       "class_doublets", "refine_class_doublets", "class_genotypes", "match_donors", "match_donors_gp"]
THROUGH_CLUSTER_CHECK = ["cluster", "cluster_m_step", "cluster_e_step"]
THROUGH_DONOR_CHECK = ["donor_tables", "donor_posteriors", "donor_fit", "donor_pair_fractions"]
THROUGH_DONOR_GP_CHECK = ["donor_posteriors_gp", "donor_weights"]
THROUGH_AMBIENT_CHECK = ["ambient_tables", "ambient_profile", "estimate_ambient"]


@pytest.fixture(scope="module")
def mods(hip_lib_path):
    from cellector_amd import Cellector, ffi
    return dict(Cellector=Cellector, ffi=ffi)


def _loaded(mods, shard=None):
    g = mods["Cellector"](0)
    if shard:
        g.set_shard(*shard)
    g.load_synthetic(L_, N_, 0.3)
    return g


@pytest.fixture(scope="module")
def fresh(mods):
    with mods["Cellector"](0) as g:
        yield g


@pytest.fixture(scope="module")
def in_flight(mods):
    with _loaded(mods) as g:
        g.em_begin()
        yield g
        g.em_threshold()
        g.em_finish()


@pytest.fixture(scope="module")
def sharded(mods):
    with _loaded(mods, (0, N_ // 2)) as g:
        assert g.n_local == N_ // 2
        yield g


def _refused(mods, g, name):
    with pytest.raises(mods["ffi"].CellectorError) as e:
        CALLS[name](g)
    assert e.value.status == EINVAL, str(e.value)
    return str(e.value).split(": ", 1)[1]  # (CellectorError puts the status name in front)


def test_every_preamble_call_is_listed():
    want = (PREAMBLE_SITES + THROUGH_CLASS_CHECK + THROUGH_CLUSTER_CHECK + THROUGH_DONOR_CHECK + THROUGH_DONOR_GP_CHECK +
            THROUGH_AMBIENT_CHECK)
    assert len(want) == len(set(want)) == 28
    assert set(want) <= set(CALLS)


@EACH
def test_nothing_loaded(mods, fresh, name):
    assert _refused(mods, fresh, name) == "no matrix loaded"


@EACH
def test_iteration_in_flight(mods, in_flight, name):
    assert _refused(mods, in_flight, name).startswith(f"{name}: iteration in flight")


@EACH
def test_shard_range(mods, sharded, name):
    msg = _refused(mods, sharded, name)
    assert msg.startswith(f"{name} works on a ctx that holds all cells"), msg


@pytest.mark.parametrize("D", [0, 65])
def test_donor_count_range(mods, D):
    with _loaded(mods) as g:
        with pytest.raises(mods["ffi"].CellectorError) as e:
            g.donor_posteriors(np.zeros((D, L_), np.uint8))
    assert e.value.status == EINVAL
    assert f"donor_posteriors: {D} donors, 1..64 are supported" in str(e.value)


def test_tables_without_donors_succeed(mods):
    with _loaded(mods) as g:
        L = g.dims().loci_used
        mom1, mom2 = g.donor_moment_tables()
        assert mom1.shape == (L, 4, 2) and mom2.shape == (L, 16, 2)
        assert g.pair_fraction_tables()["tab"].shape == (L, 16, 17, 2)
