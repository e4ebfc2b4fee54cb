"""High-precision reference of the locus pass (get_locus_log_likelihoods, main.rs:368-420), the device's error bound, and
the hand-built matrices of the locus sweep (tests/test_gpu_locus_sweep.py; tests/test_locus_reference.py holds all of it on the CPU).

A plain helper (no fixtures, no GPU).  locus_reference() takes the COO arrays in load order (a (locus, cell) pair listed twice is two
entries), the per-locus alpha / beta and mask that were in force when the iteration began and the NEW exclusion set (quirk Q9: the
log-pmfs of iteration i are those of its em_begin, split by the set the iteration itself produces).  Every entry's log-pmf comes from
tile_reference.term_values (80-bit products, ln C from mpmath); a locus' two sums are taken in longdouble and rounded to double.
A masked locus has no PMFData (main.rs:556): contributions and cell counts zero.  The allele tallies alt_* / ref_* are returned
over EVERY entry, masked loci included: they feed init_alpha_betas, which ignores the mask (alpha_betas() after the iteration shows
them; locus_outputs() itself reports zeros at a masked locus, like the oracle).  A 0/0 entry (quirk Q14) adds exactly 0.0 and counts.

Value paths of the device (csrc/kernels_tiled.hip, k_locus_finalize; `form` = dict(engine, t2, deep, shards)):

  regular   1 <= n <= 4            count x table value (k_build_tables: dm_log_bb_pmf, product form)
  tier 2    5 <= n <= 8, t2 on     count x table value (k_t2_tables: one log of a ratio of two products of n factors, product form)
  listed    everything else        a value per entry, 16 lanes striding the locus' list:
              t2 on, shallow       k_ovx_values: dm_log_beta_ratio / ov_slow_log_pmf          -> product form
              t2 on, deep          inline: prefix form for n <= 17, product form above
              t2 off               k_ovf_values or inline: prefix form for n <= 17 (totals 5..8 are listed too), product form above
  engine 1  every entry            k_locus_stats: dm_log_bb_pmf per entry, 64 lanes           -> product form

The device's bound (u = 2^-53; derived from the operations of the code, nothing fitted to what a GPU returned)

  Product form, per entry: tile_reference.term_bound — (2 n + 2 + ceil(n / 8)) u on the ratios, an ulp of each of the ceil(n / 8)
    logs, the ln C part.
  Prefix form, per entry (1 <= n <= 17): lp = (lf[n] - lf[a] - lf[r]) + (LA[a] + LB[r] - LAB[n]) with LA[i] = sum_{m<i} ln(alpha + m) a
    running sum stored by k_ovf_tables (LB, LAB likewise over beta, alpha + beta).  For a family of k logs starting at x0, M = ln(x0 + k - 1)
    being its largest log:
      * each log: one ulp of its value (at most an ulp of M) and u for its rounded argument (alpha + beta is a rounded sum; x0 + m is
        exact for the whole numbers the loop produces, counted anyway): k (ulp(M) + u);
      * the running additions: the first adds to 0.0 exactly, addition i = 2..k rounds at the size of its partial sum <= i M:
        half an ulp of i M each;
    for the three families (alpha, a), (beta, r), (alpha + beta, n); then
      * the two combining operations: half an ulp of LA[a] + LB[r] <= a Ma + r Mb, and half an ulp of the difference, whose
        size is at most LAB[n] <= n Mab (the ratio is below one);
      * ln C from three table values: tile_reference.ln_choose_bound;
      * the last addition: half an ulp of max(ln C, n Mab), which is at least |lp| (the two parts have opposite signs).
    This is larger than the product form's bound and grows with ln(alpha + beta): the errors are absolute at the size of the
    PARTIAL SUMS (up to 17 ln(alpha + beta)), not relative on a ratio near one.  At alpha + beta ~ 1e6 and n = 17 it is ~5e-13
    an entry against ~1e-14 for the product form.
  An entry with n == 0 is exactly zero in every path: bound 0.
  count x value: the product rounds once (u |count x value|: u times the sum of |term| over the counted entries of that side) and
    carries count x (the value's bound) = the sum of the entries' bounds.
  The reduction (engine 2): lane j adds one regular product, up to two tier-2 products (t2 on) and at most ceil(n_listed / 16)
    listed values of that side, the 4-step butterfly four more; every one rounds at a size of at most S = sum of |term| of that side
    (all terms have one sign):  (1 + 2 [t2] + ceil(n_listed / 16) + 4) u S,  n_listed the locus' listed entries of BOTH sides (a lane's
    share of one side's is no more).
  Engine 1: (ceil(n / 64) + 6) u S, n the locus' entries; no products.
  A ctx of shards: every shard runs the pass over its cells (no more additions per lane than above) and the all-reduce adds one
    partial sum per shard: + shards u S.
  Plus half an ulp of the reference's own rounding to double.
  A side with no entries, only 0/0 entries, or a masked locus: bound 0, the device must be exact.

Accuracy of the reference itself: per term tile_reference's REF_OPS(n) 2^-64 max(1, |t|, partial); a sum of m terms adds m 2^-64 S.
"""
import numpy as np

import tile_reference as tr

LD = np.longdouble
U53 = tr.U53
OV_NT = 18          # csrc/tiled.h: the prefix rows serve totals below this
LF_LANES = 16
T_BLU = 639
LR_LOCI = 4096
KEYS = ("cells_min", "cells_maj", "alt_min", "ref_min", "alt_maj", "ref_maj")
PATHS = ("regular", "tier2", "listed-prefix", "listed-product", "zero")

# tier-2 pair number <-> (n, r): csrc/tiled.h t2_code = n (n + 1) / 2 - 15 + r
T2_PAIRS = [(n, r) for n in (5, 6, 7, 8) for r in range(n + 1)]
assert len(T2_PAIRS) == 30 and [T2_PAIRS.index(p) for p in ((5, 0), (6, 0), (7, 0), (8, 0))] == [0, 6, 13, 21]


def prefix_bound(alpha, beta, a, r):
    """per-entry bound of the prefix-sum form (module docstring); arrays"""
    alpha = np.asarray(alpha, np.float64)
    beta = np.asarray(beta, np.float64)
    a = np.asarray(a, np.int64)
    r = np.asarray(r, np.int64)
    n = a + r
    out = np.zeros(len(n), np.float64)
    big = {}
    for name, x0, k in (("a", alpha, a), ("b", beta, r), ("ab", alpha + beta, n)):
        M = np.log(x0 + np.maximum(k - 1, 0))
        out += k * (np.spacing(M) + U53)
        for i in range(2, OV_NT):
            out += np.where(i <= k, 0.5 * np.spacing(i * M), 0.0)
        big[name] = k * M
    out += 0.5 * np.spacing(big["a"] + big["b"]) + 0.5 * np.spacing(big["ab"])
    lnc = np.zeros(len(n), np.float64)
    lnc_b = np.zeros(len(n), np.float64)
    for key in set(zip(n.tolist(), a.tolist())):
        sel = (n == key[0]) & (a == key[1])
        lnc_b[sel] = tr.ln_choose_bound(*key)
        lnc[sel] = float(tr.ln_choose_ld(*key)) if key[0] >= 2 else 0.0
    out += lnc_b + 0.5 * np.spacing(np.maximum(lnc, big["ab"]))
    return np.where(n == 0, 0.0, out)


def entry_paths(alt, ref, form):
    """index into PATHS per entry"""
    n = np.asarray(alt, np.int64) + np.asarray(ref, np.int64)
    if form.get("engine", 2) == 1:
        return np.where(n == 0, 4, 3)
    t2, deep = bool(form.get("t2", True)), bool(form.get("deep", False))
    p = np.full(len(n), 3)
    p[(n >= 1) & (n < OV_NT) & ((not t2) or deep)] = 2
    if t2:
        p[(n >= 5) & (n <= 8)] = 1
    p[(n >= 1) & (n <= 4)] = 0
    p[n == 0] = 4
    return p


def _by_locus(n_loci, locus, v, dtype=None):
    """sum of v per locus in v's own precision (longdouble stays longdouble)"""
    order = np.argsort(locus, kind="stable")
    cnt = np.bincount(locus, minlength=n_loci)
    out = np.zeros(n_loci, dtype or v.dtype)
    nz = cnt > 0
    if len(v):
        starts = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        out[nz] = np.add.reduceat(v[order], starts[nz])
    return out


def entry_terms(locus, alt, ref, alpha, beta):
    """per entry: log-pmf (longdouble), product-form bound, prefix-form bound — evaluated once per distinct (locus, alt, ref)"""
    locus = np.asarray(locus, np.int64)
    alt = np.asarray(alt, np.int64)
    ref = np.asarray(ref, np.int64)
    assert (alt < 65536).all() and (ref < 65536).all()
    key = (locus << 32) | (alt << 16) | ref
    uk, inv = np.unique(key, return_inverse=True)
    kl, ka, kr = uk >> 32, (uk >> 16) & 0xFFFF, uk & 0xFFFF
    al, be = np.asarray(alpha, np.float64)[kl], np.asarray(beta, np.float64)[kl]
    t, log_ulps, _ = tr.term_values(al, be, ka, kr)
    b_prod = np.where(ka + kr == 0, 0.0, tr.term_bound(ka + kr, ka, log_ulps))
    small = (ka + kr) < OV_NT
    b_pre = np.zeros(len(uk))
    b_pre[small] = prefix_bound(al[small], be[small], ka[small], kr[small])
    return t[inv], b_prod[inv], b_pre[inv]


def locus_reference(n_loci, locus, cell, alt, ref, alpha, beta, excluded, mask=None):
    """The locus pass; a dict of per-locus arrays.  contrib_* doubles; KEYS integers (cells_* zero at masked loci, the allele tallies
    over every entry); per_cell; and per side ("min" / "maj") what locus_bound needs: abs_* (sum of |term|), n_* [L, 5] entry counts by
    the class (1..4, 5..8, 9..17, >= 18, 0) the forms map to their paths, bprod_* / bpre_* [L, 5] sums of the per-entry bounds of either
    form by class, abs_cls_* [L, 5] sum of |term| by class.  `live` is the mask as booleans; `entry_term` the per-entry doubles."""
    locus = np.asarray(locus, np.int64)
    cell = np.asarray(cell, np.int64)
    alt = np.asarray(alt, np.int64)
    ref = np.asarray(ref, np.int64)
    excluded = np.asarray(excluded) != 0
    live = np.ones(n_loci, bool) if mask is None else np.asarray(mask) != 0
    t, b_prod, b_pre = entry_terms(locus, alt, ref, alpha, beta)
    n = alt + ref
    cls = np.select([n == 0, n <= 4, n <= 8, n < OV_NT], [4, 0, 1, 2], 3)
    keep = live[locus]
    side = excluded[cell]
    out = dict(live=live, entry_term=np.where(keep, t, 0).astype(np.float64), entry_side=side, entry_class=cls)
    for tag, sel_side in (("min", side), ("maj", ~side)):
        sel = sel_side & keep
        lo = locus[sel]
        out["contrib_" + tag] = _by_locus(n_loci, lo, t[sel], LD).astype(np.float64)
        out["abs_" + tag] = _by_locus(n_loci, lo, np.abs(t[sel]), LD).astype(np.float64)
        out["cells_" + tag] = np.bincount(lo, minlength=n_loci).astype(np.uint64)
        for name, v in (("n_", np.ones(int(sel.sum()))), ("bprod_", b_prod[sel]), ("bpre_", b_pre[sel]),
                        ("abs_cls_", np.abs(t[sel]).astype(np.float64))):
            out[name + tag] = np.stack([np.bincount(lo[cls[sel] == c], weights=v[cls[sel] == c], minlength=n_loci) for c in range(5)], axis=1)
        la = locus[sel_side]
        out["alt_" + tag] = np.bincount(la, weights=alt[sel_side].astype(np.float64), minlength=n_loci).astype(np.uint64)
        out["ref_" + tag] = np.bincount(la, weights=ref[sel_side].astype(np.float64), minlength=n_loci).astype(np.uint64)
    cm = out["cells_min"].astype(np.float64)
    out["per_cell"] = np.where(cm > 0, out["contrib_min"] / np.where(cm > 0, cm, 1.0), 0.0)
    return out


def _class_paths(form):
    """the value path (index into PATHS) of each entry class (1..4, 5..8, 9..17, >= 18, 0) under a form"""
    return entry_paths(np.array([1, 5, 9, 18, 0]), np.zeros(5, np.int64), form)


def locus_bound(ref, form):
    """(bound_min, bound_maj) of the device's contrib_min / contrib_maj under `form` = dict(engine=2, t2=True, deep=False, shards=1)"""
    paths = _class_paths(form)
    engine, shards = form.get("engine", 2), form.get("shards", 1)
    t2 = engine == 2 and bool(form.get("t2", True))
    listed = np.isin(paths, (2, 3, 4))
    n_all = ref["n_min"].sum(axis=1) + ref["n_maj"].sum(axis=1)
    n_listed = ref["n_min"][:, listed].sum(axis=1) + ref["n_maj"][:, listed].sum(axis=1)
    out = []
    for tag in ("min", "maj"):
        S = ref["abs_" + tag]
        b = np.zeros(len(S))
        counted = np.zeros(len(S))
        for c in range(5):
            b += ref["bpre_" + tag][:, c] if paths[c] == 2 else ref["bprod_" + tag][:, c]
            if paths[c] in (0, 1):
                counted += ref["abs_cls_" + tag][:, c]
        if engine == 1:
            adds = np.ceil(n_all / 64.0) + 6
        else:
            adds = 1 + (2 if t2 else 0) + np.ceil(n_listed / float(LF_LANES)) + 4
            b += U53 * counted
        if shards > 1:
            adds = adds + shards
        b += adds * U53 * S
        b += np.where(b > 0, 0.5 * np.spacing(np.abs(ref["contrib_" + tag])), 0.0)
        out.append(np.where(S > 0, b, 0.0))
    return out[0], out[1]


def path_of_locus(ref, form, l):
    """the value paths with entries at locus l (for failure reports)"""
    paths = _class_paths(form)
    got = sorted({PATHS[paths[c]] for c in range(5) if ref["n_min"][l, c] + ref["n_maj"][l, c] > 0})
    return "+".join(got) or "empty"


# ---- the sweep's matrices ----------------------------------------------------------------------------------------------------
# Cells 0 .. POOL-1 are the pool the exclusion sets are drawn from; the others (`ballast`) are never in any set: their reads fix
# alpha / beta of the loaded loci (unequal between neighbours, far from alpha == beta: the discrimination test needs both).
POOL = 1000
BALLAST_TYPES = [(80, 4), (5, 70), (120, 10), (10, 110), (70, 2), (3, 65), (90, 20)]  # (4, 0) and (0, 4) entries per loaded locus: an imbalance of 240 reads and more, beyond what the other entries of a locus can cancel
LISTED_COUNTS = (0, 1, 15, 16, 17, 63, 64, 65, 128, 129)
TOTALS = (0, 5, 8, 9, 16, 17, 18, 19, 40, 200)
SINGLE_PAIRS = (0, 5, 6, 12, 13, 20, 21, 29)
GEOMETRY_L = (1, 15, 16, 17, 638, 639, 640, 1278, 4095, 4096, 4097, 4099)


class _Builder:
    def __init__(self, L, N, seed):
        assert N > POOL + 200
        self.L, self.N = L, N
        self.rng = np.random.default_rng(seed)
        perm = self.rng.permutation(POOL)
        self.A = np.zeros(N, bool)
        self.A[perm[:150]] = True
        self.B = np.zeros(N, bool)
        self.B[perm[100:260]] = True       # 50 cells stay, 110 are new, 100 are rescued; 160 < N / 8
        self.rows = [[], [], [], []]
        self.used = {}                      # locus -> cells already holding an entry there (pairs stay distinct unless asked)
        self.roles = {}
        self.cls = {"min": np.nonzero(self.B)[0], "min_in_A": np.nonzero(self.B & self.A)[0],
                    "maj": np.nonzero(~self.B[:POOL])[0], "maj_in_A": np.nonzero(~self.B & self.A)[0],
                    "maj_free": np.nonzero(~self.B[:POOL] & ~self.A[:POOL])[0], "ballast": np.arange(POOL, N)}

    def pick(self, l, cls, k):
        used = self.used.setdefault(l, set())
        cand = [c for c in self.rng.permutation(self.cls[cls]) if c not in used][:k]
        assert len(cand) == k, (l, cls, k)
        used.update(cand)
        return np.array(cand, np.int64)

    def add(self, l, cells, a, r):
        cells = np.atleast_1d(cells)
        for i, v in enumerate((np.full(len(cells), l), cells, np.broadcast_to(a, cells.shape), np.broadcast_to(r, cells.shape))):
            self.rows[i].append(np.asarray(v, np.int64))

    def role(self, l, name):
        self.roles.setdefault(name, []).append(l)

    # -- what a locus can be given
    def ballast(self, l, kind):
        ma, mb = BALLAST_TYPES[kind % len(BALLAST_TYPES)]
        self.add(l, self.pick(l, "ballast", ma), 4, 0)
        self.add(l, self.pick(l, "ballast", mb), 0, 4)

    def codes(self, l, k_min=2, k_maj=3):
        for n in (1, 2, 3, 4):
            for r in range(n + 1):
                self.add(l, self.pick(l, "min", k_min), n - r, r)
                self.add(l, self.pick(l, "maj", k_maj), n - r, r)

    def listed(self, l, count, side, totals=(9, 0, 17, 18, 12, 40, 10, 19, 16, 200, 11, 25)):
        """`count` listed entries (totals outside 1..8: the count is the same whether tier 2 is on or not)"""
        for i in range(count):
            n = totals[i % len(totals)]
            a = int(self.rng.integers(0, n + 1))
            cls = side if side != "mixed" else ("min", "maj")[i % 2]
            self.add(l, self.pick(l, cls, 1), a, n - a)

    def pairs(self, l, which, k_min=1, k_maj=2):
        for c2 in which:
            n, r = T2_PAIRS[c2]
            self.add(l, self.pick(l, "min", k_min), n - r, r)
            self.add(l, self.pick(l, "maj", k_maj), n - r, r)

    def loaded(self, l, kind):
        """every regular code on both sides, listed entries of the totals around the paths' edges, a few tier-2 pairs, ballast"""
        self.codes(l)
        for n in (0, 9, 17, 18, 40):
            for cls in ("min", "maj"):
                a = int(self.rng.integers(0, n + 1))
                self.add(l, self.pick(l, cls, 1), a, n - a)
        self.pairs(l, sorted(self.rng.choice(30, 4, replace=False).tolist()))
        self.ballast(l, kind)
        self.role(l, "loaded")

    def deep(self, l, which):
        """alpha / beta from ballast reads of 240 per cell; which: 0 both ~5e5 (every ballast cell lists its pair four times), 1 beta == 1
        beside alpha ~2.4e5 (every ref read at the locus sits in a cell of A), 2 alpha == 1 likewise.  (With 1.0 on one side an entry of
        one read of the other allele is a term of -1 / (alpha + beta): at 1e6 it would move the majority sum, whose bound carries the
        thousands of ballast terms, by less than 100 bounds.)  Entries of every total 1..17 on both sides."""
        repeats = 4 if which == 0 else 1
        cells = self.cls["ballast"]
        self.used.setdefault(l, set()).update(cells.tolist())
        for _ in range(repeats):
            if which == 0:
                self.add(l, cells[::2], 240, 0)
                self.add(l, cells[1::2], 0, 240)
            else:
                self.add(l, cells, 240 if which == 1 else 0, 0 if which == 1 else 240)
        for n in range(1, OV_NT):
            for a in sorted({0, n // 2, n}):
                r = n - a
                zero_side = r if which == 1 else (a if which == 2 else 0)
                self.add(l, self.pick(l, "min_in_A" if zero_side else "min", 1), a, r)
                self.add(l, self.pick(l, "maj_in_A" if zero_side else "maj", 1), a, r)
        self.role(l, "deep%d" % which)

    def below_filter(self, l):
        """per_cell far below -80: alpha ~ 2000 against beta ~ 1 and minority reads of (0, 40): ~ -270 a cell"""
        self.add(l, self.pick(l, "ballast", 500), 4, 0)
        self.add(l, self.pick(l, "min_in_A", 6), 0, 40)
        self.add(l, self.pick(l, "maj_free", 3), 2, 0)
        self.role(l, "below_filter")

    def finish(self):
        coo = [np.concatenate(x) if x else np.zeros(0, np.int64) for x in self.rows]
        assert coo[0].max(initial=0) < self.L and coo[1].max(initial=0) < self.N
        return coo


def _case(b, mask=None):
    coo = b.finish()
    return dict(L=b.L, N=b.N, coo=coo, A=b.A, B=b.B, mask=np.ones(b.L, np.uint8) if mask is None else mask, roles=b.roles)


def geometry_matrix(L, N=2000):
    """Locus geometry: loci 0, 638, 639, 640, L - 1 and both sides of 4096 loaded (every regular code, listed entries, pairs), every
    53rd locus between them too (53 and 639 are coprime: every slot residue class of the chunked table gets its share); the rest empty."""
    b = _Builder(L, N, seed=L)
    edges = [l for l in (0, 1, 637, 638, 639, 640, 1277, 1278, 4094, 4095, 4096, 4097, L - 2, L - 1) if 0 <= l < L]
    loci = sorted(set(edges) | set(range(0, L, 53)))
    for i, l in enumerate(loci):
        b.loaded(l, i)
    case = _case(b)
    case["edges"] = sorted(set(edges))
    return case


def _feature_block(b, base):
    """the feature loci from `base` on; returns the next free locus"""
    l = base
    for count in LISTED_COUNTS:
        for side in ("min", "maj", "mixed"):
            b.codes(l, 1, 1)
            b.listed(l, count, side)
            b.ballast(l, l)
            b.role(l, "listed_%d_%s" % (count, side))
            l += 1
    for n in TOTALS:
        for split in ("alt", "ref", "balanced"):
            a = {"alt": n, "ref": 0, "balanced": n // 2}[split]
            b.add(l, b.pick(l, "min", 2), a, n - a)
            b.add(l, b.pick(l, "maj", 2), a, n - a)
            b.add(l, b.pick(l, "min", 1), 1, 0)
            b.add(l, b.pick(l, "maj", 1), 0, 1)
            b.ballast(l, l)
            b.role(l, "total_%d_%s" % (n, split))
            l += 1
    b.codes(l)
    b.pairs(l, range(30))
    b.ballast(l, l)
    b.role(l, "all_pairs")
    l += 1
    for c2 in SINGLE_PAIRS:
        b.pairs(l, [c2], 2, 1)
        b.add(l, b.pick(l, "min", 1), 1, 1)
        b.ballast(l, l)
        b.role(l, "pair_%d" % c2)
        l += 1
    for which in (0, 1, 2):
        b.deep(l, which)
        l += 1
    b.below_filter(l)
    l += 1
    b.add(l, b.pick(l, "maj", 5), 1, 2)          # no minority entry: cells_min == 0, per_cell 0
    b.add(l, b.pick(l, "maj", 2), 9, 3)
    b.ballast(l, l)
    b.role(l, "no_minority")
    l += 1
    b.loaded(l, l)
    return l + 1


def feature_matrix(N=2000):
    """Three chunks and a bit (L = 1300).  The feature block (listed counts x sides, totals x splits, the tier-2 pair loci, three loci
    with alpha + beta ~ 1e6, a locus far below the -80 filter, one without minority entries, a loaded one) stands at locus 1 (live), at
    400 (every locus of it masked one by one, the loci between them live) and at 650 inside chunk 1 (639..1277), which is masked
    as a whole; loci 0, 638, 639, 640, 1277, 1278 and L - 1 are loaded.  One (locus, cell) pair is listed three times."""
    L = 1300
    b = _Builder(L, N, seed=77)
    end1 = _feature_block(b, 1)
    end2 = _feature_block(b, 400)
    end3 = _feature_block(b, 650)
    assert end1 <= 400 and end2 <= 638 and end3 <= 1277
    for i, l in enumerate((0, 638, 639, 640, 1277, 1278, L - 1)):
        b.loaded(l, i)
    c = int(b.cls["min"][0])
    for _ in range(3):
        b.add(1290, [c], 1, 0)
    b.add(1290, b.pick(1290, "maj", 2), 0, 2)
    b.ballast(1290, 3)
    b.role(1290, "repeated_pair")
    mask = np.ones(L, np.uint8)
    mask[400:end2] = 0
    mask[T_BLU:2 * T_BLU] = 0
    case = _case(b, mask)
    case["blocks"] = (1, 400, 650)
    case["block_len"] = end1 - 1
    return case


def iteration0_matrix(N=2000):
    """the feature block with an EMPTY first set: alpha / beta are the whole-number totals + 1 of iteration 0"""
    b = _Builder(700, N, seed=5)
    _feature_block(b, 3)
    for i, l in enumerate((0, 638, 639, 699)):
        b.loaded(l, i)
    b.A[:] = False
    return _case(b)


_cache = {}


def sweep_case(name):
    """the sweep's matrices by name ("geometry-<L>", "features", "iteration0"), built once"""
    if name not in _cache:
        if name.startswith("geometry-"):
            _cache[name] = geometry_matrix(int(name.split("-")[1]))
        else:
            _cache[name] = {"features": feature_matrix, "iteration0": iteration0_matrix}[name]()
    return _cache[name]


SWEEP_CASES = tuple("geometry-%d" % L for L in GEOMETRY_L) + ("features", "iteration0")


def alpha_beta_of(case, excluded):
    """init_alpha_betas (main.rs:598-611): the totals of every cell outside the set, + 1, over every locus"""
    lo, ce, al, re = case["coo"]
    keep = ~np.asarray(excluded, bool)[ce]
    L = case["L"]
    return (np.bincount(lo[keep], weights=al[keep].astype(np.float64), minlength=L) + 1.0,
            np.bincount(lo[keep], weights=re[keep].astype(np.float64), minlength=L) + 1.0)
