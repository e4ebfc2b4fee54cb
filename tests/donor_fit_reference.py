"""80-bit reference of the donor fit (cellector_donor_moment_tables / cellector_donor_fit; csrc/kernels_donors.hip: k_donor_moments,
k_donor_fit), the device's error bounds, and the comparison the CPU and the GPU tests share.

A plain helper for the tests (no fixtures, no GPU), independent of cellector_amd/donors.py: it shares no code with the twin.  It stands
on donor_reference: the donor call's own sums, decisions and their bounds come from donor_reference.reference(), and the model of the
fit is stated once more here in np.longdouble (u64 = 2^-64).

Bounds (u = U = 2^-53; nothing here is fitted to observed errors).  n = the entries of the cell at used, unmasked loci.

  tables th and rest = 1.0 - th are chains of IEEE operations on doubles: the device's th IS the double formed here in double.  la =
         log(th), lb = log(rest) are good to C_LOG u relative (donor_reference's tab bound).
         h = (th la) + (rest lb): each product carries C_LOG u of its log and u of its own rounding, both products are <= 0 so the sum
         does not cancel, and it rounds once: B_h = (C_LOG + 1) u (|th la| + |rest lb|) + u |h|, a relative bound.
         d = la - lb cancels near theta = 0.5, so its bound is absolute: B_d = C_LOG u (|la| + |lb|) + u |d|.
         v = (th rest) (d d): d d carries 2 |d| B_d + B_d^2 and u of its rounding, th rest u, the last product u:
         B_v = (th rest) (2 |d| B_d + B_d^2) + 3 u v, absolute.
  sums   E, V, PE, PV are sums of doubles (the moment tables the device returned, so no table error enters them): one rounded product
         per entry and one rounded add, B = (n + 1) u sum |n h|, as donor_reference's B_s.
  z      = (s - E) / sqrt(V): the difference carries B_s + B_E and rounds once, sqrt carries B_V / (2 V) relative and an ulp (2 u), the
         quotient rounds once: B_z = (B_s + B_E) / sqrt(V) + |z| (B_V / (2 V) + 4 u).  V = 0.0 is decided exactly: every term n v is
         >= 0 and is 0.0 on both sides or on neither.
  call_z the z of the called hypothesis, comparable where donor_reference decides the status and the hypothesis' donor (best for a
         singlet hypothesis, best_pair for a pair) by more than its bounds.
  keys   the call_z of the status-0 cells.  An order statistic is monotone in every key and moves by no more than the largest bound
         among the keys that can reach it: the bound of q1 (of q3) is the largest B_z among the keys within two of the largest key
         bound of its two bracketing order statistics, plus u of each of its three operations.  A cell whose status donor_reference
         leaves undecided may or may not be a key, and a status-0 cell whose best is undecided may hold any key: the quartiles are taken
         over every such choice (in / out; at -inf / at +inf) and the interval of the threshold is [(1 + k) q1_lo - k q3_hi, (1 + k)
         q1_hi - k q3_lo] widened by their bounds.  More than MAX_OPEN such cells leave the threshold open: every flag is undecided.  (A cell
         of undecided status AND undecided best: out, at -inf, at +inf.)
  flags  a cell whose call_z lies within its bound of the threshold's interval is undecided and left out of the flag comparison.

The reference repeats the operations at 2^-64: every bound is widened by posterior_reference.REF_SHARE of itself, and a comparison adds
half an ulp of the double the reference is rounded to (donor_reference._ratio).
"""
import itertools
import math

import numpy as np

import donor_reference as dr

LD = dr.LD
U = dr.U
F = dr.F
C_LOG = dr.C_LOG
NONE = 255
DEFAULTS = dict(iqr_multiple=3.0, min_cells=8)
MAX_OPEN = 8


# ---- tables ----------------------------------------------------------------------------------------------------------------------
def mom_reference(A, R, err=0.01, ambient=0.03, mask=None):
    """(mom1 [L, 4, 2], mom2 [L, 16, 2]) in longdouble from the double thetas, and their bounds [(L, 4, 2), (L, 16, 2)]"""
    th = dr.theta_double(A, R, err, ambient)
    th2 = np.empty((len(th), 16))
    for a in range(4):
        for b in range(4):
            th2[:, 4 * a + b] = 0.5 * (th[:, a] + th[:, b])
    out, bounds = [], []
    for t in (th, th2):
        rest = 1.0 - t
        tL, rL = t.astype(LD), rest.astype(LD)
        la, lb = np.log(tL), np.log(rL)
        pa, pb = tL * la, rL * lb
        h, d, tr = pa + pb, la - lb, tL * rL
        v = tr * (d * d)
        f = lambda x: np.abs(x).astype(np.float64)
        B_h = (C_LOG + 1.0) * U * (f(pa) + f(pb)) + U * f(h)
        B_d = C_LOG * U * (f(la) + f(lb)) + U * f(d)
        B_v = f(tr) * (2.0 * f(d) * B_d + B_d * B_d) + 3.0 * U * f(v)
        mom, B = np.stack([h, v], axis=-1), np.stack([B_h, B_v], axis=-1) * F
        if mask is not None:
            mom[np.asarray(mask) == 0] = 0
            B[np.asarray(mask) == 0] = 0
        out.append(mom)
        bounds.append(B)
    return out[0], out[1], bounds


def compare_moms(A, R, err, ambient, mask, mom1, mom2):
    w1, w2, (b1, b2) = mom_reference(A, R, err, ambient, mask)
    return dict(mom1=dr._ratio(mom1, w1, b1), mom2=dr._ratio(mom2, w2, b2))


# ---- the cell sums and the z -------------------------------------------------------------------------------------------------------
def sums_reference(N, coo, gt_used, mom1, mom2, anchor, mask=None):
    """(E, V, PE, PV) [N, D] longdouble and their bounds, from DOUBLE moment tables (the device's, or the twin's) and the anchors"""
    g = np.asarray(gt_used, np.int64).T
    lo, ce, al, re = dr._rows(coo, mask)
    m1, m2 = np.asarray(mom1, np.float64).astype(LD), np.asarray(mom2, np.float64).astype(LD)
    gl = g[lo]
    n = (al + re).astype(LD)[:, None]
    a = np.asarray(anchor, np.int64)
    out, bounds = [], []
    for t in (m1[lo[:, None], gl], m2[lo[:, None], 4 * gl[np.arange(len(lo)), a[ce]][:, None] + gl]):
        for j in range(2):
            term = n * t[:, :, j]
            s, cnt = dr._seg_sum(ce, term, N)
            mag, _ = dr._seg_sum(ce, np.abs(term), N)
            out.append(s)
            bounds.append((cnt[:, None] + 1.0) * U * mag.astype(np.float64) * F)
    return out, bounds


def _z(s, B_s, E, B_E, V, B_V):
    Vf = V.astype(np.float64)
    pos = Vf > 0
    Vs = np.where(pos, V, LD(1))
    z = np.where(pos, (s - E) / np.sqrt(Vs), LD(0))
    Vd = np.where(pos, Vf, 1.0)
    B = ((B_s + B_E) / np.sqrt(Vd) + np.abs(z).astype(np.float64) * (B_V / (2.0 * Vd) + 4.0 * U)) * F
    return z, np.where(pos, B, 0.0)


def _quartiles(srt):
    """(q1, q3, the ranks that bracket them) as statrs forms them, on sorted keys (at least 4)"""
    n = len(srt)
    h1, h3 = (n + 1.0 / 3.0) * 0.25 + 1.0 / 3.0, (n + 1.0 / 3.0) * 0.75 + 1.0 / 3.0
    q1 = srt[int(h1) - 1] + LD(h1 - int(h1)) * (srt[int(h1)] - srt[int(h1) - 1])
    q3 = srt[int(h3) - 1] + LD(h3 - int(h3)) * (srt[int(h3)] - srt[int(h3) - 1])
    return q1, q3, (int(h1) - 1, int(h1)), (int(h3) - 1, int(h3))


def order_statistics(keys, iqr_multiple):
    """(median, iqr, threshold) in longdouble of the keys"""
    srt = np.sort(np.asarray(keys, LD))
    n, k = len(srt), len(srt) // 2
    med = srt[k] if n % 2 else (srt[k - 1] + srt[k]) / LD(2)
    q1, q3, _, _ = _quartiles(srt)
    return med, q3 - q1, q1 - LD(iqr_multiple) * (q3 - q1)


def _threshold_interval(keys, B, open_in_out, open_any, iqr_multiple, min_cells):
    """[lo, hi] that holds the device's threshold: keys / B the certain keys and their bounds, open_in_out [(value, bound) or None] the
    cells that may or may not be keys (None: and of unknown value), open_any the number of certain keys of unknown value"""
    if len(open_in_out) + open_any > MAX_OPEN:
        return -math.inf, math.inf
    k = float(iqr_multiple)
    q1_lo = q3_lo = math.inf
    q1_hi = q3_hi = -math.inf
    few = False
    ends = ((-math.inf, 0.0), (math.inf, 0.0))
    states = [(None, v) if v is not None else (None,) + ends for v in open_in_out] + [ends] * open_any
    for pick in itertools.product(*states):
        extra = [p for p in pick if p is not None]
        kv = np.concatenate([np.asarray(keys, LD), np.array([p[0] for p in extra], LD)])
        kb = np.concatenate([np.asarray(B, np.float64), np.array([p[1] for p in extra], np.float64)])
        if len(kv) < int(min_cells):
            few = True
            continue
        o = np.argsort(kv, kind="stable")
        srt, sb = kv[o], kb[o]
        q1, q3, r1, r3 = _quartiles(srt)
        fin = np.isfinite(srt.astype(np.float64))
        bmax = float(sb[fin].max(initial=0.0))

        def reach(r):
            a, b = float(srt[r[0]]), float(srt[r[1]])
            if not (math.isfinite(a) and math.isfinite(b)):
                return math.inf
            near = fin & (srt.astype(np.float64) >= a - 2 * bmax) & (srt.astype(np.float64) <= b + 2 * bmax)
            return float(sb[near].max(initial=0.0)) + 3.0 * U * (abs(a) + abs(b))

        b1, b3 = reach(r1), reach(r3)
        q1f, q3f = float(q1), float(q3)
        if not (math.isfinite(b1) and math.isfinite(b3) and math.isfinite(q1f) and math.isfinite(q3f)):
            return -math.inf, math.inf
        q1_lo, q1_hi = min(q1_lo, q1f - b1 * F), max(q1_hi, q1f + b1 * F)
        q3_lo, q3_hi = min(q3_lo, q3f - b3 * F), max(q3_hi, q3f + b3 * F)
    if q1_lo == math.inf:  # (too few keys whatever the open cells are)
        return -math.inf, -math.inf
    # threshold = q1 - k (q3 - q1): the difference, the product and the difference round once each
    w = 3.0 * U * ((1.0 + 2.0 * k) * max(abs(q1_lo), abs(q1_hi)) + 2.0 * k * max(abs(q3_lo), abs(q3_hi))) * F
    lo = -math.inf if few else (q1_lo - k * (q3_hi - q1_lo)) - w
    return lo, (q1_hi - k * (q3_lo - q1_hi)) + w


def reference(L, N, coo, gt_used, call, mom1, mom2, mask=None, iqr_multiple=3.0, min_cells=8):
    """The fit of every cell in longdouble.  call: donor_reference.reference() of the same arguments (its anchors are the ones the sums
    take); mom1 / mom2: DOUBLE moment tables.  Returns a dict (values longdouble, bounds double)."""
    (E, V, PE, PV), (B_E, B_V, B_PE, B_PV) = sums_reference(N, coo, gt_used, mom1, mom2, call["anchor"], mask)
    z, B_z = _z(call["s"], call["B_s"], E, B_E, V, B_V)
    pz, B_pz = _z(call["p"], call["B_p"], PE, B_PE, PV, B_PV)
    r = np.arange(N)
    status, best = call["status"].astype(np.int64), call["best"].astype(np.int64)
    pair = status == 1
    bp = np.where(pair, call["best_pair"].astype(np.int64), 0)
    call_z = np.where(status == 255, LD(0), np.where(pair, pz[r, bp], z[r, best]))
    B_cz = np.where(status == 255, 0.0, np.where(pair, B_pz[r, bp], B_z[r, best]))
    hyp_a = np.where(pair, call["anchor"].astype(np.int64), best).astype(np.uint8)
    hyp_b = np.where(pair, bp, NONE).astype(np.uint8)
    hyp_ok = call["status_ok"] & np.where(pair, call["pair_ok"], call["best_ok"])
    cz_ok = call["status_ok"] & ((status == 255) | hyp_ok)
    # the keys, the statistics of the reference's own keys, and the interval of the device's threshold
    is_key = status == 0
    keys = call_z[is_key]
    if len(keys) >= int(min_cells):
        med, iqr, thr = order_statistics(keys, iqr_multiple)
    else:
        med, iqr, thr = LD(np.nan), LD(np.nan), LD(-np.inf)
    sure = is_key & call["status_ok"] & call["best_ok"]
    open_any = int((is_key & call["status_ok"] & ~call["best_ok"]).sum())
    maybe = ~call["status_ok"]  # (a key or not: as a key it holds the z of its best, whichever that is)
    open_in_out = [(float(z[c, best[c]]), float(B_z[c, best[c]])) if call["best_ok"][c] else None for c in np.flatnonzero(maybe)]
    t_lo, t_hi = _threshold_interval(call_z[sure], B_cz[sure], open_in_out, open_any, iqr_multiple, min_cells)
    czf = call_z.astype(np.float64)
    unmatched = ((status != 255) & (call_z < thr)).astype(np.uint8)
    below, above = czf + B_cz < t_lo, czf - B_cz >= t_hi
    flag_ok = (call["status_ok"] & (status == 255)) | (cz_ok & (below | above))
    if t_lo == -math.inf and t_hi == -math.inf:  # (no threshold on any side: nothing is flagged)
        flag_ok = np.ones(N, bool)
    return dict(E=E, V=V, PE=PE, PV=PV, B_E=B_E, B_V=B_V, B_PE=B_PE, B_PV=B_PV, z=z, pz=pz, B_z=B_z, B_pz=B_pz, call_z=call_z,
                B_cz=B_cz, hyp_a=hyp_a, hyp_b=hyp_b, status=call["status"], hyp_ok=hyp_ok, cz_ok=cz_ok, keys=keys, median=med, iqr=iqr,
                threshold=thr, t_lo=t_lo, t_hi=t_hi, unmatched=unmatched, flag_ok=flag_ok)


def compare(ref, got):
    """got: the dict of Cellector.donor_fit (or the twin's).  Returns ({name: worst observed / bound}, undecided [cells] bool): the sums
    and the z against their bounds; the hypothesis, call_z and the flags where the reference decides them (inf = a difference there);
    the device's threshold inside the reference's interval."""
    out = dict(fit_e=dr._ratio(got["fit_e"], ref["E"], ref["B_E"]), fit_v=dr._ratio(got["fit_v"], ref["V"], ref["B_V"]),
               pair_e=dr._ratio(got["pair_e"], ref["PE"], ref["B_PE"]), pair_v=dr._ratio(got["pair_v"], ref["PV"], ref["B_PV"]),
               z=dr._ratio(got["z"], ref["z"], ref["B_z"]), pair_z=dr._ratio(got["pair_z"], ref["pz"], ref["B_pz"]))
    ok = ref["cz_ok"]
    out["call_z"] = dr._ratio(np.asarray(got["call_z"])[ok], ref["call_z"][ok], ref["B_cz"][ok])
    h = ref["hyp_ok"]
    same = np.array_equal(np.asarray(got["hyp_a"])[h], ref["hyp_a"][h]) and np.array_equal(np.asarray(got["hyp_b"])[h], ref["hyp_b"][h])
    out["hypothesis"] = 0.0 if same else np.inf
    s = got["summary"]
    thr = float(s["threshold"] if isinstance(s, dict) else s.threshold)
    inside = ref["t_lo"] <= thr <= ref["t_hi"] or (thr == -math.inf and ref["t_lo"] == -math.inf)
    out["threshold"] = 0.0 if inside else np.inf
    f = ref["flag_ok"]
    out["unmatched"] = 0.0 if np.array_equal(np.asarray(got["unmatched"])[f], ref["unmatched"][f]) else np.inf
    return out, ~(h & ok & f)
