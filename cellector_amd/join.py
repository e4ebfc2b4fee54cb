"""Numpy twin of the keyed join of two count streams (cellector_ingest_coo_joined / _mtx_joined, csrc/kernels_join.hip).

Two streams of (locus, cell, count), FIRST and SECOND, each in any order, become one staged COO with an entry per distinct
(locus, cell) key of either stream, ascending strictly by that key:
  MODE_REF    SECOND holds ref counts:  alt = FIRST's count or 0, ref = SECOND's count or 0
  MODE_DEPTH  SECOND holds alt + ref:   alt likewise, ref = depth - alt with an absent depth 0; depth < alt is refused
All-integer, so the device result is bit-identical; the refusals are the device's, in its order, with its words."""
import numpy as np

MODE_REF, MODE_DEPTH = 1, 2
TILE = 2048  # entries of the two streams one block of the join kernels walks (cellector_join_summary.join_tile)
MAX_COUNT = 65535
EINVAL = 1
SIDES = ("FIRST", "SECOND")
KINDS = ("", "index 0 (indices are 1-based)", "locus index out of range", "cell index out of range", "count above 65535 not supported")
KIND_INDEX0, KIND_LOCUS, KIND_CELL, KIND_COUNT = 1, 2, 3, 4


class JoinError(ValueError):
    """A refusal of the join: .status (EINVAL), .what ('entry' | 'duplicate' | 'depth' | 'mode'), .side (0 FIRST, 1 SECOND, None),
    .entry (position in its stream) or .locus / .cell (0-based) of the smallest offender; str() is the device's message."""

    def __init__(self, what, message, side=None, entry=None, kind=None, locus=None, cell=None):
        super().__init__(message)
        self.status, self.what, self.message = EINVAL, what, message
        self.side, self.entry, self.kind, self.locus, self.cell = side, entry, kind, locus, cell


def _triple(t):
    a = [np.ascontiguousarray(x, dtype=np.uint64).ravel() for x in t]
    if len(a) != 3 or not (a[0].shape == a[1].shape == a[2].shape):
        raise ValueError("a stream is three arrays of one length: (locus, cell, count)")
    return a


def _check(side, l, c, v, base, total_loci, total_cells):
    kind = np.zeros(l.shape, np.uint8)
    kind[v > MAX_COUNT] = KIND_COUNT
    kind[c - base >= total_cells] = KIND_CELL  # (unsigned: an index below the base wraps to a huge one; index 0 is named below)
    kind[l - base >= total_loci] = KIND_LOCUS
    if base:
        kind[(l == 0) | (c == 0)] = KIND_INDEX0
    bad = np.flatnonzero(kind)
    if bad.size:
        i, k = int(bad[0]), int(kind[bad[0]])
        raise JoinError("entry", f"join: {SIDES[side]} entry {i}: {KINDS[k]}", side=side, entry=i, kind=k)


def _ordered(key, v):
    if key.size < 2 or bool(np.all(key[1:] > key[:-1])):
        return key, v, 1
    order = np.argsort(key, kind="stable")
    return key[order], v[order], 0


def _duplicates(side, key):
    eq = np.flatnonzero(key[1:] == key[:-1]) if key.size > 1 else np.zeros(0, np.int64)
    if eq.size:
        k = int(key[eq].min())
        raise JoinError("duplicate", f"join: {SIDES[side]} lists (locus {(k >> 32) + 1}, cell {(k & 0xffffffff) + 1}) twice", side=side,
                        locus=k >> 32, cell=k & 0xffffffff)


def join_coo(first, second, mode, total_loci=1 << 32, total_cells=1 << 32, one_based=False):
    """first, second: (locus, cell, count) triples, 0-based (one_based: 1-based, as the text files hold them).  Returns
    (locus0, cell0, alt, ref, summary): four uint32 arrays ascending by (locus, cell) and the counts of
    cellector_join_summary as a dict.  Raises JoinError as the device refuses."""
    if mode not in (MODE_REF, MODE_DEPTH):
        raise JoinError("mode", "join: mode must be CELLECTOR_JOIN_REF (1) or CELLECTOR_JOIN_DEPTH (2)")
    base = np.uint64(1 if one_based else 0)
    sides = [_triple(first), _triple(second)]
    for s, (l, c, v) in enumerate(sides):
        _check(s, l, c, v, base, np.uint64(total_loci), np.uint64(total_cells))
    keys, vals, asc = [], [], []
    for l, c, v in sides:
        k, v, a = _ordered((l - base) << np.uint64(32) | (c - base), v)
        keys.append(k); vals.append(v); asc.append(a)
    for s in range(2):
        _duplicates(s, keys[s])
    (ka, kb), (va, vb) = keys, vals
    union = np.union1d(ka, kb)
    a = np.zeros(union.shape, np.uint64)
    b = np.zeros(union.shape, np.uint64)
    a[np.searchsorted(union, ka)] = va
    b[np.searchsorted(union, kb)] = vb
    if mode == MODE_DEPTH:
        low = np.flatnonzero(b < a)
        if low.size:
            k = int(union[low[0]])
            raise JoinError("depth", f"join: depth below alt at (locus {(k >> 32) + 1}, cell {(k & 0xffffffff) + 1})", locus=k >> 32,
                            cell=k & 0xffffffff)
        b = b - a
    n_both = int(ka.size + kb.size - union.size)
    summary = dict(n_first=int(ka.size), n_second=int(kb.size), n_both=n_both, n_first_only=int(ka.size) - n_both,
                   n_second_only=int(kb.size) - n_both, n_out=int(union.size), first_sorted=asc[0], second_sorted=asc[1], join_tile=TILE)
    return ((union >> np.uint64(32)).astype(np.uint32), (union & np.uint64(0xffffffff)).astype(np.uint32), a.astype(np.uint32),
            b.astype(np.uint32), summary)
