"""Exact restatement of the ingest build (ingest_build, csrc/kernels_ingest.hip: get_loci_used, load_data.rs:254-280, and
load_cell_data, load_data.rs:134-181) in plain numpy, and the hand-built matrices of the ingest sweep
(tests/test_gpu_ingest_sweep.py; tests/test_ingest_reference.py holds all of it on the CPU, against the oracle).

A plain helper: no project code, no fixtures, no GPU.  Everything is a whole number.

build(TL, N, coo, min_alt, min_ref, cell_range=None) takes the COO arrays in file order (a (locus, cell) pair listed twice is two
lines) and returns a dict:

  pass1         [5][TL] int64, the planes of CELLECTOR_XCHG_PASS1 in their order: lines with ref > 0, lines with alt > 0,
                sum of ref, sum of alt, lines.  With a cell range [cb, ce): of the lines of those cells only (what a shard holds
                after cellector_ingest_coo, before the exchange).
  pass1_global  the same over every cell: what the exchange leaves in the buffer and what the filter reads.
  used          [TL] bool: lines with ref > 0 >= min_ref AND lines with alt > 0 >= min_alt (load_data.rs:268-273), over ALL cells.
  to_used       [TL] int64: the compact index of a used locus, -1 otherwise.
  locus_ids     [L] uint64, L; locus_counts [L][2] float64 (sum of ref, sum of alt: cellector_locus_counts), over all cells.
  nnz_used      lines of the range's cells at used loci.
  row_ptr       [cells of the range + 1] uint64; entries [nnz_used] uint64, locus_index | alt << 32 | ref << 48: a row ascends by
                used-locus index, repeated (locus, cell) lines keep their file order — the stable sort by locus followed by the
                stable sort by cell (local index); the row order include/cellector_ffi.h documents for cellector_cell_pmfs.  For a
                locus-major file that is the file order inside every cell: cell_loci_data's.

tallies(ref, chosen) gives, per USED locus (indexed through locus_ids), the six integer columns of a cell subset that
tests/test_gpu_tally_capacity._counts forms: lines, sum of alt, sum of ref of the chosen cells ("min") and of the others ("maj").

The constants the cases lean on, restated with their source:
  IB = 256            csrc/kernels_ingest.hip: the block of k_pass1 / k_count / k_fill / k_row_ptr_from_keys
  WAVE = 64           gfx950: what __ballot / __shfl of those kernels span
  SCAN_TILE = 2048    csrc/kernels_ingest.hip: IB * SCAN_ITEMS, the elements one block of k_scan_block takes
  MAX_COUNT = 65535   include/cellector_ffi.h: CELLECTOR_MAX_COUNT, a count is 16 bits of the packed entry

The cases.  case(name) -> dict(name, TL, N, coo, min_alt, min_ref) (+ `sorted`: the file ascends by locus; `own`: the cell range
of the one-shard test).  Every builder asserts the geometry it was built for — the file index of every run boundary it names, the
filter outcome of every locus it names, the empty rows it names — so a change to a builder that moves a case off its edge fails on the
CPU (tests/test_ingest_reference.py builds them all).

  filter-edges-drop / -keep / -mins0   16 loci, min_alt 3, min_ref 2 (unequal: a swap shows at (3,2) and (2,3)); per-locus (alt lines, ref
                      lines) exactly at, one below either, and above the thresholds; a locus that reaches (3,2) through ONE cell listed three
                      times; one line of 60000 / 60000 (many reads, few lines: fails); only 0/0 lines; no lines; first and last locus
                      dropped / kept; the same entries at mins 0 (every locus used, empty ones too: L = TL).
  scan-edges-<TL>[-mins0]   TL either side of one and two scan tiles: the scans of the used flags and of the per-locus line counts
                      are TL + 1 long; at mins 0 L = TL, so the scan of csc_ptr (L + 1) crosses the tile too.
  scan-deep           TL = 2048^2 + 3: both TL-long scans recurse three levels; lines either side of the first- and second-level tile edges.
  run-edges-<nnz>     locus-sorted; runs that begin or end on file indices 63 / 64 / 65 / 255 / 256 / 257, a run of 300 lines (longer than
                      a block), a wave of 64 single-line runs; nnz 255 / 256 / 257 (k_row_ptr_from_keys' grid is cut from nnz + 1);
                      nnz 1281 and 1343: a last wave of 1 and of 63 lines.
  row-edges, row-edges-one-cell   N = 700: empty rows at the front, 260 in a row in the middle, 300 at the back, one row of 300; N = 1.
  sort-bits-N-<n>, sort-bits-TL-<n>   n in {1, 2, 3, 256, 257, 65536, 65537} as the cell count (end_bit of the by-cell sort) and as
                      total_loci with the file out of order (end_bit of the locus sort): lines at index n - 1 and n - 1 - 2^(bits - 1),
                      listed so that a sort blind to the top bit leaves them out of order.
  unsorted-filter-*, unsorted-run-*   the filter-edges and run-edges lines permuted, reversed, and sorted but for the last two; repeated
                      (locus, cell) lines with different counts show whether the sorts are stable.
  unsorted-other-shard   run-edges whose inversions lie only in the cells >= 160: the shard [0, 160) stages an ascending file.
  counts              alt / ref from {0, 1, 65535} in all nine pairs at two neighbouring loci: the packing at bits 32..63.
  empty-nnz0, empty-L0   no lines at mins 0 (L = 5, every row empty); lines but no locus passes (L = 0, nnz_used = 0).
"""
import numpy as np

IB = 256
WAVE = 64
SCAN_TILE = 2048
MAX_COUNT = 65535
P1_PLANES = ("cells_ref", "cells_alt", "sum_ref", "sum_alt", "entries")
KEYS = ("cells_min", "cells_maj", "alt_min", "ref_min", "alt_maj", "ref_maj")


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def _planes(TL, lo, al, re):
    p = np.zeros((5, TL), np.int64)
    np.add.at(p[0], lo[re > 0], 1)
    np.add.at(p[1], lo[al > 0], 1)
    np.add.at(p[2], lo, re)
    np.add.at(p[3], lo, al)
    np.add.at(p[4], lo, 1)
    return p


def build(TL, N, coo, min_alt, min_ref, cell_range=None):
    lo, ce, al, re = (np.asarray(x).astype(np.int64) for x in coo)
    assert len(lo) == len(ce) == len(al) == len(re)
    if len(lo):
        assert 0 <= lo.min() and lo.max() < TL and 0 <= ce.min() and ce.max() < N
        assert 0 <= min(al.min(), re.min()) and max(al.max(), re.max()) <= MAX_COUNT
    cb, cend = (0, N) if cell_range is None else (int(cell_range[0]), int(cell_range[1]))
    assert 0 <= cb <= cend <= N
    own = (ce >= cb) & (ce < cend)
    glob = _planes(TL, lo, al, re)
    used = (glob[0] >= min_ref) & (glob[1] >= min_alt)
    locus_ids = np.nonzero(used)[0]
    L = len(locus_ids)
    to_used = np.full(TL, -1, np.int64)
    to_used[locus_ids] = np.arange(L)
    keep = np.nonzero(own & used[lo])[0]          # file order
    by_locus = keep[np.argsort(lo[keep], kind="stable")]
    order = by_locus[np.argsort(ce[by_locus], kind="stable")]
    packed = (to_used[lo[order]].astype(np.uint64) | (al[order].astype(np.uint64) << np.uint64(32))
              | (re[order].astype(np.uint64) << np.uint64(48)))
    rows = np.zeros(cend - cb, np.int64)
    np.add.at(rows, ce[keep] - cb, 1)
    return dict(TL=TL, N=N, cell_range=(cb, cend), pass1=_planes(TL, lo[own], al[own], re[own]), pass1_global=glob, used=used,
                to_used=to_used, locus_ids=locus_ids.astype(np.uint64), L=L,
                locus_counts=np.stack([glob[2][locus_ids], glob[3][locus_ids]], axis=1).astype(np.float64), nnz_used=len(keep),
                row_ptr=np.concatenate([[0], np.cumsum(rows)]).astype(np.uint64), entries=packed,
                lines=(to_used[lo[keep]], ce[keep] - cb, al[keep], re[keep]))


def tallies(ref, chosen):
    """the six integer columns of locus_outputs() for the cell subset `chosen` (booleans over the range's cells), per used locus"""
    u, cell, al, re = ref["lines"]
    chosen = np.asarray(chosen, bool)
    assert chosen.shape == (ref["cell_range"][1] - ref["cell_range"][0],)
    m = chosen[cell]
    out = {}
    for tag, sel in (("min", m), ("maj", ~m)):
        for key, w in (("cells_", np.ones(len(u), np.int64)), ("alt_", al), ("ref_", re)):
            acc = np.zeros(ref["L"], np.int64)
            np.add.at(acc, u[sel], w[sel])
            out[key + tag] = acc.astype(np.uint64)
    return out


def unpack(entries):
    e = np.asarray(entries, np.uint64)
    return ((e & np.uint64(0xFFFFFFFF)).astype(np.int64), ((e >> np.uint64(32)) & np.uint64(0xFFFF)).astype(np.int64),
            (e >> np.uint64(48)).astype(np.int64))


# ---- helpers of the builders -------------------------------------------------------------------------------------------------------
def _mk(name, TL, N, lo, ce, al, re, min_alt, min_ref, **more):
    coo = tuple(np.ascontiguousarray(x, np.uint32) for x in (lo, ce, al, re))
    lo64 = coo[0].astype(np.int64)
    return dict(name=name, TL=int(TL), N=int(N), coo=coo, min_alt=int(min_alt), min_ref=int(min_ref),
                sorted=bool((np.diff(lo64) >= 0).all()), **more)


def ref_of(case, cell_range=None):
    return build(case["TL"], case["N"], case["coo"], case["min_alt"], case["min_ref"], cell_range)


def runs_of(lo):
    """(first file index, last file index, locus) of every run of equal loci in file order"""
    lo = np.asarray(lo, np.int64)
    if not len(lo):
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    first = np.concatenate([[0], np.nonzero(np.diff(lo) != 0)[0] + 1])
    last = np.concatenate([first[1:] - 1, [len(lo) - 1]])
    return first, last, lo[first]


def sort_bits(n):
    """end_bit of both radix sorts (ingest_build): the smallest bits >= 1 with 2^bits >= n"""
    bits = 1
    while bits < 32 and (1 << bits) < n:
        bits += 1
    return bits


def _blind_to_top_bit_is_visible(keys, n):
    """a stable sort of `keys` (in the order the sort meets them) that ignores bit bits - 1 does not leave them ascending"""
    keys = np.asarray(keys, np.int64)
    low = keys & ((1 << (sort_bits(n) - 1)) - 1)
    return bool((np.diff(keys[np.argsort(low, kind="stable")]) < 0).any())


# ---- filter-edges ------------------------------------------------------------------------------------------------------------------
def _filter_edges(name, keep_ends, mins=(3, 2)):
    rng = np.random.default_rng(16)
    TL, N = 16, 40
    # locus -> lines with (alt only, ref only, both, neither)
    spec = {1: (1, 0, 2, 0),   # (3, 2): exactly at both thresholds
            2: (0, 0, 2, 0),   # (2, 2): one alt line short
            3: (2, 0, 1, 0),   # (3, 1): one ref line short
            4: (0, 1, 4, 0),   # (4, 5): above both
            5: (0, 1, 2, 0),   # (2, 3): passes only if the thresholds are swapped
            8: (0, 0, 0, 4),   # only 0/0 lines
            9: (0, 0, 0, 0)}   # no lines
    spec[0], spec[15] = ((1, 0, 2, 0), (0, 1, 4, 1)) if keep_ends else ((2, 1, 0, 0), (1, 0, 0, 0))   # (dropped: a single last line)
    for l in range(10, 15):
        spec[l] = tuple(int(x) for x in rng.integers(0, 4, 4))
    rows = []
    for l in range(TL):
        if l == 6:      # (3, 2) only because ONE cell is listed three times, with different counts each time
            rows += [(6, 17, 2, 1), (6, 17, 1, 0), (6, 17, 4, 3)]
            continue
        if l == 7:      # many reads in few lines
            rows.append((7, 5, 60000, 60000))
            continue
        kinds = np.repeat(np.arange(4), spec[l])
        cells = np.sort(rng.choice(N, len(kinds), replace=False))
        for c, k in zip(cells, rng.permutation(kinds)):
            rows.append((l, int(c), int(rng.integers(1, 6)) if k in (0, 2) else 0, int(rng.integers(1, 6)) if k in (1, 2) else 0))
    lo, ce, al, re = (np.array(x, np.int64) for x in zip(*rows))
    case = _mk(name, TL, N, lo, ce, al, re, *mins)
    r = ref_of(case)
    p = r["pass1_global"]
    assert case["sorted"] and (case["min_alt"], case["min_ref"]) == mins
    assert [(int(p[1][l]), int(p[0][l])) for l in (1, 2, 3, 4, 5, 6, 7, 8, 9)] == \
        [(3, 2), (2, 2), (3, 1), (4, 5), (2, 3), (3, 2), (1, 1), (0, 0), (0, 0)]
    assert (p[4][6], p[4][7], p[4][8], p[4][9]) == (3, 1, 4, 0) and (p[2][7], p[3][7]) == (60000, 60000) and p[2][8] + p[3][8] == 0
    assert len(set(zip(lo[lo == 6], ce[lo == 6]))) == 1 and len(set(zip(al[lo == 6], re[lo == 6]))) == 3
    if mins == (0, 0):
        assert r["used"].all() and r["L"] == TL and r["nnz_used"] == len(lo)
    else:
        assert r["used"][[1, 2, 3, 4, 5, 6, 7, 8, 9]].tolist() == [True, False, False, True, False, True, False, False, False]
        assert r["used"][0] == keep_ends and r["used"][15] == keep_ends
        # the swapped thresholds decide (3, 2) and (2, 3) the other way round
        swapped = build(TL, N, case["coo"], mins[1], mins[0])["used"]
        assert not swapped[1] and swapped[5]
    return case


# ---- scan-edges, scan-deep ---------------------------------------------------------------------------------------------------------
def _scan_lines(rng, TL, N, named, n_rest, rest_loci=None):
    """locus-sorted lines: 1..3 at each named locus (alt > 0: used at min_alt 1), 1..3 at `n_rest` seeded others, a fifth of which
    have alt == 0 on every line (not used at min_alt 1)"""
    named = sorted({l for l in named if 0 <= l < TL})
    if rest_loci is None:
        rest_loci = rng.choice(TL, min(n_rest, TL), replace=False)
    rest = sorted(set(int(x) for x in rest_loci) - set(named))
    rows = []
    for l in sorted(named + rest):
        cells = np.sort(rng.choice(N, int(rng.integers(1, 4)), replace=False))
        dead = l not in named and rng.random() < 0.2
        for c in cells:
            rows.append((l, int(c), 0 if dead else int(rng.integers(1, 5)), int(rng.integers(0, 3))))
    return tuple(np.array(x, np.int64) for x in zip(*rows)), named


SCAN_TLS = (2047, 2048, 2049, 4095, 4096, 4097)


def _scan_edges(name, TL, mins0):
    rng = np.random.default_rng(TL)
    N = 32
    (lo, ce, al, re), named = _scan_lines(rng, TL, N, (0, 2046, 2047, 2048, TL - 1), 150)
    case = _mk(name, TL, N, lo, ce, al, re, 0 if mins0 else 1, 0)
    r = ref_of(case)
    assert case["sorted"] and r["used"][named].all() and (r["pass1_global"][4][named] > 0).all()
    # blocks of the TL + 1 long scans: one tile, one element past it, two tiles, one element past them
    assert -(-(TL + 1) // SCAN_TILE) == {2047: 1, 2048: 2, 2049: 2, 4095: 2, 4096: 3, 4097: 3}[TL]
    if mins0:
        assert r["L"] == TL                        # the scan of csc_ptr is L + 1 = TL + 1 long
    else:
        assert 100 < r["L"] < 160 and not r["used"].all() and (r["pass1_global"][4][~r["used"]] > 0).any()
    return case


def _scan_deep(name):
    T = SCAN_TILE
    TL = T * T + 3
    rng = np.random.default_rng(7)
    named = (0, T - 1, T, T * (T - 1) - 1, T * (T - 1), T * T - 1, T * T, TL - 1)
    (lo, ce, al, re), named = _scan_lines(rng, TL, 40, named, 0, rest_loci=(1, 5 * T + 17, 1000 * T + 2047, T * T + 1, 999_999, 3_000_000))
    case = _mk(name, TL, 40, lo, ce, al, re, 1, 0)
    r = ref_of(case)
    assert case["sorted"] and 20 <= len(lo) <= 45 and r["used"][named].all() and 8 <= r["L"] <= 14
    # three levels: more than SCAN_TILE block sums, and used loci / lines in the second block of the second level
    assert -(-(TL + 1) // T) > T and (r["locus_ids"] >= T * T).sum() >= 2 and r["to_used"][T * T] >= 6
    return case


# ---- run-edges ---------------------------------------------------------------------------------------------------------------------
RUN_N = 320
_run_lines = None


def _run_edges_lines():
    """1343 locus-sorted lines over 320 cells; run lengths 63, 1, 1, 190, 1, 1, 300, 19, 64 x 1, then seeded ones"""
    global _run_lines
    if _run_lines is None:
        rng = np.random.default_rng(1300)
        lengths = [63, 1, 1, 190, 1, 1, 300, 19] + [1] * 64
        assert sum(lengths[:8]) == 576
        for target, singles in ((1278, 4), (1340, 3)):    # (both variants end in single-line runs: their last two lines differ in locus)
            while sum(lengths) < target:
                lengths.append(min(int(rng.integers(1, 30)), target - sum(lengths)))
            lengths += [1] * singles
        assert sum(lengths) == 1343
        rows, l = [], 1
        for i, k in enumerate(lengths):
            if i == 7:    # (the run of 19) a cell listed twice in a row with different counts
                cells = np.sort(rng.choice(RUN_N, 18, replace=False))
                cells = np.insert(cells, 7, cells[7])
            else:
                cells = np.sort(rng.choice(RUN_N, k, replace=False))
            for j, c in enumerate(cells):
                a, r = int(rng.choice([0, 0, 1, 1, 2, 3, 7])), int(rng.choice([0, 0, 1, 1, 2, 5]))
                if i == 7 and j in (7, 8):
                    a, r = (2, 1) if j == 7 else (5, 3)
                rows.append((l, int(c), a, r))
            l += int(rng.integers(1, 4))
        _run_lines = tuple(np.array(x, np.int64)[:1343] for x in zip(*rows)), l + 2
    return _run_lines


def _run_edges(name, nnz):
    (lo, ce, al, re), TL = _run_edges_lines()
    lo, ce, al, re = lo[:nnz], ce[:nnz], al[:nnz], re[:nnz]
    case = _mk(name, TL, RUN_N, lo, ce, al, re, 1, 1)
    r = ref_of(case)
    first, last, loci = runs_of(lo)
    assert case["sorted"] and len(lo) == nnz and 0 < r["L"] <= len(first)
    if nnz in (255, 256, 257):
        assert -(-(nnz + 1) // IB) == (1 if nnz == 255 else 2)     # the grid of k_row_ptr_from_keys
        assert {63, 64, 65}.issubset(first.tolist()) and {62, 63, 64}.issubset(last.tolist())
    else:
        assert {63, 64, 65, 255, 256, 257}.issubset(first.tolist()) and {62, 63, 64, 254, 255, 256}.issubset(last.tolist())
        assert r["L"] < len(first) and (last - first + 1).max() == 300 and first[np.argmax(last - first + 1)] == 257        # longer than a block
        assert set(range(576, 641)).issubset(first.tolist()) and 576 % WAVE == 0                 # a wave of 64 distinct loci
        single = r["used"][loci[(first >= 576) & (first < 640)]]
        assert len(single) == 64 and single.any() and not single.all()                           # ... kept and dropped ones among them
        assert nnz % WAVE == {1281: 1, 1343: 63}[nnz]                                            # the last wave's lines
        dup = (lo[1:] == lo[:-1]) & (ce[1:] == ce[:-1])
        assert dup.sum() == 1 and (al[1:][dup] != al[:-1][dup]).all()
    return case


# ---- row-edges ---------------------------------------------------------------------------------------------------------------------
def _row_edges(name):
    rng = np.random.default_rng(700)
    TL, N, heavy = 400, 700, 50
    heavy_loci = np.sort(rng.choice(TL, 300, replace=False))
    rows = [(int(l), heavy, int(rng.integers(1, 4)), int(rng.integers(1, 4))) for l in heavy_loci]
    live = [c for c in list(range(10, 100)) + list(range(360, 400)) if c != heavy]
    for c in live:
        if c in (10, 99, 360, 399):      # the rows beside the empty stretches hold a line the filter cannot take
            rows.append((int(heavy_loci[c % 300]), c, 1, 1))
        for l in rng.choice(TL, int(rng.integers(1, 7)), replace=False):
            rows.append((int(l), c, int(rng.integers(0, 4)), int(rng.integers(0, 4))))
    rows.sort(key=lambda t: (t[0], t[1]))
    lo, ce, al, re = (np.array(x, np.int64) for x in zip(*rows))
    case = _mk(name, TL, N, lo, ce, al, re, 1, 1)
    r = ref_of(case)
    n = np.diff(r["row_ptr"].astype(np.int64))
    assert case["sorted"] and 300 <= r["L"] < TL
    assert (n[:10] == 0).all() and (n[100:360] == 0).all() and (n[400:] == 0).all() and n[heavy] == 300 > IB
    assert min(n[10], n[99], n[360], n[399]) >= 1 and (n[live] < 8).all()
    return case


def _one_cell(name):
    case = _mk(name, 6, 1, [0, 1, 1, 3, 5], [0] * 5, [1, 2, 3, 0, 65535], [0, 1, 1, 4, 0], 1, 0)
    r = ref_of(case)
    assert r["locus_ids"].tolist() == [0, 1, 5] and r["row_ptr"].tolist() == [0, 4]
    return case


# ---- sort-bits ---------------------------------------------------------------------------------------------------------------------
SORT_NS = (1, 2, 3, 256, 257, 65536, 65537)


def _sort_bits_cells(name, n):
    """n cells: end_bit of the by-cell sort.  The sort meets the entries in by-locus order: the top cell stands at an earlier locus than
    its twin without the top bit."""
    rng = np.random.default_rng(n)
    half = 1 << (sort_bits(n) - 1)
    top, twin = n - 1, n - 1 - half
    named = [c for c in (top, twin, 0, twin, top) if c >= 0]
    rest_l = np.sort(rng.integers(len(named), 40, 30))
    lo = np.concatenate([np.arange(len(named)), rest_l])
    ce = np.concatenate([named, rng.integers(0, n, 30)]).astype(np.int64)
    al, re = rng.integers(1, 5, len(lo)), rng.integers(0, 3, len(lo))
    case = _mk(name, 40, n, lo, ce, al, re, 1, 0)
    r = ref_of(case)
    assert case["sorted"] and r["nnz_used"] == len(lo) and (ce == top).any() and (n < 2 or (1 << sort_bits(n)) >= n > half)
    if n >= 2:
        assert top & half and _blind_to_top_bit_is_visible(ce, n)
    return case


def _sort_bits_loci(name, n):
    """n loci, the file out of order: end_bit of the locus sort.  The top locus is listed before its twin without the top bit."""
    rng = np.random.default_rng(1000 + n)
    N = 24
    half = 1 << (sort_bits(n) - 1)
    top, twin = n - 1, n - 1 - half
    named = [l for l in (top, twin, 0, top, twin) if l >= 0]
    lo = np.concatenate([named, rng.integers(0, n, 30)]).astype(np.int64)
    ce = rng.integers(0, N, len(lo))
    al, re = rng.integers(1, 5, len(lo)), rng.integers(0, 3, len(lo))
    case = _mk(name, n, N, lo, ce, al, re, 1, 0)
    r = ref_of(case)
    assert r["nnz_used"] == len(lo) and r["used"][top]
    if n >= 2:
        assert not case["sorted"] and top & half and _blind_to_top_bit_is_visible(lo, n)
    else:
        assert case["sorted"]          # one locus cannot be out of order: this one takes the sorted kernels
    return case


# ---- unsorted ----------------------------------------------------------------------------------------------------------------------
def _reordered(name, base, kind):
    b = case(base)
    n = len(b["coo"][0])
    if kind == "perm":
        order = np.random.default_rng(n).permutation(n)
    elif kind == "reversed":
        order = np.arange(n)[::-1]
    else:
        order = np.concatenate([np.arange(n - 2), [n - 1, n - 2]])
    c = _mk(name, b["TL"], b["N"], *(x[order] for x in b["coo"]), b["min_alt"], b["min_ref"])
    lo, ce, al, re = (x.astype(np.int64) for x in c["coo"])
    assert not c["sorted"] and (kind != "swapped" or ((np.diff(lo)[:-1] >= 0).all() and lo[-1] < lo[-2]))
    # stability is visible: some (locus, cell) pair is listed more than once, with different counts
    key = lo * c["N"] + ce
    u, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    rep = np.nonzero(cnt[inv] > 1)[0]
    assert len(rep) >= 2 and len(set(zip(al[rep], re[rep]))) >= 2
    return c


OTHER_SHARD_CUT = 160


def _other_shard(name):
    """run-edges-1281 with the lines of the cells >= 160 in reversed order among themselves: the lines of the cells below ascend"""
    b = case("run-edges-1281")
    lo, ce, al, re = (x.astype(np.int64) for x in b["coo"])
    pos = np.nonzero(ce >= OTHER_SHARD_CUT)[0]
    order = np.arange(len(lo))
    order[pos] = pos[::-1]
    c = _mk(name, b["TL"], b["N"], lo[order], ce[order], al[order], re[order], b["min_alt"], b["min_ref"], own=(0, OTHER_SHARD_CUT))
    lo2, ce2 = c["coo"][0].astype(np.int64), c["coo"][1].astype(np.int64)
    mine = ce2 < OTHER_SHARD_CUT
    assert not c["sorted"] and (np.diff(lo2[mine]) >= 0).all() and (np.diff(lo2[~mine]) < 0).any() and 400 < mine.sum() < 900
    return c


# ---- counts, empty -----------------------------------------------------------------------------------------------------------------
def _counts(name):
    vals = (0, 1, MAX_COUNT)
    pairs = [(a, r) for a in vals for r in vals]
    rows = [(1, 2, 3, 4), (1, 20, 1, 1)]
    rows += [(3, c, a, r) for c, (a, r) in enumerate(pairs)]
    rows += [(4, 5 + c, a, r) for c, (a, r) in enumerate(pairs[::-1])]
    rows += [(6, 0, 2, 2), (6, 23, 0, 1), (6, 23, 1, 0)]
    lo, ce, al, re = (np.array(x, np.int64) for x in zip(*rows))
    case = _mk(name, 8, 24, lo, ce, al, re, 1, 1)
    r = ref_of(case)
    assert case["sorted"] and r["locus_ids"].tolist() == [1, 3, 4, 6]
    for l in (3, 4):
        assert sorted(zip(al[lo == l], re[lo == l])) == sorted(pairs)
    assert r["locus_counts"][1].tolist() == [3 * MAX_COUNT + 3, 3 * MAX_COUNT + 3]
    assert (np.uint64(1) | np.uint64(MAX_COUNT) << np.uint64(32) | np.uint64(MAX_COUNT) << np.uint64(48)) in r["entries"]
    return case


def _empty(name, with_lines):
    if with_lines:
        case = _mk(name, 5, 4, [0, 0, 2, 2, 4, 4], [0, 1, 1, 3, 0, 2], [1, 2, 0, 1, 3, 1], [1, 0, 2, 1, 0, 1], 100, 100)
        r = ref_of(case)
        assert r["L"] == 0 and r["nnz_used"] == 0 and r["pass1"][4].sum() == 6
    else:
        none = np.zeros(0, np.int64)
        case = _mk(name, 5, 4, none, none, none, none, 0, 0)
        r = ref_of(case)
        assert r["L"] == 5 and r["nnz_used"] == 0 and not r["pass1"].any()
    assert r["row_ptr"].tolist() == [0] * 5 and len(r["entries"]) == 0
    return case


# ---- the registry ------------------------------------------------------------------------------------------------------------------
_BUILDERS = {
    "filter-edges-drop": lambda n: _filter_edges(n, False),
    "filter-edges-keep": lambda n: _filter_edges(n, True),
    "filter-edges-mins0": lambda n: _filter_edges(n, False, (0, 0)),
    "scan-deep": _scan_deep,
    "row-edges": _row_edges,
    "row-edges-one-cell": _one_cell,
    "unsorted-other-shard": _other_shard,
    "counts": _counts,
    "empty-nnz0": lambda n: _empty(n, False),
    "empty-L0": lambda n: _empty(n, True),
}
for _TL in SCAN_TLS:
    _BUILDERS["scan-edges-%d" % _TL] = lambda n, TL=_TL: _scan_edges(n, TL, False)
    _BUILDERS["scan-edges-%d-mins0" % _TL] = lambda n, TL=_TL: _scan_edges(n, TL, True)
RUN_NNZ = (255, 256, 257, 1281, 1343)
for _n in RUN_NNZ:
    _BUILDERS["run-edges-%d" % _n] = lambda n, nnz=_n: _run_edges(n, nnz)
for _n in SORT_NS:
    _BUILDERS["sort-bits-N-%d" % _n] = lambda n, k=_n: _sort_bits_cells(n, k)
    _BUILDERS["sort-bits-TL-%d" % _n] = lambda n, k=_n: _sort_bits_loci(n, k)
for _tag, _base in (("filter", "filter-edges-drop"), ("run", "run-edges-1281")):
    for _kind in ("perm", "reversed", "swapped"):
        _BUILDERS["unsorted-%s-%s" % (_tag, _kind)] = lambda n, b=_base, k=_kind: _reordered(n, b, k)

CASES = tuple(sorted(_BUILDERS))
# the cases with fewer than 16 cells: no exclusion set with N / 8 < |B| < N / 4 that an iteration can place; the by-locus test leaves
# them (and only them) out
SMALL_N = ("row-edges-one-cell", "sort-bits-N-1", "sort-bits-N-2", "sort-bits-N-3", "empty-nnz0", "empty-L0")
SHARD_CASES = ("filter-edges-drop", "run-edges-1281", "row-edges", "unsorted-filter-perm", "unsorted-run-perm", "unsorted-run-swapped")
_cache = {}


def case(name):
    """a case by name, built (and its geometry asserted) once"""
    if name not in _cache:
        _cache[name] = _BUILDERS[name](name)
        assert _cache[name]["name"] == name
    return _cache[name]
