"""CPU: the restatement of the ingest build (tests/ingest_reference.py) against the oracle's loader, on every case of the ingest sweep
(tests/test_gpu_ingest_sweep.py), and the geometry each case was built for.

Every case, scan-deep included (the oracle loads its 4.2 M loci in well under a second: nothing of it is left out), is held to
oracle.binding.Oracle.from_coo exactly: loci_used, nnz, locus_ids(), locus_counts(), entries_per_cell(), row_ptr().  entries() is
compared in order for the locus-sorted cases; for the others each row is compared as a multiset: inside a row the oracle keeps the
reference's file order (load_data.rs:165-173) while this library documents locus order (cellector_cell_pmfs), and the restatement's own
order is then asserted directly: ascending used-locus index, repeated (locus, cell) lines in file order.
"""
import numpy as np
import pytest

import ingest_reference as ir


@pytest.mark.parametrize("name", ir.CASES)
def test_case_geometry_and_oracle(oracle_lib, name):
    case = ir.case(name)     # (the builder's own geometry assertions run here)
    TL, N, coo = case["TL"], case["N"], case["coo"]
    r = ir.ref_of(case)
    o = oracle_lib.Oracle.from_coo(TL, N, *coo, case["min_alt"], case["min_ref"])
    assert (o.loci_used, o.nnz) == (r["L"], r["nnz_used"])
    assert np.array_equal(o.locus_ids(), r["locus_ids"])
    assert np.array_equal(o.locus_counts(), r["locus_counts"])
    assert np.array_equal(o.row_ptr(), r["row_ptr"])
    assert np.array_equal(o.entries_per_cell(), np.diff(r["row_ptr"].astype(np.int64)).astype(np.uint32))
    li, al, re, _ = o.entries()
    want = (li.astype(np.uint64) | (al.astype(np.uint64) << np.uint64(32)) | (re.astype(np.uint64) << np.uint64(48)))
    if case["sorted"]:
        bad = np.nonzero(want != r["entries"])[0]
        assert bad.size == 0, (name, bad[:5])
    else:
        rp = r["row_ptr"].astype(np.int64)
        row = np.repeat(np.arange(N), np.diff(rp))
        # the same multiset per row: sorted by (row, packed value) the two lists are equal
        a = np.lexsort((want, row))
        b = np.lexsort((r["entries"], row))
        assert np.array_equal(want[a], r["entries"][b]), name
    o.close()
    # a row ascends by used-locus index
    u, _, _ = ir.unpack(r["entries"])
    rp = r["row_ptr"].astype(np.int64)
    inner = np.ones(len(u), bool)
    inner[rp[:-1][rp[:-1] < len(u)]] = False      # the first entry of a row has no predecessor in it
    assert (np.diff(u)[inner[1:]] >= 0).all()
    # PASS1: whole numbers; lines = the file's; the sums are those of the file
    p = r["pass1"]
    assert p.dtype == np.int64 and p.shape == (5, TL) and p[4].sum() == len(coo[0])
    assert p[2].sum() == int(coo[3].astype(np.int64).sum()) and p[3].sum() == int(coo[2].astype(np.int64).sum())


def test_registry_covers_what_the_sweep_names():
    names = set(ir.CASES)
    for TL in ir.SCAN_TLS:
        assert {"scan-edges-%d" % TL, "scan-edges-%d-mins0" % TL} <= names
    for n in ir.SORT_NS:
        assert {"sort-bits-N-%d" % n, "sort-bits-TL-%d" % n} <= names
    assert {"run-edges-%d" % n for n in ir.RUN_NNZ} <= names and set(ir.SHARD_CASES) <= names
    # the by-locus exemption is exactly the cases with fewer than 16 cells
    assert sorted(ir.SMALL_N) == sorted(n for n in ir.CASES if ir.case(n)["N"] < 16)
    assert (ir.IB, ir.WAVE, ir.SCAN_TILE, ir.MAX_COUNT) == (256, 64, 2048, 65535)


@pytest.mark.parametrize("name", ["filter-edges-drop", "unsorted-run-perm", "row-edges"])
def test_cell_range_is_the_rows_of_the_whole(name):
    """a cell range's PASS1 planes count its own cells and add up to the global ones; its filter is the global one; its rows are the
    whole matrix' rows of those cells; an empty range has no rows"""
    case = ir.case(name)
    N = case["N"]
    whole = ir.ref_of(case)
    cuts = [0, N // 3, N // 3, (2 * N) // 3, N]
    parts = [ir.ref_of(case, (cuts[i], cuts[i + 1])) for i in range(4)]
    assert np.array_equal(sum(p["pass1"] for p in parts), whole["pass1"])
    rp = whole["row_ptr"].astype(np.int64)
    for (cb, ce), p in zip(zip(cuts[:-1], cuts[1:]), parts):
        assert np.array_equal(p["pass1_global"], whole["pass1"]) and np.array_equal(p["locus_ids"], whole["locus_ids"])
        assert np.array_equal(p["locus_counts"], whole["locus_counts"])
        assert np.array_equal(p["row_ptr"].astype(np.int64), rp[cb:ce + 1] - rp[cb])
        assert np.array_equal(p["entries"], whole["entries"][rp[cb]:rp[ce]]) and p["nnz_used"] == rp[ce] - rp[cb]
    assert parts[1]["row_ptr"].tolist() == [0] and not parts[1]["pass1"].any()


def test_tallies_are_the_counts_of_the_rows():
    """tallies(): from the lines, equal to the same sums formed from the packed rows; both sides add up to locus_counts"""
    case = ir.case("run-edges-1281")
    r = ir.ref_of(case)
    chosen = np.zeros(case["N"], bool)
    chosen[1::2] = True
    t = ir.tallies(r, chosen)
    u, al, re = ir.unpack(r["entries"])
    row = np.repeat(np.arange(case["N"]), np.diff(r["row_ptr"].astype(np.int64)))
    for tag, sel in (("min", chosen[row]), ("maj", ~chosen[row])):
        for key, w in (("cells_", np.ones(len(u), np.int64)), ("alt_", al), ("ref_", re)):
            acc = np.zeros(r["L"], np.int64)
            np.add.at(acc, u[sel], w[sel])
            assert np.array_equal(t[key + tag], acc.astype(np.uint64)), key + tag
    assert np.array_equal((t["ref_min"] + t["ref_maj"]).astype(np.float64), r["locus_counts"][:, 0])
    assert np.array_equal((t["alt_min"] + t["alt_maj"]).astype(np.float64), r["locus_counts"][:, 1])
