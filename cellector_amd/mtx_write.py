"""Host twin of cellector_write_mtx / cellector_format_mtx (csrc/kernels_mtx_write.hip, csrc/mtx_format.h): a COO as the bytes of a
MatrixMarket text pair.

A file is the two fixed header lines, the size line `total_loci SEP total_cells SEP count`, then one line
`locus0+1 SEP cell0+1 SEP value` per entry that is written, in the order of the arrays.  Which entries a file holds and which
value, per mode:
  aligned  every entry in both files: alt in the first, ref in the second (the combiner's files; zeros explicit)
  sparse   the first file holds the entries with alt > 0, the second those with ref > 0
  depth    the first holds alt where alt > 0, the second alt + ref where alt + ref > 0
Byte-identical with the device: plain decimal, no sign, padding or exponent, b"\\n" behind every line.
"""
import numpy as np

MODE_ALIGNED, MODE_SPARSE, MODE_DEPTH = 0, 1, 2
MODES = {"aligned": 0, "sparse": 1, "depth": 2, 0: 0, 1: 1, 2: 2}
FLAG_SPACE, FLAG_HEADER_ZERO = 1, 2
BANNER = b"%%MatrixMarket matrix coordinate real general\n% written by sprs\n"
WINDOW = 1 << 23  # MW_WINDOW_DEFAULT of csrc/kernels_mtx_write.hip: entries per window when option write_window is 0
MAX_LINE = 29     # MTXF_MAX_LINE of csrc/mtx_format.h


def _sep(sep):
    sep = sep.encode() if isinstance(sep, str) else bytes(sep)
    if sep not in (b"\t", b" "):
        raise ValueError("sep is a tab or a space")
    return sep


def flags(sep="\t", header_zero=False):
    """the flags word of the C ABI for a separator and a header style"""
    return (FLAG_SPACE if _sep(sep) == b" " else 0) | (FLAG_HEADER_ZERO if header_zero else 0)


def values(alt, ref, which, mode):
    """(value, written) of every entry in file `which` (0 / 1): the third token, and whether the file has a line for the entry"""
    mode = MODES[mode]
    if which not in (0, 1):
        raise ValueError("which is 0 (first file) or 1 (second)")
    alt, ref = np.asarray(alt, np.int64), np.asarray(ref, np.int64)
    v = alt if which == 0 else (alt + ref if mode == MODE_DEPTH else ref)
    return v, (np.ones(v.shape, bool) if mode == MODE_ALIGNED else v > 0)


def format_lines(locus0, cell0, alt, ref, which, mode="aligned", sep="\t"):
    """the body lines of file `which` for the entries, as bytes"""
    sep = _sep(sep)
    v, w = values(alt, ref, which, mode)
    l1, c1 = np.asarray(locus0, np.int64) + 1, np.asarray(cell0, np.int64) + 1
    line = b"%d" + sep + b"%d" + sep + b"%d\n"
    return b"".join(line % t for t in zip(l1[w].tolist(), c1[w].tolist(), v[w].tolist()))


def n_lines(alt, ref, which, mode="aligned"):
    return int(values(alt, ref, which, mode)[1].sum())


def header(total_loci, total_cells, count, sep="\t"):
    """the three header lines; count: the size line's third number (the file's body lines, or 0 as the combiner writes it)"""
    sep = _sep(sep)
    return BANNER + b"%d" % total_loci + sep + b"%d" % total_cells + sep + b"%d\n" % count


def file_bytes(total_loci, total_cells, locus0, cell0, alt, ref, which, mode="aligned", sep="\t", header_zero=False):
    """one whole file"""
    count = 0 if header_zero else n_lines(alt, ref, which, mode)
    return header(total_loci, total_cells, count, sep) + format_lines(locus0, cell0, alt, ref, which, mode, sep)


def n_windows(n_entries, write_window=0):
    """cellector_write_summary.n_windows: windows per file"""
    w = write_window if write_window > 0 else WINDOW
    return (n_entries + w - 1) // w


def summary(total_loci, total_cells, locus0, cell0, alt, ref, mode="aligned", sep="\t", header_zero=False, write_window=0):
    """cellector_write_summary as a dict"""
    alt, ref = np.asarray(alt, np.int64), np.asarray(ref, np.int64)
    files = [file_bytes(total_loci, total_cells, locus0, cell0, alt, ref, k, mode, sep, header_zero) for k in (0, 1)]
    return dict(n_entries=len(alt), lines_first=n_lines(alt, ref, 0, mode), lines_second=n_lines(alt, ref, 1, mode),
                bytes_first=len(files[0]), bytes_second=len(files[1]), n_dropped_keys=int(((alt == 0) & (ref == 0)).sum()),
                n_windows=n_windows(len(alt), write_window))


def write_pair(first_path, second_path, total_loci, total_cells, locus0, cell0, alt, ref, mode="aligned", sep="\t", header_zero=False):
    """both files written; returns the summary"""
    for k, path in enumerate((first_path, second_path)):
        with open(path, "wb") as f:
            f.write(file_bytes(total_loci, total_cells, locus0, cell0, alt, ref, k, mode, sep, header_zero))
    return summary(total_loci, total_cells, locus0, cell0, alt, ref, mode, sep, header_zero)


def expected_read_back(locus0, cell0, alt, ref, mode="aligned"):
    """what a reader of the pair stages, for a source that ascends strictly by (locus, cell): the entries themselves (aligned), or
    those that are not both zero (sparse through the join, depth through the depth join)"""
    arrs = [np.asarray(a, np.uint32) for a in (locus0, cell0, alt, ref)]
    if MODES[mode] == MODE_ALIGNED:
        return tuple(arrs)
    keep = (arrs[2] != 0) | (arrs[3] != 0)
    return tuple(a[keep] for a in arrs)
