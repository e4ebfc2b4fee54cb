#!/usr/bin/env python3
"""Makes the preset Huffman table of the BGZF writer (cellector_amd/bgzf.py, csrc/bgzf_format.h); needs no GPU.

  python tools/bgzf_preset.py [--check]

The table is length-limited Huffman (package-merge, 15 bits) over the twin's token histogram of the project's synthetic matrix —
a 3000 x 2000 one and a 40 x 500 000 one (long cell indices), both files of the aligned pair, written with tabs and with spaces, in
locus-major and in cell-major order — plus 1 on every symbol, so that every byte and every match stays encodable.  The table's own
encoding (HLIT, HDIST, HCLEN, the code-length code, the 316 lengths with repeat symbol 16) is built here once too: it is a constant
bit string in every block.  The result is frozen as data in cellector_amd/bgzf_preset.py and cellector_amd/csrc/bgzf_preset.h;
--check regenerates it and compares with the two files instead of writing them.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cellector_amd import bgzf, mtx_write, synth  # noqa: E402

CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def length_limited(freqs, limit):
    """optimal code lengths <= limit for the (positive) frequencies: package-merge"""
    leaves = sorted((int(f), (i,)) for i, f in enumerate(freqs))
    packages = list(leaves)
    for _ in range(limit - 1):
        merged = [(packages[k][0] + packages[k + 1][0], packages[k][1] + packages[k + 1][1]) for k in range(0, len(packages) - 1, 2)]
        packages = sorted(leaves + merged, key=lambda x: x[0])
    lengths = [0] * len(freqs)
    for _, syms in packages[:2 * len(freqs) - 2]:
        for s in syms:
            lengths[s] += 1
    return lengths


def corpus():
    texts = []
    for L, N, density in ((3000, 2000, 0.01), (40, 500000, 0.01)):
        lo, ce, al, re = synth.generate_coo(L, N, density, seed=4)
        by_cell = np.lexsort((lo, ce))
        for order in (slice(None), by_cell):
            for sep in ("\t", " "):
                for which in (0, 1):
                    texts.append(mtx_write.file_bytes(L, N, lo[order], ce[order], al[order], re[order], which, "aligned", sep))
    return texts


class Bits:
    def __init__(self):
        self.bits = []

    def put(self, value, n):  # LSB first
        self.bits += [(value >> k) & 1 for k in range(n)]


def table_header(litlen, dist):
    """BFINAL = 1, BTYPE = 10 and the table: (bytes, bit count)"""
    seq, syms, k = litlen + dist, [], 0
    while k < len(seq):  # (symbol, extra value): a length, or 16 = the length before, 3..6 times more
        run = 1
        while k + run < len(seq) and seq[k + run] == seq[k]:
            run += 1
        syms.append((seq[k], 0))
        left = run - 1
        while left >= 3:
            take = min(6, left)
            syms.append((16, take - 3))
            left -= take
        syms += [(seq[k], 0)] * left
        k += run
    freq = [0] * 19
    for s, _ in syms:
        freq[s] += 1
    used = [s for s in range(19) if freq[s]]
    cl = [0] * 19
    if len(used) == 1:
        used.append(0 if used[0] else 1)  # (a complete code needs two symbols)
    for s, x in zip(used, length_limited([max(freq[s], 1) for s in used], 7)):
        cl[s] = x
    codes = bgzf.canonical_codes(cl)
    hclen = max(k for k in range(19) if cl[CL_ORDER[k]]) + 1
    out = Bits()
    out.put(1, 1)
    out.put(2, 2)
    out.put(len(litlen) - 257, 5)
    out.put(len(dist) - 1, 5)
    out.put(max(hclen, 4) - 4, 4)
    for k in range(max(hclen, 4)):
        out.put(cl[CL_ORDER[k]], 3)
    for s, extra in syms:
        out.put(codes[s], cl[s])
        if s == 16:
            out.put(extra, 2)
    n = len(out.bits)
    return np.packbits(np.asarray(out.bits + [0] * (-n % 8), np.uint8), bitorder="little").tobytes(), n


def make():
    ll, dd = np.zeros(bgzf.N_LITLEN, np.int64), np.zeros(bgzf.N_DIST, np.int64)
    for text in corpus():
        a, b = bgzf.histogram(text)
        ll += a
        dd += b
    litlen, dist = length_limited(ll + 1, 15), length_limited(dd + 1, 15)
    header, bits = table_header(litlen, dist)
    return litlen, dist, header, bits


def rows(values, per=24):
    return ",\n".join("    " + ", ".join("%d" % v for v in values[k:k + per]) for k in range(0, len(values), per))


def render(litlen, dist, header, bits):
    note = "made by tools/bgzf_preset.py; data only, do not edit"
    py = ('"""The preset Huffman table of the BGZF writer (%s)."""\n' % note +
          "LITLEN_LENGTHS = [\n%s,\n]\nDIST_LENGTHS = [\n%s,\n]\n" % (rows(litlen), rows(dist)) +
          "HEADER_BITS = %d  # BFINAL, BTYPE and the table, LSB first\nHEADER_HEX = (\n%s\n)\n" %
          (bits, "\n".join('    "%s"' % header[k:k + 48].hex() for k in range(0, len(header), 48))))
    words = np.frombuffer(header + b"\0" * (-len(header) % 4), "<u4")
    c = ("// The preset Huffman table of the BGZF writer (%s).\n#pragma once\n#include <stdint.h>\n" % note +
         "static const uint8_t BGZF_LITLEN_LENGTHS[286] = {\n%s,\n};\nstatic const uint8_t BGZF_DIST_LENGTHS[30] = {\n%s,\n};\n" %
         (rows(litlen), rows(dist)) +
         "#define BGZF_HEADER_BITS %du  // BFINAL, BTYPE and the table, LSB first\n#define BGZF_HEADER_WORDS %du\n" % (bits, len(words)) +
         "static const uint32_t BGZF_HEADER[BGZF_HEADER_WORDS] = {\n%s,\n};\n" % ",\n".join(
             "    " + ", ".join("0x%08xu" % w for w in words[k:k + 8]) for k in range(0, len(words), 8)))
    return py, c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    py, c = render(*make())
    paths = (os.path.join(ROOT, "cellector_amd", "bgzf_preset.py"), os.path.join(ROOT, "cellector_amd", "csrc", "bgzf_preset.h"))
    for path, text in zip(paths, (py, c)):
        if args.check:
            if open(path).read() != text:
                sys.exit("%s differs from what the tool makes" % path)
        else:
            with open(path, "w") as f:
                f.write(text)
    print("preset %s: %s, %s" % ("unchanged" if args.check else "written", *paths))


if __name__ == "__main__":
    main()
