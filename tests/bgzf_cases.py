"""The inputs of the BGZF writer's tests (tests/test_bgzf_reference.py, test_bgzf_host.py, test_gpu_bgzf.py): name -> bytes, made once
per process, with the twin's output of each cached beside it.  Everything is derived from seeds and from the preset; nothing is
read from a file."""
import functools

import numpy as np

from cellector_amd import bgzf, mtx_write, synth

P = bgzf.PAYLOAD


def _text(n_bytes, seed=1):
    """mtx-like lines (ascending second index, repeated first), cut at n_bytes: the last line is partial"""
    rng = np.random.default_rng(seed)
    n = n_bytes // 8 + 16
    first = 1 + np.cumsum(rng.random(n) < 0.02)
    second = rng.integers(1, 99999, n)
    value = np.where(rng.random(n) < 0.6, 0, rng.integers(1, 30, n))
    out = b"".join(b"%d\t%d\t%d\n" % t for t in zip(first.tolist(), second.tolist(), value.tolist()))
    assert len(out) >= n_bytes
    return out[:n_bytes]


def _literal_bits(data):
    p = bgzf.preset()
    return p["header_bits"] + p["litlen"][256] + sum(p["litlen"][b] for b in data)


def tie_blocks():
    """two blocks without a newline (all literals) whose preset deflate bytes are exactly len + 5 (a tie: stored) and len + 4 (kept)"""
    p = bgzf.preset()["litlen"]
    cheap = min((b for b in range(256) if b != 10), key=lambda b: p[b])
    dear = max((b for b in range(256) if b != 10), key=lambda b: p[b])
    assert p[cheap] < 8 < p[dear]
    found = {}
    for n_cheap in range(0, 600):
        for n_dear in range(0, 80):
            data = bytes([cheap]) * n_cheap + bytes([dear]) * n_dear
            if not data:
                continue
            over = (_literal_bits(data) + 7) // 8 - len(data)
            if over in (4, 5) and over not in found:
                found[over] = data
        if len(found) == 2:
            break
    return found[5], found[4]


def synthetic(order="locus"):
    """the project's synthetic matrix (2500 x 1500 at 1 %), locus-major as generated or cell-major: (dims, coo)"""
    L, N = 2500, 1500
    lo, ce, al, re = synth.generate_coo(L, N, 0.01, seed=11)
    if order == "cell":
        k = np.lexsort((lo, ce))
        lo, ce, al, re = lo[k], ce[k], al[k], re[k]
    return (L, N), (lo, ce, al, re)


@functools.lru_cache(maxsize=None)
def mtx_texts():
    """name -> one file of the writer's twin: three modes x both separators x both files, in both entry orders (aligned only for
    the cell-major one)"""
    out = {}
    for order in ("locus", "cell"):
        dims, coo = synthetic(order)
        for mode in (("aligned", "sparse", "depth") if order == "locus" else ("aligned",)):
            for sep, sname in (("\t", "tab"), (" ", "space")):
                for which in (0, 1):
                    out["mtx_%s_%s_%s_%d" % (order, mode, sname, which)] = mtx_write.file_bytes(*dims, *coo, which, mode, sep)
    return out


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(5)
    c = {}
    for name, n in (("size_0", 0), ("size_1", 1), ("size_P-1", P - 1), ("size_P", P), ("size_P+1", P + 1), ("size_2P", 2 * P),
                    ("size_2P+1", 2 * P + 1)):
        c[name] = _text(n, seed=n % 97)
    c["one_newline"] = b"\n"
    c["only_newlines"] = b"\n" * (P + 100)
    c["no_newline"] = b"abcdefgh" * 5000
    c["random"] = rng.integers(0, 256, 2 * P + 777).astype(np.uint8).tobytes()
    c["tie_stored"], c["tie_kept"] = tie_blocks()
    for L in list(range(255, 263)) + list(range(513, 520)):
        line = rng.integers(97, 123, L - 1).astype(np.uint8).tobytes() + b"\n"
        c["equal_lines_%d" % L] = line * 2
        c["equal_lines_%d_x3" % L] = b"#\n" + line * 3 + b"tail"
    c["long_line"] = b"head\n" + b"x" * (P + 5000) + b"\n" + b"y" * 300 + b"\n" + b"y" * 300 + b"\n"
    c["changing_lengths"] = b"".join(b"z" * k + b"\n" for k in range(0, 300))
    c["high_bytes"] = (bytes(range(0x90, 0x100)) + b"\n") * 40
    c["all_bytes"] = bytes(range(256)) * 130 + (bytes(range(256)) + b"\n") * 3
    c["partial_first_segment"] = b"7\t12" + b"\n" + _text(3 * P // 2, seed=3)[5:]  # block 2 opens inside a line
    c["no_trailing_newline"] = b"1 2 3\n1 3 3\n1 4 3"
    c.update(mtx_texts())
    return c


@functools.lru_cache(maxsize=None)
def expected(name):
    """(the twin's stream, its stats) of a case"""
    stats = {}
    return bgzf.compress(cases()[name], stats), stats
