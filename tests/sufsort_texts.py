"""The texts of the suffix-sort tests (tests/test_sufsort_gpu.py, tests/test_sufsort_host.py): the smallest at which each step of
nvbio_amd/csrc/sufsort.hip can still go wrong.  Symbols 0..3 = ACGT."""
import numpy as np

# lengths round the 29-symbol round-0 key, the 16-symbol word and the 64-symbol occurrence block
SMALL_LENGTHS = [1, 2, 3, 15, 16, 17, 28, 29, 30, 31, 32, 33, 63, 64, 65, 127, 128, 129]


def pack(text, big_endian, pad_words=0):
    """2-bit PackedStream words (uint32) of a symbol array, in either order"""
    t = np.asarray(text, dtype=np.uint64)
    nw = (t.size + 15) // 16 + pad_words
    buf = np.zeros(nw * 16, dtype=np.uint64)
    buf[:t.size] = t
    k = np.arange(16, dtype=np.uint64)
    sh = (30 - 2 * k) if big_endian else 2 * k
    return (buf.reshape(nw, 16) << sh).sum(axis=1).astype(np.uint32)


def fibonacci_word(n, a=0, b=2):
    x, y = [b], [a]
    while len(y) < n:
        x, y = y, y + x
    return np.array(y[:n], dtype=np.uint8)


def small_texts():
    """(id, text) for every small length: i.i.d. and all-T"""
    out = []
    for n in SMALL_LENGTHS:
        out.append(("iid%d" % n, np.random.default_rng(1000 + n).integers(0, 4, n, dtype=np.uint8)))
        out.append(("allT%d" % n, np.full(n, 3, dtype=np.uint8)))
    return out


def structured_texts():
    rng = np.random.default_rng(77)
    lo = np.zeros(37, dtype=np.uint8); lo[4:] = rng.integers(1, 4, 33); lo[4] = 1        # AAAAC + no further A: suffix 0 is the smallest suffix
    hi = np.zeros(41, dtype=np.uint8); hi[0] = 3                                       # TAAAA...: suffix 0 is the largest
    return [
        ("allA4097", np.zeros(4097, dtype=np.uint8)),                      # one group that shrinks for eight or more rounds
        ("acgt4099", np.tile(np.arange(4, dtype=np.uint8), 1025)[:4099]),
        ("unit301x17", np.tile(rng.integers(0, 4, 301, dtype=np.uint8), 17)),   # groups of 17 whose members resolve in different rounds
        ("fib5779", fibonacci_word(5779)),
        ("iid8191", rng.integers(0, 4, 8191, dtype=np.uint8)),
        ("primary_first", lo),
        ("primary_last", hi),
    ]


def big_text():
    """the text of tests/test_fmindex_gpu.py::test_device_built_index_equals_host_index"""
    text = np.random.default_rng(21).integers(0, 4, 300007, dtype=np.uint8)
    text[1000:3000] = 2
    return text
