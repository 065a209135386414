"""The string sets of the set suffix-sort tests (tests/test_set_sufsort_host.py, tests/test_set_sufsort_gpu.py,
tests/test_compat_set_sufsort_gpu.py): the smallest at which each step of the set path of nvbio_amd/csrc/sufsort.hip can still go wrong.
Symbols 0..3 = ACGT.  A case is a symbol stream and the begin / length arrays of an nvbio_hip_string_set over it; `strings` is what
those arrays select, for the reference."""
import numpy as np

from tests import sufsort_texts as T


class SetCase:
    def __init__(self, id, stream, begin, length=None, fixed_length=0):
        self.id = id
        self.stream = np.asarray(stream, dtype=np.uint8)                   # the whole symbol stream; no padding word follows it
        self.begin = np.asarray(begin, dtype=np.uint64)
        self.length = None if length is None else np.asarray(length, dtype=np.uint32)
        self.fixed_length = int(fixed_length)
        lens = self.length if self.length is not None else np.full(self.begin.size, fixed_length, dtype=np.uint32)
        self.strings = [self.stream[int(b):int(b) + int(l)] for b, l in zip(self.begin, lens)]
        assert all(len(t) == int(l) for t, l in zip(self.strings, lens))
        self.n_strings = self.begin.size
        self.n_suffixes = int(lens.astype(np.uint64).sum()) + self.n_strings

    def words(self, big_endian):
        """the stream's 2-bit words: exactly ceil(symbols / 16) of them, one where the stream is empty"""
        return T.pack(self.stream if self.stream.size else np.zeros(1, dtype=np.uint8), big_endian)


def concatenated(id, strings):
    """the strings one after another, a length array"""
    strings = [np.asarray(t, dtype=np.uint8) for t in strings]
    lens = np.array([t.size for t in strings], dtype=np.uint64)
    begin = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    return SetCase(id, np.concatenate(strings + [np.zeros(0, dtype=np.uint8)]), begin, lens)


def single_string_cases():
    return [concatenated("single_" + i, [t]) for i, t in T.small_texts()]


def small_cases():
    rng = np.random.default_rng(4242)
    iid = lambda n: rng.integers(0, 4, n, dtype=np.uint8)
    A, out = np.zeros, []
    out.append(concatenated("only_empty", [A(0, np.uint8)] * 3))
    out.append(concatenated("empty_A_empty_AA", [A(0, np.uint8), A(1, np.uint8), A(0, np.uint8), A(2, np.uint8)]))
    for copies in (2, 3):
        for n in (1, 16, 28, 29, 30, 58, 59, 100):                      # the tie by id below the key length, at it and after doubling
            out.append(concatenated("same%dx%d" % (n, copies), [iid(n)] * copies))
    t = iid(37)
    out.append(concatenated("prefixes_and_suffixes", [t] + [t[:k] for k in range(1, 37)] + [t[k:] for k in range(1, 37)]))
    out.append(concatenated("allA27to31", [A(n, np.uint8) for n in range(27, 32)]))          # pads against real A
    out.append(concatenated("allT28to30", [np.full(n, 3, dtype=np.uint8) for n in range(28, 31)]))
    # begin at every offset of a word; the stream ends with its last string, on a word boundary and off it (the n_words clamp)
    for tail, name in ((0, "on"), (5, "off")):
        lens = [33] * 15 + [33 + 15 + tail]                             # 16 strings of 33: begin = 33 k, k mod 16 takes every value
        total = sum(lens)
        total += (-(total - tail)) % 16                                  # stretch the last so that the stream ends `tail` past a boundary
        lens[-1] += total - sum(lens)
        stream = iid(total)
        begin = np.concatenate([[0], np.cumsum(lens)[:-1]])
        assert sorted(int(b) % 16 for b in begin) == list(range(16)) and total % 16 == tail
        out.append(SetCase("every_offset_end_%s_boundary" % name, stream, begin, lens))
    stream = iid(150)
    out.append(SetCase("out_of_stream_order", stream, [100, 0, 61, 30], [50, 30, 39, 31]))
    out.append(SetCase("overlapping", stream, [10, 40, 40, 3, 149], [60, 60, 35, 0, 1]))       # two share their start, one is empty
    for n in (1, 29, 33):
        k = 7
        out.append(SetCase("fixed%d" % n, iid(5 + k * n), 5 + n * np.arange(k), None, n))
    return out


def short_iid_case():
    """i.i.d. strings all shorter than 29: round 0 resolves every slot"""
    rng = np.random.default_rng(99)
    return concatenated("short_iid", [rng.integers(0, 4, int(n), dtype=np.uint8) for n in rng.integers(0, 29, 300)])


def medium_case():
    """4 000 reads of 100 symbols from a 20 000-symbol i.i.d. genome, 200 of them exact duplicates of others and 200 cut to random
    lengths 0..99: about 400 k slots, with doubling rounds up to an order of 116 symbols"""
    rng = np.random.default_rng(2024)
    genome = rng.integers(0, 4, 20000, dtype=np.uint8)
    reads = [genome[q:q + 100] for q in rng.integers(0, 20000 - 100, 4000)]
    order = rng.permutation(4000)
    for dst, src in zip(order[:200], order[200:400]):
        reads[dst] = reads[src]
    for i, n in zip(order[400:600], rng.integers(0, 100, 200)):
        reads[i] = reads[i][:int(n)]
    return concatenated("medium", reads)


def all_small():
    return single_string_cases() + small_cases() + [short_iid_case()]
