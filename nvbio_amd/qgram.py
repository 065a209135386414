"""Q-gram indices and the q-gram filter: the reference's nvbio/qgram (QGramIndex, QGramSetIndex, generate_qgrams, QGramFilter).  All
compute happens in libnvbio_hip.so (nvbio_amd/csrc/qgram.hip); with device="cpu" the same calls go through the
library's host twins and return the same bytes in host tensors.

A q-gram is the 64-bit word sum_j sym(i + j) << 2j, j < q, over 2-bit symbols: the first symbol lowest, symbols past the string's end 0.
Unsigned words live in signed tensors of the same width: q-grams and 64-bit slots in int64, coordinates, ranges and counts in int32.

A string is a uint8 tensor / array of symbols 0..3, or a packed triple `(words, n)` / `(words, n, big_endian)` with `words` an int32
tensor of 2-bit PackedStream words (big-endian by default).  A string set is a PackedStringSet with bits == 2, or a list of symbol
arrays, which is packed first."""
import ctypes as C

import torch

from ._lib import lib, check, current_stream_ptr, QGramIndexStruct
from .strings import pack_symbols, PackedStringSet

MAX_QGRAMS = 0xFFFFFFFF


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _device(device, *tensors):
    if device is not None:
        return torch.device(device)
    for t in tensors:
        if torch.is_tensor(t) and t.is_cuda:
            return t.device
    return torch.device("cuda")


def _is_packed_string(x):
    return isinstance(x, (tuple, list)) and len(x) in (2, 3) and torch.is_tensor(x[0]) and isinstance(x[1], int)


def _is_set(x):
    if isinstance(x, PackedStringSet):
        return True
    return isinstance(x, (tuple, list)) and not _is_packed_string(x) and (len(x) == 0 or hasattr(x[0], "__len__"))


def _string(string, device):
    """-> (words int32 tensor with at least one word, n, big_endian) on the device"""
    if _is_packed_string(string):
        words, n = string[0], int(string[1])
        be = bool(string[2]) if len(string) > 2 else True
        assert words.dtype == torch.int32 and words.is_contiguous() and words.numel() * 16 >= n
        dev = _device(device, words)
        words = words.to(dev)
        if words.numel() == 0:
            words = torch.zeros(1, dtype=torch.int32, device=dev)
        return words, n, be
    sym = torch.as_tensor(string)
    dev = _device(device, sym)
    sym = sym.to(dev).to(torch.uint8).reshape(-1)
    return pack_symbols(sym, 2, True, pad_words=0 if sym.numel() else 1), sym.numel(), True


def _string_set(string_set, device):
    """-> a 2-bit PackedStringSet on the device"""
    if not isinstance(string_set, PackedStringSet):
        strings = [torch.as_tensor(t).to(torch.uint8).reshape(-1) for t in string_set]
        dev = _device(device, *strings)
        length = torch.tensor([t.numel() for t in strings], dtype=torch.int64)
        begin = torch.cumsum(length, 0) - length
        stream = torch.cat([t.to(dev) for t in strings]) if strings else torch.zeros(0, dtype=torch.uint8, device=dev)
        words = pack_symbols(stream, 2, True, pad_words=1)
        return PackedStringSet(words, 2, True, begin.to(dev), length.to(torch.int32).to(dev))
    if string_set.bits != 2:
        raise ValueError("q-grams: only 2-bit string sets are supported, this one has %d bits a symbol" % string_set.bits)
    dev = _device(device, string_set.words)
    if string_set.words.device != dev:
        string_set = PackedStringSet(string_set.words.to(dev), 2, string_set.big_endian, string_set.begin.to(dev),
                                     None if string_set.length is None else string_set.length.to(dev), string_set.fixed_length)
    return string_set


def _check_q(q, qlut=0):
    if not 1 <= q <= 32:
        raise ValueError("q-grams: q must be between 1 and 32, not %d" % q)
    if not 0 <= qlut <= min(q, 16):
        raise ValueError("q-grams: the LUT's q-gram length must be between 0 and min(q, 16), not %d" % qlut)


def _temp(nbytes, dev):
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)


def _as(t, dtype, dev):
    """a contiguous tensor of that width on the device; unsigned numpy input keeps its bits"""
    if not torch.is_tensor(t):
        import numpy as np
        a = np.ascontiguousarray(t)
        if a.dtype.kind == "u":
            a = a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])
        t = torch.from_numpy(a)
    return t.to(dev).to(dtype).contiguous()


def generate_qgrams(string, q, coords=None, device=None):
    """The q-grams of a string at `coords` (positions; None = every position 0 .. n - 1), or of a string set at `coords` (an [n, 2]
    array of (string id, position) pairs): int64 [n].  A q-gram that runs past its string's end is padded with symbol 0."""
    _check_q(q)
    L = lib()
    if _is_set(string):
        ss = _string_set(string, device)
        dev = ss.words.device
        if coords is None:
            raise ValueError("generate_qgrams: a string set needs `coords`, an [n, 2] array of (string id, position) pairs")
        coords = _as(coords, torch.int32, dev).reshape(-1, 2)
        n = coords.shape[0]
        out = torch.empty(n, dtype=torch.int64, device=dev)
        s = ss.struct()
        if dev.type == "cpu":
            check(L.nvbio_hip_qgram_set_generate_host(C.byref(s), len(ss), q, _vp(coords), n, _vp(out), 0), "nvbio_hip_qgram_set_generate_host")
        else:
            check(L.nvbio_hip_qgram_set_generate(C.byref(s), len(ss), q, _vp(coords), n, _vp(out), current_stream_ptr()), "nvbio_hip_qgram_set_generate")
        return out
    words, length, be = _string(string, device)
    dev = words.device
    if coords is not None:
        coords = _as(coords, torch.int32, dev).reshape(-1)
    n = length if coords is None else coords.numel()
    out = torch.empty(n, dtype=torch.int64, device=dev)
    if dev.type == "cpu":
        check(L.nvbio_hip_qgram_generate_host(_vp(words), words.numel(), 2, int(be), length, q, _vp(coords), n, _vp(out), 0), "nvbio_hip_qgram_generate_host")
    else:
        check(L.nvbio_hip_qgram_generate(_vp(words), words.numel(), 2, int(be), length, q, _vp(coords), n, _vp(out), current_stream_ptr()),
              "nvbio_hip_qgram_generate")
    return out


class QGramIndex:
    """The q-gram index of one string: `qgrams` (the distinct q-grams, ascending), `slots` (the exclusive sums of their counts,
    n_unique + 1 words), `index` (the positions grouped by q-gram, ascending inside one) and `lut` (None when qlut == 0)."""
    is_set = False

    def __init__(self, q, qlut, n_qgrams, qgrams, slots, index, lut):
        self.q, self.qlut, self.n_qgrams = q, qlut, n_qgrams
        self.qgrams, self.slots, self.index, self.lut = qgrams, slots, index, lut
        self.n_unique = qgrams.numel()

    @property
    def device(self):
        return self.slots.device

    def struct(self):
        s = QGramIndexStruct()
        s.qgrams = self.qgrams.data_ptr() if self.n_unique else None
        s.slots = self.slots.data_ptr()
        s.index = self.index.data_ptr() if self.n_qgrams else None
        s.lut = self.lut.data_ptr() if self.lut is not None else None
        s.q, s.ql, s.n_unique, s.n_qgrams = self.q, self.qlut, self.n_unique, self.n_qgrams
        return s

    @classmethod
    def _finish(cls, q, qlut, n, n_unique, qgrams, slots, index, lut):
        return cls(q, qlut, n, qgrams[:n_unique].clone(), slots[:n_unique + 1].clone(), index, lut)

    @staticmethod
    def build(string, q, qlut=0, device=None):
        _check_q(q, qlut)
        words, n, be = _string(string, device)
        if n > MAX_QGRAMS:
            raise ValueError("QGramIndex.build: the string has %d symbols, more than 2^32 - 1" % n)
        L, dev = lib(), words.device
        qgrams = torch.empty(n, dtype=torch.int64, device=dev)
        slots = torch.empty(n + 1, dtype=torch.int32, device=dev)
        index = torch.empty(n, dtype=torch.int32, device=dev)
        lut = torch.empty(4 ** qlut + 1, dtype=torch.int32, device=dev) if qlut else None
        n_unique = C.c_uint32(0)
        if dev.type == "cpu":
            check(L.nvbio_hip_qgram_index_build_host(_vp(words), words.numel(), 2, int(be), n, q, qlut, _vp(qgrams), _vp(slots), _vp(index), _vp(lut),
                                                     C.byref(n_unique), 0), "nvbio_hip_qgram_index_build_host")
        else:
            tb = int(L.nvbio_hip_qgram_index_build_temp_bytes(n))
            temp = _temp(tb, dev)
            check(L.nvbio_hip_qgram_index_build(_vp(words), words.numel(), 2, int(be), n, q, qlut, _vp(qgrams), _vp(slots), _vp(index), _vp(lut),
                                                C.byref(n_unique), _vp(temp), tb, current_stream_ptr()), "nvbio_hip_qgram_index_build")
        return QGramIndex._finish(q, qlut, n, n_unique.value, qgrams, slots, index, lut)

    def range(self, queries):
        """int32 [n, 2]: the slots (begin, end) of every query q-gram in `index`, (0, 0) for one that is not in the index"""
        dev = self.device
        queries = _as(queries, torch.int64, dev).reshape(-1)
        n = queries.numel()
        out = torch.empty((n, 2), dtype=torch.int32, device=dev)
        s = self.struct()
        if dev.type == "cpu":
            check(lib().nvbio_hip_qgram_range_host(C.byref(s), _vp(queries), n, _vp(out), 0), "nvbio_hip_qgram_range_host")
        else:
            check(lib().nvbio_hip_qgram_range(C.byref(s), _vp(queries), n, _vp(out), current_stream_ptr()), "nvbio_hip_qgram_range")
        return out


class QGramSetIndex(QGramIndex):
    """The q-gram index of a string set: `index` is int32 [n, 2], the (string id, position) of every seed
    position 0, interval, .. while position + q <= length, enumerated by string and then by position."""
    is_set = True

    @staticmethod
    def build(string_set, q, interval=1, qlut=0, device=None):
        _check_q(q, qlut)
        if interval < 1:
            raise ValueError("QGramSetIndex.build: the seeding interval must be at least 1")
        ss = _string_set(string_set, device)
        L, dev, N = lib(), ss.words.device, len(ss)
        s = ss.struct()
        count = C.c_uint64(0)
        if dev.type == "cpu":
            check(L.nvbio_hip_qgram_set_count_seeds_host(C.byref(s), N, q, interval, C.byref(count), 0), "nvbio_hip_qgram_set_count_seeds_host")
        else:
            tb = int(L.nvbio_hip_qgram_set_count_seeds_temp_bytes(N))
            temp = _temp(tb, dev)
            check(L.nvbio_hip_qgram_set_count_seeds(C.byref(s), N, q, interval, C.byref(count), _vp(temp), tb, current_stream_ptr()),
                  "nvbio_hip_qgram_set_count_seeds")
        n = count.value
        if n > MAX_QGRAMS:
            raise ValueError("QGramSetIndex.build: the set has %d seeds, more than 2^32 - 1" % n)
        qgrams = torch.empty(n, dtype=torch.int64, device=dev)
        slots = torch.empty(n + 1, dtype=torch.int32, device=dev)
        index = torch.empty((n, 2), dtype=torch.int32, device=dev)
        lut = torch.empty(4 ** qlut + 1, dtype=torch.int32, device=dev) if qlut else None
        n_unique = C.c_uint32(0)
        if dev.type == "cpu":
            check(L.nvbio_hip_qgram_set_index_build_host(C.byref(s), N, q, interval, qlut, n, _vp(qgrams), _vp(slots), _vp(index), _vp(lut),
                                                         C.byref(n_unique), 0), "nvbio_hip_qgram_set_index_build_host")
        else:
            tb = int(L.nvbio_hip_qgram_set_index_build_temp_bytes(n, N))
            temp = _temp(tb, dev)
            check(L.nvbio_hip_qgram_set_index_build(C.byref(s), N, q, interval, qlut, n, _vp(qgrams), _vp(slots), _vp(index), _vp(lut),
                                                    C.byref(n_unique), _vp(temp), tb, current_stream_ptr()), "nvbio_hip_qgram_set_index_build")
        return QGramSetIndex._finish(q, qlut, n, n_unique.value, qgrams, slots, index, lut)


class QGramFilter:
    """The reference's QGramFilter: rank() looks the query q-grams up and counts their occurrences, locate() lists the hits of a range
    of them, merge() counts the hits per snapped diagonal.  A hit is (index position, query index) for a QGramIndex and (string id,
    position, query index, 0) for a QGramSetIndex."""

    def __init__(self):
        self.index = None
        self.n_queries = 0
        self.total = 0
        self.ranges = self.slots = self.indices = None

    def n_hits(self):
        return self.total

    def rank(self, index, queries, indices):
        """`queries`: the q-grams; `indices`: what each is reported as in a hit (its position in the query text, say).  -> the number
        of hits.  Keeps `ranges` (int32 [n, 2]) and `slots` (int64 [n], the inclusive sums of the range sizes)."""
        dev = index.device
        queries = _as(queries, torch.int64, dev).reshape(-1)
        self.indices = _as(indices, torch.int32, dev).reshape(-1)
        n = queries.numel()
        if self.indices.numel() != n:
            raise ValueError("QGramFilter.rank: %d queries but %d query indices" % (n, self.indices.numel()))
        self.index, self.n_queries = index, n
        self.ranges = torch.empty((n, 2), dtype=torch.int32, device=dev)
        self.slots = torch.empty(n, dtype=torch.int64, device=dev)
        total = C.c_uint64(0)
        s = index.struct()
        L = lib()
        if dev.type == "cpu":
            check(L.nvbio_hip_qgram_rank_host(C.byref(s), _vp(queries), n, _vp(self.ranges), _vp(self.slots), C.byref(total), 0), "nvbio_hip_qgram_rank_host")
        else:
            tb = int(L.nvbio_hip_qgram_rank_temp_bytes(n))
            temp = _temp(tb, dev)
            check(L.nvbio_hip_qgram_rank(C.byref(s), _vp(queries), n, _vp(self.ranges), _vp(self.slots), C.byref(total), _vp(temp), tb,
                                         current_stream_ptr()), "nvbio_hip_qgram_rank")
        self.total = total.value
        return self.total

    def locate(self, begin, end):
        """hits [begin, end) of the last rank(): int32 [end - begin, 2], or [end - begin, 4] for a set index"""
        if self.index is None:
            raise RuntimeError("QGramFilter.locate: call rank() first")
        if not 0 <= begin <= end <= self.total:
            raise ValueError("QGramFilter.locate: [%d, %d) is not inside the %d hits" % (begin, end, self.total))
        dev, is_set = self.index.device, self.index.is_set
        hits = torch.empty((end - begin, 4 if is_set else 2), dtype=torch.int32, device=dev)
        s = self.index.struct()
        name = "nvbio_hip_qgram_set_locate" if is_set else "nvbio_hip_qgram_locate"
        if dev.type == "cpu":
            check(getattr(lib(), name + "_host")(C.byref(s), self.n_queries, _vp(self.ranges), _vp(self.slots), _vp(self.indices), begin, end, _vp(hits), 0),
                  name + "_host")
        else:
            check(getattr(lib(), name)(C.byref(s), self.n_queries, _vp(self.ranges), _vp(self.slots), _vp(self.indices), begin, end, _vp(hits),
                                       current_stream_ptr()), name)
        return hits

    def merge(self, interval, hits):
        """-> (merged, counts): the distinct snapped diagonals of `hits`, ascending, and how many hits fall on each.  A diagonal is
        query index - index position in wrapping uint32, snapped as the reference's util::round does; merged is int32 [m]
        for string hits and int32 [m, 2], (diagonal, string id) ordered by string id first, for set hits."""
        if interval < 1:
            raise ValueError("QGramFilter.merge: the interval must be at least 1")
        hits = hits.contiguous()
        assert hits.dtype == torch.int32 and hits.dim() == 2 and hits.shape[1] in (2, 4)
        is_set = hits.shape[1] == 4
        n, dev = hits.shape[0], hits.device
        merged = torch.empty((n, 2) if is_set else (n,), dtype=torch.int32, device=dev)
        counts = torch.empty(n, dtype=torch.int32, device=dev)
        n_merged = C.c_uint32(0)
        L = lib()
        name = "nvbio_hip_qgram_set_merge" if is_set else "nvbio_hip_qgram_merge"
        if dev.type == "cpu":
            check(getattr(L, name + "_host")(_vp(hits), n, interval, _vp(merged), _vp(counts), C.byref(n_merged), 0), name + "_host")
        else:
            tb = int(getattr(L, name + "_temp_bytes")(n))
            temp = _temp(tb, dev)
            check(getattr(L, name)(_vp(hits), n, interval, _vp(merged), _vp(counts), C.byref(n_merged), _vp(temp), tb, current_stream_ptr()), name)
        return merged[:n_merged.value], counts[:n_merged.value]
