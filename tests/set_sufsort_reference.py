"""The expected results of the string-set suffix sorter and BWT (nvbio_hip_set_suffix_sort / nvbio_hip_set_bwt), by definition:

  * the slots of a set are the pairs (s, p), 0 <= p <= len[s], the empty suffix p == len[s] included;
  * slot (s, p) has the global index g = cum[s - 1] + p, cum[s] = the inclusive sum of len + 1;
  * the slots are sorted by (the symbols from p on, s) -- Python's bytes order puts a proper prefix first;
  * bwt[row] = symbol p - 1 of string s, 255 where p == 0; dollar_rows / dollar_ids list those rows and their strings."""
import numpy as np


class Expected:
    def __init__(self, strings):
        lens = np.array([len(t) for t in strings], dtype=np.uint64)
        self.n_strings = len(strings)
        self.cum = np.cumsum(lens + 1).astype(np.uint32)
        self.n_suffixes = int(self.cum[-1])
        first = np.concatenate([[0], self.cum[:-1]]).astype(np.int64)
        slots = []
        for s, t in enumerate(strings):
            b = bytes(np.asarray(t, dtype=np.uint8))
            slots.extend((b[p:], s, p) for p in range(len(b) + 1))
        slots.sort(key=lambda x: (x[0], x[1]))
        sid = np.array([x[1] for x in slots], dtype=np.int64)
        pos = np.array([x[2] for x in slots], dtype=np.int64)
        self.suffixes = (first[sid] + pos).astype(np.uint32)
        self.string_ids = np.repeat(np.arange(self.n_strings, dtype=np.uint32), (lens + 1).astype(np.int64))
        self.pairs = np.stack([pos, sid], axis=1).astype(np.uint32).reshape(-1)             # (p, s) of every row
        flat = np.concatenate([np.asarray(t, dtype=np.uint8) for t in strings] + [np.zeros(1, dtype=np.uint8)])
        start = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        self.bwt = np.where(pos > 0, flat[np.maximum(start[sid] + pos - 1, 0)], 255).astype(np.uint8)
        self.dollar_rows = np.flatnonzero(pos == 0).astype(np.uint32)
        self.dollar_ids = sid[pos == 0].astype(np.uint32)


_cache = {}


def expected(case):
    """the Expected of a tests.set_sufsort_sets case, computed once"""
    if case.id not in _cache:
        _cache[case.id] = Expected(case.strings)
    return _cache[case.id]
