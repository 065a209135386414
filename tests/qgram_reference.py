"""The q-gram index and filter by definition, in plain numpy (include/nvbio_hip.h, "Q-gram indices and the q-gram filter"): what
tests/test_qgram_host.py, tests/test_qgram_gpu.py and tests/test_compat_qgram_gpu.py compare every layer with.  Nothing here looks at a
LUT when it answers a query: a range is a plain search of the distinct q-grams, so a LUT that narrows wrongly shows."""
import numpy as np

U64 = np.uint64


def qgrams_at(sym, positions, q):
    """the q-grams of the string `sym` at `positions` (uint64): symbol j of a q-gram at bits [2j, 2j + 2), symbols past the end 0"""
    sym = np.asarray(sym, dtype=np.uint8)
    positions = np.asarray(positions, dtype=np.int64)
    pad = np.zeros(sym.size + 33, dtype=U64)
    pad[:sym.size] = sym
    out = np.zeros(positions.size, dtype=U64)
    inside = positions < sym.size
    p = np.where(inside, positions, sym.size)           # a position past the end reads only padding
    for j in range(q):
        out |= pad[np.minimum(p + j, sym.size + 32)] << U64(2 * j)
    return out


def set_qgrams_at(strings, coords, q):
    """the q-grams of a string set at (string id, position) pairs; an id past the set gives 0"""
    coords = np.asarray(coords, dtype=np.int64).reshape(-1, 2)
    lens = np.array([len(t) for t in strings] + [0], dtype=np.int64)               # one empty string for the ids past the set
    offs = np.concatenate([[0], np.cumsum(lens + 33)])                              # 33 symbols of padding after every string
    flat = np.zeros(int(offs[-1]), dtype=U64)
    for t, o in zip(strings, offs):
        flat[o:o + len(t)] = t
    s = np.minimum(coords[:, 0], len(strings))
    p = offs[s] + np.minimum(coords[:, 1], lens[s])                                 # a position past the end reads only padding
    out = np.zeros(coords.shape[0], dtype=U64)
    for j in range(q):
        out |= flat[p + j] << U64(2 * j)
    return out


def set_seeds(strings, q, interval):
    """the (string id, pos) pairs of uniform_seeds_functor(q, interval): by string, then by position, while pos + q <= length"""
    out = [(s, p) for s, t in enumerate(strings) for p in range(0, len(t) - q + 1, interval)]
    return np.array(out, dtype=np.uint32).reshape(-1, 2)


class Index:
    def __init__(self, keys, coords, q, ql):
        keys = np.asarray(keys, dtype=U64)
        order = np.argsort(keys, kind="stable")          # ties stay in enumeration order
        self.q, self.ql, self.n_qgrams = q, ql, keys.size
        self.qgrams, counts = np.unique(keys, return_counts=True)
        self.n_unique = self.qgrams.size
        self.slots = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
        self.index = np.asarray(coords, dtype=np.uint32)[order]
        self.lut = None
        if ql:
            firsts = np.arange(4 ** ql, dtype=U64) << U64(2 * (q - ql))
            self.lut = np.concatenate([np.searchsorted(self.qgrams, firsts, side="left"), [self.n_unique]]).astype(np.uint32)

    def ranges(self, queries):
        queries = np.asarray(queries, dtype=U64)
        i = np.searchsorted(self.qgrams, queries, side="left")
        found = (i < self.n_unique) & (self.qgrams[np.minimum(i, max(self.n_unique - 1, 0))] == queries) if self.n_unique else np.zeros(queries.size, bool)
        k = np.where(found, i, 0)
        out = np.zeros((queries.size, 2), dtype=np.uint32)
        if self.n_unique:
            out[:, 0] = np.where(found, self.slots[k], 0)
            out[:, 1] = np.where(found, self.slots[k + 1], 0)
        return out


def string_index(sym, q, ql):
    n = len(sym)
    return Index(qgrams_at(sym, np.arange(n), q), np.arange(n, dtype=np.uint32), q, ql)


def set_index(strings, q, interval, ql):
    coords = set_seeds(strings, q, interval)
    return Index(set_qgrams_at(strings, coords, q), coords, q, ql)


def rank(index, queries):
    """(ranges, slots = the inclusive 64-bit sums of the range sizes, total)"""
    r = index.ranges(queries)
    slots = np.cumsum((r[:, 1] - r[:, 0]).astype(U64), dtype=U64)
    return r, slots, int(slots[-1]) if slots.size else 0


def locate(index, ranges, slots, indices, begin, end):
    """hits [begin, end): rows (index coordinate.., query index[, 0])"""
    is_set = index.index.ndim == 2
    out = np.zeros((end - begin, 4 if is_set else 2), dtype=np.uint32)
    o = np.arange(begin, end, dtype=U64)
    slot = np.searchsorted(slots, o, side="right")
    base = np.where(slot > 0, slots[np.maximum(slot, 1) - 1], U64(0)).astype(U64)
    at = ranges[slot, 0].astype(np.int64) + (o - base).astype(np.int64)
    if is_set:
        out[:, 0:2] = index.index[at]
        out[:, 2] = np.asarray(indices, dtype=np.uint32)[slot]
    else:
        out[:, 0] = index.index[at]
        out[:, 1] = np.asarray(indices, dtype=np.uint32)[slot]
    return out


def snap(diag, interval):
    """the reference's util::round(diag, interval) as written: r = (diag / interval) * interval, and r + 1 -- one, not interval -- where
    uint32((diag - r) * 2) > interval"""
    diag = np.asarray(diag, dtype=np.uint32)
    r = (diag // np.uint32(interval)) * np.uint32(interval)
    up = ((diag - r) * np.uint32(2)) > np.uint32(interval)
    return np.where(up, r + np.uint32(1), r).astype(np.uint32)


def merge(hits, interval):
    """(merged keys ascending, counts): uint32 diagonals for [n, 2] hits; (diagonal, string id) rows, ordered by string id first, for
    [n, 4] hits"""
    hits = np.asarray(hits, dtype=np.uint32)
    if hits.shape[1] == 2:
        keys, counts = np.unique(snap(hits[:, 1] - hits[:, 0], interval), return_counts=True)
        return keys.astype(np.uint32), counts.astype(np.uint32)
    words = (hits[:, 0].astype(U64) << U64(32)) | snap(hits[:, 2] - hits[:, 1], interval).astype(U64)
    keys, counts = np.unique(words, return_counts=True)
    merged = np.stack([(keys & U64(0xFFFFFFFF)).astype(np.uint32), (keys >> U64(32)).astype(np.uint32)], axis=1)
    return merged, counts.astype(np.uint32)
