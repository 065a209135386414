"""The wavelet tree and the FM-index over it by definition, in plain numpy (include/nvbio_hip.h, "Byte alphabets"): what the library's
arrays and answers must equal.  Nothing here imports the product."""
import numpy as np


def mask(text, S):
    return (np.asarray(text, dtype=np.uint8) & np.uint8((1 << S) - 1)).astype(np.uint8)


def tree_arrays(text, S):
    """-> (bits uint32 [W], splits uint32 [K], occ uint32 [K + W]) of the masked text"""
    t = mask(text, S).astype(np.int64)
    n, K = t.size, 1 << S
    W = (n * S + 31) // 32
    stream = np.zeros(W * 32, dtype=np.uint8)
    for l in range(S):
        order = np.argsort(t >> (S - l), kind="stable")           # stable by the top l bits
        stream[l * n:(l + 1) * n] = (t[order] >> (S - 1 - l)) & 1
    bits = np.packbits(stream).view(">u4").astype(np.uint32)       # global bit g = bit 31 - g % 32 of word g / 32
    ones = np.concatenate(([0], np.cumsum(stream, dtype=np.int64)))    # ones[g] = the 1 bits before bit g
    smaller = np.concatenate(([0], np.cumsum(np.bincount(t, minlength=K))))   # smaller[s] = the symbols below s
    splits = np.zeros(K, dtype=np.uint32)
    occ = np.zeros(K + W, dtype=np.uint32)
    for l in range(S):
        for j in range(1 << l):
            node, first = (1 << l) - 1 + j, j * (K >> l)
            splits[node] = smaller[first + (K >> (l + 1))]
            occ[node] = ones[l * n + smaller[first]]
    occ[K:] = ones[0:W * 32:32]
    return bits, splits, occ


def prefix_counts(text, S):
    """counts[c, i] = the occurrences of symbol c in [0, i), uint32 [K, n + 1]"""
    t = mask(text, S)
    K = 1 << S
    counts = np.zeros((K, t.size + 1), dtype=np.uint32)
    for c in np.unique(t):
        counts[c, 1:] = np.cumsum(t == c)
    return counts


def rank(counts, n, positions, symbols, S):
    """occurrences of symbols[i] & (K - 1) in [0, positions[i]]: a position in [n, 2^32 - 2] counts as n - 1, 2^32 - 1 gives 0"""
    p = np.asarray(positions, dtype=np.uint64)
    end = np.where(p == 0xFFFFFFFF, 0, np.minimum(p + 1, n)).astype(np.int64)
    c = np.asarray(symbols, dtype=np.int64) & ((1 << S) - 1)
    return counts[c, end].astype(np.uint32)


def text_at(text, S, positions):
    t = mask(text, S)
    p = np.asarray(positions, dtype=np.int64)
    return np.where(p < t.size, t[np.minimum(p, t.size - 1)], 0).astype(np.uint8)


def suffix_array(text, S):
    """uint32 [n + 1] by prefix doubling: SA[0] = n, a suffix that is a proper prefix of another first"""
    t = mask(text, S).astype(np.int64)
    n = t.size
    rank_ = t + 1                                                   # 0 = past the end
    h = 1
    while True:
        second = np.zeros(n, dtype=np.int64)
        second[:max(n - h, 0)] = rank_[h:]
        key = rank_ * (n + 2) + second
        order = np.argsort(key, kind="stable")
        sk = key[order]
        new = np.empty(n, dtype=np.int64)
        new[order] = np.concatenate(([1], 1 + np.cumsum(sk[1:] != sk[:-1])))
        rank_ = new
        if rank_.max() == n:
            sa = np.empty(n + 1, dtype=np.uint32)
            sa[0] = n
            sa[rank_] = np.arange(n)
            return sa
        h *= 2


def bwt(text, S, sa):
    """-> (bwt uint8 [n] with the '$' row dropped, primary)"""
    t = mask(text, S)
    primary = int(np.nonzero(sa == 0)[0][0])
    rows = np.delete(sa, primary).astype(np.int64)
    return t[rows - 1], primary


def ssa(sa, sa_int):
    out = sa[::sa_int].copy()
    out[0] = 0xFFFFFFFF
    return out


def L2(text, S):
    K = 1 << S
    return np.concatenate(([0], np.cumsum(np.bincount(mask(text, S), minlength=K)))).astype(np.uint32)


def match_rows(text, S, sa, pattern):
    """the inclusive SA range of a pattern by brute force over the sorted suffixes, or None where it does not occur (the search's
    answer is then any x > y); the empty pattern matches every row: (0, n)"""
    t = mask(text, S)
    n = t.size
    pattern = np.asarray(pattern, dtype=np.int64)
    m = pattern.size
    if m == 0:
        return 0, n
    if m > n or (pattern >= (1 << S)).any():
        return None
    windows = np.lib.stride_tricks.sliding_window_view(t, m)
    starts = np.nonzero((windows == pattern.astype(np.uint8)).all(axis=1))[0]
    if starts.size == 0:
        return None
    inverse = np.empty(n + 1, dtype=np.int64)
    inverse[sa.astype(np.int64)] = np.arange(n + 1)
    rows = np.sort(inverse[starts])
    assert rows[-1] - rows[0] + 1 == rows.size                      # the suffixes a pattern prefixes are contiguous
    return int(rows[0]), int(rows[-1])
