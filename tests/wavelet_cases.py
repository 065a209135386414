"""The texts the wavelet-tree and wavelet FM-index tests share (tests/test_wavelet_host.py, tests/test_wavelet_gpu.py)."""
import collections

import numpy as np

TreeCase = collections.namedtuple("TreeCase", "id S text")
FMCase = collections.namedtuple("FMCase", "id S text")

# the reference's own seven known ranks (nvbio-test/wavelet_test.cu): positions, symbols, results
KNOWN_P = (0, 1, 2, 2, 3, 4, 5)
KNOWN_C = (41, 59, 59, 41, 41, 59, 0)
KNOWN_R = (1, 1, 2, 1, 2, 3, 0)

PROTEIN_TEXT = "ACDEFGHIKLMNOPQRSTVWYBZX"      # the text of the reference's examples/waveletfm: every suffix occurs once


def _rng(seed):
    return np.random.default_rng(seed)


def known_ranks_text():
    t = _rng(41).integers(1, 256, 1000, dtype=np.uint8)
    t[:5] = (41, 59, 59, 41, 59)
    t[5] = 7
    return t


def tree_cases():
    r = _rng(2024)
    out = [
        TreeCase("s1_n1", 1, np.array([1], dtype=np.uint8)),
        TreeCase("s8_n1_255", 8, np.array([255], dtype=np.uint8)),
        TreeCase("s1_n31", 1, r.integers(0, 2, 31, dtype=np.uint8)),
        TreeCase("s1_n32", 1, r.integers(0, 2, 32, dtype=np.uint8)),
        TreeCase("s1_n33", 1, r.integers(0, 2, 33, dtype=np.uint8)),
        TreeCase("s8_n64", 8, r.integers(0, 256, 64, dtype=np.uint8)),              # every level starts on a word
        TreeCase("s5_n33", 5, r.integers(0, 32, 33, dtype=np.uint8)),               # levels start inside a word
        TreeCase("s3_n97", 3, r.integers(0, 8, 97, dtype=np.uint8)),
        TreeCase("known_ranks", 8, known_ranks_text()),
        TreeCase("s8_two_values", 8, (r.integers(0, 2, 1000, dtype=np.uint8) * 255).astype(np.uint8)),     # nearly every node is empty
        TreeCase("s8_const200", 8, np.full(70, 200, dtype=np.uint8)),
        TreeCase("s8_const0", 8, np.zeros(40, dtype=np.uint8)),
        TreeCase("s8_24values", 8, r.integers(0, 24, 4097, dtype=np.uint8)),
        TreeCase("s5_24values", 5, r.integers(0, 24, 4097, dtype=np.uint8)),
        TreeCase("s8_n20011", 8, r.integers(0, 256, 20011, dtype=np.uint8)),         # several blocks of any kernel, a tail in each
        TreeCase("s4_n300007", 4, r.integers(0, 16, 300007, dtype=np.uint8)),
        TreeCase("s5_high_bits", 5, r.integers(0, 256, 333, dtype=np.uint8)),        # bits above S set: the tree of the masked text
        TreeCase("s3_high_bits", 3, (r.integers(0, 8, 97, dtype=np.uint8) | 0xA8).astype(np.uint8)),
    ]
    return out


def zero_runs_text():
    """ends in ten 0 symbols, with 0-runs of 6 to 12 inside: the pad of the round-0 key equals the smallest symbol (K0 = 7 at S = 8)"""
    r = _rng(77)
    parts = []
    for run in (6, 7, 8, 9, 10, 11, 12, 7, 6, 12):
        parts.append(r.integers(0, 5, int(r.integers(3, 30)), dtype=np.uint8))
        parts.append(np.zeros(run, dtype=np.uint8))
    parts.append(r.integers(1, 5, 20, dtype=np.uint8))
    parts.append(np.zeros(10, dtype=np.uint8))
    return np.concatenate(parts)


def fm_cases():
    r = _rng(4242)
    from nvbio_amd import alphabet
    iid4 = r.integers(0, 4, 1000, dtype=np.uint8)
    return [
        FMCase("protein24", 8, alphabet.encode(PROTEIN_TEXT)),
        FMCase("n1", 8, np.array([9], dtype=np.uint8)),
        FMCase("seven_seven", 8, np.array([7, 7], dtype=np.uint8)),
        FMCase("const300", 8, np.full(300, 33, dtype=np.uint8)),
        FMCase("repeat13x400", 8, np.tile(r.integers(0, 256, 13, dtype=np.uint8), 400)),       # about ten doubling rounds
        FMCase("iid4_s8", 8, iid4),
        FMCase("iid4_s2", 2, iid4),
        FMCase("iid256", 8, r.integers(0, 256, 8191, dtype=np.uint8)),
        FMCase("iid24_s5", 5, r.integers(0, 24, 20011, dtype=np.uint8)),
        FMCase("zero_runs", 8, zero_runs_text()),
    ]


def fm_patterns(case, seed=9):
    """patterns cut from the text (lengths 1 to 40), mutated copies, patterns with a symbol absent from the text, a symbol >= K, the empty one"""
    r = _rng(seed)
    t, S = case.text, case.S
    n, K = t.size, 1 << S
    masked = t & np.uint8(K - 1)
    present = np.unique(masked)
    absent = np.setdiff1d(np.arange(K), present)
    out = [np.zeros(0, dtype=np.uint8)]
    for _ in range(60):
        m = int(r.integers(1, 41))
        at = int(r.integers(0, n))
        p = masked[at:at + m].copy()
        out.append(p)
        q = p.copy()
        q[int(r.integers(0, q.size))] = present[int(r.integers(0, present.size))]
        out.append(q)
        if absent.size:
            a = p.copy()
            a[int(r.integers(0, a.size))] = absent[int(r.integers(0, absent.size))]
            out.append(a)
        if K < 256:
            b = p.copy()
            b[int(r.integers(0, b.size))] = int(r.integers(K, 256))
            out.append(b)
    out.append(masked.copy())                                       # the whole text
    if K < 256:
        out.append(np.array([K], dtype=np.uint8))                   # exactly K: the reference's c > K lets this one through
    return out
