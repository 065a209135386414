"""The inputs of the q-gram tests (tests/test_qgram_host.py, tests/test_qgram_gpu.py, tests/test_compat_qgram_gpu.py): the smallest
at which each step of nvbio_amd/csrc/qgram.hip can still go wrong.  Symbols 0..3 = ACGT."""
import numpy as np

from tests.set_sufsort_sets import SetCase

QS = [1, 3, 12, 16, 17, 20, 31, 32]
INTERVALS = [1, 3, 10, 1000]            # 1000 is longer than every string of every set below
U64 = np.uint64


def qluts(q):
    """0, 1, 6 and q itself where q <= 8 -- those that the limit QL <= min(q, 16) admits"""
    return sorted({ql for ql in (0, 1, 6, q if q <= 8 else 0) if ql <= q})


def strings(q):
    """(id, symbols): lengths round q, the 16-symbol word and the 64-bit window; all-A, where the truncated q-grams of the tail equal
    full ones; a period-7 repeat with long slot runs; a 4 096-symbol i.i.d. text (more than one block of the all-positions kernel)"""
    rng = np.random.default_rng(500 + q)
    out = []
    for n in sorted({1, max(q - 1, 1), q, 15, 16, 17, 31, 32, 33, 64, 65}):
        out.append(("iid%d" % n, rng.integers(0, 4, n, dtype=np.uint8)))
    out.append(("allA70", np.zeros(70, dtype=np.uint8)))
    out.append(("period7", np.tile(rng.integers(0, 4, 7, dtype=np.uint8), 30)[:203]))
    out.append(("iid4096", rng.integers(0, 4, 4096, dtype=np.uint8)))
    return out


def filter_strings(q):
    """the strings the query and filter tests run on"""
    return [(i, t) for i, t in strings(q) if i in ("iid33", "allA70", "period7", "iid4096")]


def sets():
    rng = np.random.default_rng(808)
    iid = lambda n: rng.integers(0, 4, n, dtype=np.uint8)
    out = []
    lens = [0, 5, 33, 0, 50, 100, 31, 32, 1, 64, 0]
    stream = iid(sum(lens))
    begin = np.concatenate([[0], np.cumsum(lens)[:-1]])
    out.append(SetCase("concatenated_with_empty_and_short", stream, begin, lens))
    stream = iid(301)
    out.append(SetCase("unaligned_out_of_order_overlapping", stream, [201, 3, 77, 77, 150, 300, 5], [100, 70, 33, 64, 0, 1, 40]))
    out.append(SetCase("ends_with_the_stream", stream, [0, 269], [40, 32]))                    # the n_words clamp: no word follows
    for n in (1, 33, 40):
        out.append(SetCase("fixed%d" % n, iid(3 + 6 * n), 3 + n * np.arange(6), None, n))
    out.append(SetCase("same_read_x3", np.tile(iid(45), 3), [0, 45, 90], [45, 45, 45]))          # ties between strings: by id
    out.append(SetCase("no_strings", iid(4), [], []))
    return out


def queries_for(ref, rng):
    """Query q-grams for the index `ref` (a qgram_reference.Index built with ql == 0): present ones; absent ones below the first, above
    the last and between two; for every LUT size of qluts(q), absent ones in empty buckets, in buckets that also hold present q-grams
    and in the last bucket; duplicates; random words of 2q bits."""
    q = ref.q
    top = (1 << (2 * q)) - 1
    present = [int(g) for g in ref.qgrams]
    have = set(present)
    out = [present[i] for i in rng.permutation(len(present))[:40]]
    out += [0, top, 1 % (top + 1)]
    if present:
        out += [max(present[0] - 1, 0), min(present[-1] + 1, top)]
        out += [g + 1 for g in present[:200] if g + 1 <= top and g + 1 not in have][:10]         # between two, in the bucket of a present one
    for ql in qluts(q):
        if ql == 0:
            continue
        sh = 2 * (q - ql)
        occupied = {g >> sh for g in present}
        empty = [k for k in range(4 ** ql) if k not in occupied]
        for k in empty[:4] + empty[-4:]:
            out += [k << sh, ((k + 1) << sh) - 1]
        out += [(4 ** ql - 1) << sh]                                                            # the first word of the last bucket
        for k in sorted(occupied)[:4]:
            out += [g for g in (k << sh, ((k + 1) << sh) - 1, (k << sh) + 1) if g not in have][:2]
    out += out[:5]                                                                              # duplicates
    out += [int(g) & top for g in rng.integers(0, 1 << 63, 20, dtype=np.uint64)]
    return np.array(out, dtype=U64)


def medium_text():
    """100 000 i.i.d. symbols with 10 % planted repeats: a hundred copies of one 100-symbol unit"""
    rng = np.random.default_rng(31337)
    text = rng.integers(0, 4, 100000, dtype=np.uint8)
    unit = rng.integers(0, 4, 100, dtype=np.uint8)
    for p in rng.choice(990, 100, replace=False) * 100:
        text[p:p + 100] = unit
    return text


def medium_reads(text):
    """2 000 reads of 50 to 150 symbols of the medium text"""
    rng = np.random.default_rng(4711)
    lens = rng.integers(50, 151, 2000)
    starts = rng.integers(0, len(text) - 150, 2000)
    return [text[s:s + n] for s, n in zip(starts, lens)]
