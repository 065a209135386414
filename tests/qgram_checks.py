"""Shared helpers of the q-gram tests (tests/test_qgram_host.py, tests/test_qgram_gpu.py, tests/test_compat_qgram_gpu.py): packing the cases
of tests/qgram_cases.py for a device, and the check_* functions that run one layer of nvbio_amd.qgram on a device ("cpu" = the host
twins) and compare it with the definitions of tests/qgram_reference.py.  Every order is total, so every comparison is exact."""
import ctypes as C

import numpy as np
import torch

import nvbio_amd as nvb
from tests import qgram_cases as QC
from tests import qgram_reference as R
from tests import sufsort_texts as T


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def packed(sym, big_endian, dev):
    """the packed triple of a symbol array: exactly ceil(n / 16) words, nothing after them"""
    words = T.pack(sym, big_endian)
    return (torch.from_numpy(words.view(np.int32)).to(dev), len(sym), big_endian)


def packed_set(case, big_endian, dev):
    return nvb.PackedStringSet.from_host(case.words(big_endian), 2, big_endian, case.begin, case.length, case.fixed_length, device=dev)


def index_arrays(ix):
    """the index as the numpy arrays the reference has"""
    return u64(ix.qgrams), u32(ix.slots), u32(ix.index), None if ix.lut is None else u32(ix.lut)


def assert_index(ix, e):
    qgrams, slots, index, lut = index_arrays(ix)
    assert ix.n_unique == e.n_unique and ix.n_qgrams == e.n_qgrams
    assert (qgrams == e.qgrams).all() and (slots == e.slots).all() and slots[-1] == e.n_qgrams
    assert index.shape == e.index.shape and (index == e.index).all()
    assert (lut is None) == (e.lut is None)
    if lut is not None:
        assert lut.size == 4 ** e.ql + 1 and (lut == e.lut).all()


def check_string_builds(q, big_endian, dev):
    """-> every (index, reference) built, for the callers that go on with them"""
    built = {}
    for name, sym in QC.strings(q):
        text = packed(sym, big_endian, dev)
        assert (u64(nvb.generate_qgrams(text, q, device=dev)) == R.qgrams_at(sym, np.arange(len(sym)), q)).all()
        where = np.array([0, len(sym) - 1, len(sym) // 2, len(sym), len(sym) + 40, 0], dtype=np.uint32)      # past the end too
        assert (u64(nvb.generate_qgrams(text, q, where, device=dev)) == R.qgrams_at(sym, where, q)).all()
        for ql in QC.qluts(q):
            ix = nvb.QGramIndex.build(text, q, ql, device=dev)
            e = R.string_index(sym, q, ql)
            assert_index(ix, e)
            built[name, ql] = (ix, e)
    return built


def check_set_builds(q, big_endian, dev):
    built = {}
    for case in QC.sets():
        ss = packed_set(case, big_endian, dev)
        coords = np.array([(s, p) for s in range(case.n_strings + 1) for p in (0, 1, 17, 31, 99, 200)], dtype=np.uint32)
        assert (u64(nvb.generate_qgrams(ss, q, coords, device=dev)) == R.set_qgrams_at(case.strings, coords, q)).all()
        for interval in QC.INTERVALS:
            for ql in QC.qluts(q)[:2] if interval != 3 else QC.qluts(q):
                ix = nvb.QGramSetIndex.build(ss, q, interval, ql, device=dev)
                e = R.set_index(case.strings, q, interval, ql)
                assert_index(ix, e)
                built[case.id, interval, ql] = (ix, e)
    return built


def check_queries(ix, e, queries, dev):
    """range() of a batch as it is, sorted and shuffled; one query and none"""
    rng = np.random.default_rng(7)
    expect = e.ranges(queries)
    assert (u32(ix.range(queries)) == expect).all()
    order = np.argsort(queries, kind="stable")
    assert (u32(ix.range(queries[order])) == expect[order]).all()
    perm = rng.permutation(queries.size)
    shuffled = u32(ix.range(queries[perm]))
    back = np.empty_like(shuffled); back[perm] = shuffled
    assert (back == expect).all()                                        # the same ranges after un-permuting
    assert (u32(ix.range(queries[:1])) == expect[:1]).all()
    assert ix.range(queries[:0]).shape == (0, 2)


def batch_borders(ranges, slots, total):
    """borders inside [0, total]: in the middle of a query's range, and at a range's end where empty ranges follow"""
    sizes = (ranges[:, 1] - ranges[:, 0]).astype(np.int64)
    cuts = {0, total, total // 3}
    wide = np.flatnonzero(sizes >= 2)
    for j in wide[:2]:
        cuts.add(int(slots[j]) - int(sizes[j]) // 2)                     # inside query j's range
    before_empty = [j for j in range(len(sizes) - 1) if sizes[j] and not sizes[j + 1]]
    for j in before_empty[:2]:
        cuts.add(int(slots[j]))                                          # slots[j] == slots[j + 1]: on an empty range
    return sorted(cuts)


def check_filter(ix, e, queries, dev, intervals=(1, 10, 16)):
    """rank, locate whole and in batches, merge: -> the hits"""
    rng = np.random.default_rng(11)
    indices = rng.integers(0, 300, queries.size).astype(np.uint32)       # below many index positions: those diagonals wrap
    f = nvb.QGramFilter()
    total = f.rank(ix, torch.from_numpy(queries.view(np.int64)), torch.from_numpy(indices.view(np.int32)))
    ranges, slots, etotal = R.rank(e, queries)
    assert total == etotal == f.n_hits()
    assert (u32(f.ranges) == ranges).all() and (u64(f.slots) == slots).all()
    expect = R.locate(e, ranges, slots, indices, 0, total)
    whole = f.locate(0, total)
    assert whole.shape == expect.shape and (u32(whole) == expect).all()
    cuts = batch_borders(ranges, slots, total)
    parts = [u32(f.locate(a, b)) for a, b in zip(cuts[:-1], cuts[1:])]
    assert (np.concatenate(parts + [expect[:0]]) == expect).all()
    assert f.locate(total // 2, total // 2).shape[0] == 0                # begin == end
    for interval in intervals:
        if total:
            merged, counts = f.merge(interval, whole)
            em, ec = R.merge(expect, interval)
            assert u32(merged).shape == em.shape and (u32(merged) == em).all() and (u32(counts) == ec).all()
            assert int(ec.sum()) == total
    return whole


def string_filter_cases(q, big_endian, dev):
    for name, sym in QC.filter_strings(q):
        queries = QC.queries_for(R.string_index(sym, q, 0), np.random.default_rng(q))
        for ql in QC.qluts(q):
            yield nvb.QGramIndex.build(packed(sym, big_endian, dev), q, ql, device=dev), R.string_index(sym, q, ql), queries


def set_filter_cases(q, big_endian, dev):
    for case in QC.sets():
        if case.n_strings < 3:
            continue
        for interval in (1, 3):
            queries = QC.queries_for(R.set_index(case.strings, q, interval, 0), np.random.default_rng(q))
            for ql in QC.qluts(q)[-2:]:
                yield (nvb.QGramSetIndex.build(packed_set(case, big_endian, dev), q, interval, ql, device=dev),
                       R.set_index(case.strings, q, interval, ql), queries)


def check_merge_edges(dev):
    f = nvb.QGramFilter()
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.uint32).view(np.int32)).to(dev)
    # the reference's rounding, pinned: interval 10, diagonals 10 .. 19 -> remainders 0 .. 9; 2 * 5 > 10 is false, 2 * 6 > 10 is true,
    # and a diagonal that rounds up moves to r + 1, not to r + interval
    hits = np.array([(0, d) for d in range(10, 20)], dtype=np.uint32)
    merged, counts = f.merge(10, t(hits))
    assert u32(merged).tolist() == [10, 11] and u32(counts).tolist() == [6, 4]
    merged, counts = f.merge(16, t([(0, 8), (0, 9), (0, 15), (0, 16), (0, 31)]))
    assert u32(merged).tolist() == [0, 1, 16, 17] and u32(counts).tolist() == [1, 2, 1, 1]
    # query index below the index position: the diagonal wraps
    hits = np.array([(7, 2), (100, 0), (5, 5)], dtype=np.uint32)
    for interval in (1, 10, 16):
        merged, counts = f.merge(interval, t(hits))
        em, ec = R.merge(hits, interval)
        assert (u32(merged) == em).all() and (u32(counts) == ec).all()
    assert u32(f.merge(1, t(hits))[0]).tolist() == [0, 0xFFFFFF9C, 0xFFFFFFFB]
    # one hit; all hits on one diagonal
    merged, counts = f.merge(10, t([(3, 45)]))
    assert u32(merged).tolist() == [40] and u32(counts).tolist() == [1]
    merged, counts = f.merge(16, t([(p, p + 32) for p in range(1000)]))
    assert u32(merged).tolist() == [32] and u32(counts).tolist() == [1000]
    # set hits (string id, pos, query idx, 0) of several strings: ordered by string id first, then by diagonal
    hits = np.array([(2, 0, 5, 0), (0, 9, 3, 0), (2, 1, 6, 0), (1, 0, 77, 0), (0, 0, 17, 0), (2, 0, 18, 0)], dtype=np.uint32)
    for interval in (1, 10, 16):
        merged, counts = f.merge(interval, t(hits))
        em, ec = R.merge(hits, interval)
        assert u32(merged).shape == em.shape and (u32(merged) == em).all() and (u32(counts) == ec).all()
    merged, counts = f.merge(10, t(hits))                                # diagonals 5, -6, 5, 77, 17, 18 -> 0, -6, 0, 71, 11, 11
    assert u32(merged).tolist() == [[11, 0], [0xFFFFFFFA, 0], [71, 1], [0, 2], [11, 2]] and u32(counts).tolist() == [1, 1, 1, 2, 1]
    # no hits
    merged, counts = f.merge(10, t(np.zeros((0, 2), dtype=np.uint32)))
    assert merged.numel() == 0 and counts.numel() == 0
