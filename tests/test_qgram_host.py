"""The `_host` twins of the q-gram entries, through the Python layer on device="cpu" and directly, against the definitions in plain numpy
(tests/qgram_reference.py); the argument checks of the device entries -- no GPU needed.  The checks themselves are in
tests/qgram_checks.py, and tests/test_qgram_gpu.py runs them again on the GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import nvbio_amd as nvb
from nvbio_amd import _lib
from tests import qgram_cases as QC
from tests import qgram_reference as R
from tests import sufsort_texts as T
from tests.qgram_checks import (_p, u32, assert_index, check_string_builds, check_set_builds, check_queries, check_filter, check_merge_edges,
                                string_filter_cases, set_filter_cases)

INVALID = 1      # hipErrorInvalidValue


@pytest.mark.parametrize("big_endian", [True, False], ids=["be", "le"])
@pytest.mark.parametrize("q", QC.QS)
def test_string_index_and_generate(q, big_endian):
    check_string_builds(q, big_endian, "cpu")


@pytest.mark.parametrize("big_endian", [True, False], ids=["be", "le"])
@pytest.mark.parametrize("q", QC.QS)
def test_set_index_and_generate(q, big_endian):
    built = check_set_builds(q, big_endian, "cpu")
    assert built["no_strings", 1, 0][0].n_qgrams == 0                    # a set that yields no seed: an index with one slot, 0
    lengths = {case.id: [len(t) for t in case.strings] for case in QC.sets()}
    for (name, interval, ql), (ix, e) in built.items():
        if interval == 1000:                                             # longer than every string: position 0 of each string that holds a q-gram
            assert ix.n_qgrams == sum(n >= q for n in lengths[name])
    assert q == 1 or built["fixed1", 1, 0][0].n_qgrams == 0                # only strings shorter than q


@pytest.mark.parametrize("q", QC.QS)
def test_string_queries_and_filter(q):
    for ix, e, queries in string_filter_cases(q, q % 2 == 0, "cpu"):
        check_queries(ix, e, queries, "cpu")
        check_filter(ix, e, queries, "cpu")


@pytest.mark.parametrize("q", QC.QS)
def test_set_queries_and_filter(q):
    for ix, e, queries in set_filter_cases(q, q % 2 == 1, "cpu"):
        check_queries(ix, e, queries, "cpu")
        check_filter(ix, e, queries, "cpu")


def test_merge_edges():
    check_merge_edges("cpu")


def test_zero_queries_rank_is_zero():
    ix = nvb.QGramIndex.build(np.arange(40) % 4, 5, 1, device="cpu")
    f = nvb.QGramFilter()
    assert f.rank(ix, np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32)) == 0
    assert f.locate(0, 0).shape == (0, 2)


def test_symbol_arrays_and_packed_sets_build_the_same_index():
    rng = np.random.default_rng(3)
    reads = [rng.integers(0, 4, n, dtype=np.uint8) for n in (40, 0, 25, 33)]
    a = nvb.QGramSetIndex.build(reads, 12, 3, 6, device="cpu")
    assert_index(a, R.set_index(reads, 12, 3, 6))
    text = rng.integers(0, 4, 100, dtype=np.uint8)
    assert_index(nvb.QGramIndex.build(text, 12, 6, device="cpu"), R.string_index(text, 12, 6))


def test_python_layer_refuses_what_the_entries_cannot_take():
    text = np.zeros(40, dtype=np.uint8)
    for q, ql in ((0, 0), (33, 0), (5, 6), (20, 17)):
        with pytest.raises(ValueError):
            nvb.QGramIndex.build(text, q, ql, device="cpu")
        with pytest.raises(ValueError):
            nvb.QGramSetIndex.build([text], q, 1, ql, device="cpu")
    with pytest.raises(ValueError):
        nvb.QGramSetIndex.build([text], 5, 0, device="cpu")
    with pytest.raises(ValueError, match="coords"):
        nvb.generate_qgrams([text], 5, device="cpu")
    four_bit = nvb.PackedStringSet(torch.zeros(4, dtype=torch.int32), 4, True, torch.zeros(1, dtype=torch.int64), torch.ones(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="2-bit"):
        nvb.QGramSetIndex.build(four_bit, 5, device="cpu")


def test_invalid_arguments_are_rejected_with_the_outputs_untouched():
    """q = 0 and 33, QL > q, bits = 4, a null pointer, temp one byte short: hipErrorInvalidValue from the device entries (before anything
    is launched, so host arrays stand in for device memory) and from the host twins, and no output word changes"""
    L = nvb.lib()
    n, q = 100, 12
    sym = np.random.default_rng(5).integers(0, 4, n, dtype=np.uint8)
    words = T.pack(sym, True)
    F = 0xDEADBEEF
    outs = dict(qgrams=np.full(n, F, dtype=np.uint64), slots=np.full(n + 1, F, dtype=np.uint32), index=np.full(2 * n, F, dtype=np.uint32),
                lut=np.full(4 ** 6 + 1, F, dtype=np.uint32))
    n_unique = C.c_uint32(F)
    temp = np.zeros(16, dtype=np.uint8)
    big = 1 << 40

    def untouched():
        return all((a == F).all() for a in outs.values()) and n_unique.value == F

    def build(words=words, bits=2, q=q, ql=6, qgrams=outs["qgrams"], slots=outs["slots"], lut=outs["lut"], temp=temp, tb=big, host=False):
        if host:
            return L.nvbio_hip_qgram_index_build_host(_p(words), 7, bits, 1, n, q, ql, _p(qgrams), _p(slots), _p(outs["index"]), _p(lut), C.byref(n_unique), 1)
        return L.nvbio_hip_qgram_index_build(_p(words), 7, bits, 1, n, q, ql, _p(qgrams), _p(slots), _p(outs["index"]), _p(lut), C.byref(n_unique), _p(temp), tb, None)

    tb = L.nvbio_hip_qgram_index_build_temp_bytes(n)
    assert tb >= 2 * 8 * n + 4 * n + 4 * n
    for host in (False, True):
        assert build(q=0, host=host) == INVALID and build(q=33, host=host) == INVALID
        assert build(q=5, ql=6, host=host) == INVALID and build(q=20, ql=17, host=host) == INVALID
        assert build(bits=4, host=host) == INVALID
        assert build(words=None, host=host) == INVALID and build(qgrams=None, host=host) == INVALID
        assert build(slots=None, host=host) == INVALID and build(lut=None, host=host) == INVALID
        assert untouched()
    assert build(temp=None) == INVALID and build(tb=tb - 1) == INVALID and untouched()

    # the set entries
    s = _lib.StringSetStruct()
    begin, length = np.array([0, 50], dtype=np.uint64), np.array([50, 50], dtype=np.uint32)
    s.words, s.n_words, s.bits, s.big_endian, s.begin, s.length = words.ctypes.data, 7, 2, 1, begin.ctypes.data, length.ctypes.data
    count = C.c_uint64(F)

    def changed(**kw):
        t = _lib.StringSetStruct.from_buffer_copy(s)
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    def set_build(st=s, q=q, interval=1, ql=6, nq=78, slots=outs["slots"], temp=temp, tb=big, host=False):
        st = C.byref(st) if st is not None else None
        if host:
            return L.nvbio_hip_qgram_set_index_build_host(st, 2, q, interval, ql, nq, _p(outs["qgrams"]), _p(slots), _p(outs["index"]), _p(outs["lut"]),
                                                          C.byref(n_unique), 1)
        return L.nvbio_hip_qgram_set_index_build(st, 2, q, interval, ql, nq, _p(outs["qgrams"]), _p(slots), _p(outs["index"]), _p(outs["lut"]),
                                                 C.byref(n_unique), _p(temp), tb, None)

    set_tb = L.nvbio_hip_qgram_set_index_build_temp_bytes(78, 2)
    for host in (False, True):
        assert set_build(st=None, host=host) == INVALID and set_build(st=changed(bits=4), host=host) == INVALID
        assert set_build(st=changed(words=None), host=host) == INVALID and set_build(st=changed(begin=None), host=host) == INVALID
        assert set_build(q=0, host=host) == INVALID and set_build(q=33, host=host) == INVALID and set_build(q=5, ql=6, host=host) == INVALID
        assert set_build(interval=0, host=host) == INVALID and set_build(slots=None, host=host) == INVALID
        assert set_build(st=changed(length=None, fixed_length=50), nq=77, host=host) == INVALID       # 2 * 39 seeds are not 77
        assert untouched()
    assert set_build(temp=None) == INVALID and set_build(tb=set_tb - 1) == INVALID and untouched()
    assert set_build(nq=77, host=True) == INVALID and untouched()                                    # the twin counts the seeds itself
    assert L.nvbio_hip_qgram_set_count_seeds(C.byref(s), 2, 0, 1, C.byref(count), _p(temp), big, None) == INVALID
    assert L.nvbio_hip_qgram_set_count_seeds(C.byref(s), 2, q, 0, C.byref(count), _p(temp), big, None) == INVALID
    assert L.nvbio_hip_qgram_set_count_seeds(C.byref(s), 2, q, 1, C.byref(count), None, big, None) == INVALID
    assert L.nvbio_hip_qgram_set_count_seeds(C.byref(s), 2, q, 1, C.byref(count), _p(temp), L.nvbio_hip_qgram_set_count_seeds_temp_bytes(2) - 1, None) == INVALID
    assert count.value == F
    assert L.nvbio_hip_qgram_set_count_seeds(C.byref(changed(length=None, fixed_length=50)), 2, q, 1, C.byref(count), None, 0, None) == 0 and count.value == 78

    # generate, range, rank, locate, merge
    e = R.string_index(sym, q, 6)
    ix = _lib.QGramIndexStruct()
    lut = np.ascontiguousarray(e.lut)
    ix.qgrams, ix.slots, ix.index, ix.lut = e.qgrams.ctypes.data, e.slots.ctypes.data, e.index.ctypes.data, lut.ctypes.data
    ix.q, ix.ql, ix.n_unique, ix.n_qgrams = q, 6, e.n_unique, n

    def ix_changed(**kw):
        t = _lib.QGramIndexStruct.from_buffer_copy(ix)
        for k, v in kw.items():
            setattr(t, k, v)
        return C.byref(t)

    queries = e.qgrams[:8].copy()
    ranges, slots8 = np.full(16, F, dtype=np.uint32), np.full(8, F, dtype=np.uint64)
    total = C.c_uint64(F)
    g = outs["qgrams"]
    assert L.nvbio_hip_qgram_generate(_p(words), 7, 2, 1, n, 0, None, n, _p(g), None) == INVALID
    assert L.nvbio_hip_qgram_generate(_p(words), 7, 2, 1, n, 33, None, n, _p(g), None) == INVALID
    assert L.nvbio_hip_qgram_generate(_p(words), 7, 4, 1, n, q, None, n, _p(g), None) == INVALID
    assert L.nvbio_hip_qgram_generate(None, 7, 2, 1, n, q, None, n, _p(g), None) == INVALID
    assert L.nvbio_hip_qgram_generate(_p(words), 7, 2, 1, n, q, None, n, None, None) == INVALID
    assert L.nvbio_hip_qgram_generate_host(_p(words), 7, 2, 1, n, 33, None, n, _p(g), 1) == INVALID
    assert L.nvbio_hip_qgram_set_generate(C.byref(changed(bits=4)), 2, q, _p(ranges), 8, _p(g), None) == INVALID
    assert L.nvbio_hip_qgram_set_generate(C.byref(s), 2, q, None, 8, _p(g), None) == INVALID
    for bad in (ix_changed(q=0), ix_changed(q=33), ix_changed(q=5), ix_changed(slots=None), ix_changed(lut=None), ix_changed(qgrams=None), None):
        assert L.nvbio_hip_qgram_range(bad, _p(queries), 8, _p(ranges), None) == INVALID
        assert L.nvbio_hip_qgram_range_host(bad, _p(queries), 8, _p(ranges), 1) == INVALID
        assert L.nvbio_hip_qgram_rank(bad, _p(queries), 8, _p(ranges), _p(slots8), C.byref(total), _p(temp), big, None) == INVALID
        assert L.nvbio_hip_qgram_rank_host(bad, _p(queries), 8, _p(ranges), _p(slots8), C.byref(total), 1) == INVALID
        assert L.nvbio_hip_qgram_locate(bad, 8, _p(ranges), _p(slots8), _p(ranges), 0, 4, _p(outs["index"]), None) == INVALID
        assert L.nvbio_hip_qgram_set_locate_host(bad, 8, _p(ranges), _p(slots8), _p(ranges), 0, 4, _p(outs["index"]), 1) == INVALID
    good = C.byref(ix)
    assert L.nvbio_hip_qgram_range(good, None, 8, _p(ranges), None) == INVALID and L.nvbio_hip_qgram_range(good, _p(queries), 8, None, None) == INVALID
    assert L.nvbio_hip_qgram_rank(good, _p(queries), 8, _p(ranges), None, C.byref(total), _p(temp), big, None) == INVALID
    assert L.nvbio_hip_qgram_rank(good, _p(queries), 8, _p(ranges), _p(slots8), C.byref(total), None, big, None) == INVALID
    assert L.nvbio_hip_qgram_rank(good, _p(queries), 8, _p(ranges), _p(slots8), C.byref(total), _p(temp), L.nvbio_hip_qgram_rank_temp_bytes(8) - 1, None) == INVALID
    assert L.nvbio_hip_qgram_locate(good, 8, _p(ranges), _p(slots8), _p(ranges), 5, 4, _p(outs["index"]), None) == INVALID       # begin > end
    assert L.nvbio_hip_qgram_locate(good, 8, None, _p(slots8), _p(ranges), 0, 4, _p(outs["index"]), None) == INVALID
    assert L.nvbio_hip_qgram_locate(good, 8, _p(ranges), _p(slots8), _p(ranges), 0, 4, None, None) == INVALID
    n_merged = C.c_uint32(F)
    hits = np.zeros(16, dtype=np.uint32)
    for name in ("nvbio_hip_qgram_merge", "nvbio_hip_qgram_set_merge"):
        f, tbm = getattr(L, name), getattr(L, name + "_temp_bytes")(4)
        assert f(_p(hits), 4, 0, _p(outs["index"]), _p(outs["slots"]), C.byref(n_merged), _p(temp), big, None) == INVALID       # interval 0
        assert f(None, 4, 10, _p(outs["index"]), _p(outs["slots"]), C.byref(n_merged), _p(temp), big, None) == INVALID
        assert f(_p(hits), 4, 10, None, _p(outs["slots"]), C.byref(n_merged), _p(temp), big, None) == INVALID
        assert f(_p(hits), 4, 10, _p(outs["index"]), _p(outs["slots"]), C.byref(n_merged), None, big, None) == INVALID
        assert f(_p(hits), 4, 10, _p(outs["index"]), _p(outs["slots"]), C.byref(n_merged), _p(temp), tbm - 1, None) == INVALID
        assert getattr(L, name + "_host")(_p(hits), 4, 0, _p(outs["index"]), _p(outs["slots"]), C.byref(n_merged), 1) == INVALID
    assert untouched() and (ranges == F).all() and (slots8 == F).all() and total.value == F and n_merged.value == F
