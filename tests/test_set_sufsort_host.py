"""The `_host` twins of the string-set suffix sorter and BWT against the definition (tests/set_sufsort_reference.py), the argument checks
of the device entries and the Python layer's refusals -- no GPU needed."""
import ctypes as C

import numpy as np
import pytest

import nvbio_amd
from nvbio_amd import _lib
from tests import set_sufsort_reference as R
from tests import set_sufsort_sets as S
from tests import sufsort_texts as T

INVALID = 1      # hipErrorInvalidValue


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def host_struct(case, big_endian):
    """(nvbio_hip_string_set over host arrays, the arrays that must outlive it)"""
    words = case.words(big_endian)
    s = _lib.StringSetStruct()
    s.words, s.n_words, s.bits, s.big_endian = words.ctypes.data, words.size, 2, int(big_endian)
    s.begin = case.begin.ctypes.data
    s.length = case.length.ctypes.data if case.length is not None else None
    s.fixed_length = case.fixed_length
    return s, (words, case.begin, case.length)


def host_set_suffix_sort(case, big_endian=True, optional=True, n_threads=2):
    s, keep = host_struct(case, big_endian)
    n, N = case.n_suffixes, case.n_strings
    suffixes = np.full(n, 0xDEADBEEF, dtype=np.uint32)
    ids = np.full(n, 0xDEADBEEF, dtype=np.uint32) if optional else None
    cum = np.full(N, 0xDEADBEEF, dtype=np.uint32) if optional else None
    assert nvbio_amd.lib().nvbio_hip_set_suffix_sort_host(C.byref(s), N, n, _p(suffixes), _p(ids), _p(cum), n_threads) == 0
    return suffixes, ids, cum


def host_set_bwt(case, big_endian=True, want_pairs=True, n_threads=2):
    s, keep = host_struct(case, big_endian)
    n, N = case.n_suffixes, case.n_strings
    bwt = np.full(n, 0xEE, dtype=np.uint8)
    rows = np.full(N, 0xDEADBEEF, dtype=np.uint32)
    ids = np.full(N, 0xDEADBEEF, dtype=np.uint32)
    pairs = np.full(2 * n, 0xDEADBEEF, dtype=np.uint32) if want_pairs else None
    assert nvbio_amd.lib().nvbio_hip_set_bwt_host(C.byref(s), N, n, _p(bwt), _p(rows), _p(ids), _p(pairs), n_threads) == 0
    return bwt, rows, ids, pairs


def check_sort(got, e):
    suffixes, ids, cum = got
    assert (suffixes == e.suffixes).all()
    assert (suffixes[:e.n_strings] == e.cum - 1).all()                  # rows 0 .. N - 1: the empty suffixes in id order
    if ids is not None:
        assert (ids == e.string_ids).all() and (cum == e.cum).all()


def check_bwt(got, e):
    bwt, rows, ids, pairs = got
    assert (bwt == e.bwt).all() and (rows == e.dollar_rows).all() and (ids == e.dollar_ids).all()
    if pairs is not None:
        assert (pairs == e.pairs).all()


ALL = S.all_small()


@pytest.mark.parametrize("big_endian", [True, False], ids=["be", "le"])
@pytest.mark.parametrize("case", ALL, ids=[c.id for c in ALL])
def test_host_twins_equal_the_definition(case, big_endian):
    e = R.expected(case)
    assert e.n_suffixes == case.n_suffixes
    check_sort(host_set_suffix_sort(case, big_endian), e)
    check_bwt(host_set_bwt(case, big_endian), e)


@pytest.mark.parametrize("text", [t for _, t in T.small_texts()], ids=[i for i, _ in T.small_texts()])
def test_one_string_is_the_plain_suffix_array(text):
    """a set of one string: the sorted global indices are the plain sorter's suffix array, element for element"""
    sa = np.empty(len(text) + 1, dtype=np.uint32)
    assert nvbio_amd.lib().nvbio_hip_suffix_sort_host(_p(T.pack(text, True)), 2, 1, len(text), _p(sa), 2) == 0
    assert (host_set_suffix_sort(S.concatenated("one", [text]))[0] == sa).all()


def test_medium_set_and_optional_outputs():
    case = S.medium_case()
    e = R.expected(case)
    assert 380000 < e.n_suffixes < 410000
    check_sort(host_set_suffix_sort(case, True, optional=False, n_threads=0), e)
    check_bwt(host_set_bwt(case, False, want_pairs=False, n_threads=0), e)


def test_host_twins_refuse_a_wrong_suffix_count_with_the_outputs_untouched():
    case = S.concatenated("three", [np.zeros(5, np.uint8), np.ones(3, np.uint8), np.zeros(0, np.uint8)])
    s, keep = host_struct(case, True)
    L = nvbio_amd.lib()
    for n in (case.n_suffixes + 1, case.n_suffixes - 1):
        out = np.full(n + 8, 0xDEADBEEF, dtype=np.uint32)
        bwt = np.full(n + 8, 0xEE, dtype=np.uint8)
        rows, ids = np.full(3, 0xDEADBEEF, dtype=np.uint32), np.full(3, 0xDEADBEEF, dtype=np.uint32)
        assert L.nvbio_hip_set_suffix_sort_host(C.byref(s), 3, n, _p(out), None, None, 1) == INVALID
        assert L.nvbio_hip_set_bwt_host(C.byref(s), 3, n, _p(bwt), _p(rows), _p(ids), None, 1) == INVALID
        assert (out == 0xDEADBEEF).all() and (bwt == 0xEE).all() and (rows == 0xDEADBEEF).all() and (ids == 0xDEADBEEF).all()


def test_invalid_arguments_are_rejected_without_a_gpu():
    L = nvbio_amd.lib()
    case = S.concatenated("two", [np.zeros(40, np.uint8), np.ones(9, np.uint8)])
    n, N = case.n_suffixes, case.n_strings
    s, keep = host_struct(case, True)          # host arrays: every call below is refused before anything reads them
    out, bwt = np.zeros(2 * n, dtype=np.uint32), np.zeros(n, dtype=np.uint8)
    rows, ids = np.zeros(N, dtype=np.uint32), np.zeros(N, dtype=np.uint32)
    temp = np.zeros(16, dtype=np.uint8)
    big = 1 << 40
    sort_tb, bwt_tb = L.nvbio_hip_set_suffix_sort_temp_bytes(n, N), L.nvbio_hip_set_bwt_temp_bytes(n, N)
    assert sort_tb >= 40 * n + 8 * N and bwt_tb >= sort_tb + 4 * n
    assert L.nvbio_hip_set_suffix_sort_temp_bytes(n, 0) == 256 and L.nvbio_hip_set_bwt_temp_bytes(0xFFFFFFFF, 1) == 256

    def sort(st=s, N=N, n=n, out=out, temp=temp, tb=big):
        return L.nvbio_hip_set_suffix_sort(C.byref(st) if st is not None else None, N, n, _p(out), None, None, _p(temp), tb, None)

    def bw(st=s, N=N, n=n, bwt=bwt, rows=rows, ids=ids, temp=temp, tb=big):
        return L.nvbio_hip_set_bwt(C.byref(st) if st is not None else None, N, n, _p(bwt), _p(rows), _p(ids), None, _p(temp), tb, None)

    def changed(**kw):
        t = _lib.StringSetStruct.from_buffer_copy(s)
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    for f in (sort, bw):
        assert f(st=None) == INVALID
        assert f(st=changed(words=None)) == INVALID
        assert f(st=changed(begin=None)) == INVALID
        assert f(st=changed(bits=4)) == INVALID
        assert f(N=0) == INVALID                                       # no strings
        assert f(N=n + 1) == INVALID                                   # more strings than slots
        assert f(n=0xFFFFFFFF) == INVALID and f(n=1 << 33) == INVALID
        assert f(temp=None) == INVALID
        assert f(st=changed(length=None, fixed_length=7)) == INVALID   # 2 * (7 + 1) slots are not n: known without the device
    assert sort(out=None) == INVALID and sort(tb=sort_tb - 1) == INVALID
    assert bw(bwt=None) == INVALID and bw(rows=None) == INVALID and bw(ids=None) == INVALID and bw(tb=bwt_tb - 1) == INVALID
    # the host twins check the same
    assert L.nvbio_hip_set_suffix_sort_host(None, N, n, _p(out), None, None, 1) == INVALID
    assert L.nvbio_hip_set_suffix_sort_host(C.byref(s), N, n, None, None, None, 1) == INVALID
    assert L.nvbio_hip_set_suffix_sort_host(C.byref(changed(bits=4)), N, n, _p(out), None, None, 1) == INVALID
    assert L.nvbio_hip_set_suffix_sort_host(C.byref(s), 0, n, _p(out), None, None, 1) == INVALID
    assert L.nvbio_hip_set_suffix_sort_host(C.byref(s), N, 0xFFFFFFFF, _p(out), None, None, 1) == INVALID
    assert L.nvbio_hip_set_suffix_sort_host(C.byref(s), 0xFFFFFFFC, 0xFFFFFFFE, _p(out), None, None, 1) == INVALID      # the twins' own limit on n_strings
    assert L.nvbio_hip_set_bwt_host(C.byref(s), 0xFFFFFFFC, 0xFFFFFFFE, _p(bwt), _p(rows), _p(ids), None, 1) == INVALID
    assert L.nvbio_hip_set_bwt_host(C.byref(s), N, n, None, _p(rows), _p(ids), None, 1) == INVALID
    assert L.nvbio_hip_set_bwt_host(C.byref(s), N, n, _p(bwt), None, _p(ids), None, 1) == INVALID
    assert L.nvbio_hip_set_bwt_host(C.byref(s), N, n, _p(bwt), _p(rows), None, None, 1) == INVALID
    assert L.nvbio_hip_set_bwt_host(C.byref(changed(words=None)), N, n, _p(bwt), _p(rows), _p(ids), None, 1) == INVALID


def test_python_layer_refuses_what_the_entries_cannot_take():
    import torch
    with pytest.raises(ValueError, match="at least one string"):
        nvbio_amd.set_suffix_sort([])
    with pytest.raises(ValueError, match="at least one string"):
        nvbio_amd.set_bwt([])
    four_bit = nvbio_amd.PackedStringSet(torch.zeros(4, dtype=torch.int32), 4, True, torch.zeros(1, dtype=torch.int64), torch.ones(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="2-bit"):
        nvbio_amd.set_suffix_sort(four_bit)
    with pytest.raises(ValueError, match="2-bit"):
        nvbio_amd.set_bwt(four_bit)
    # two strings said to hold 2^31 - 1 symbols each: 2^32 slots (the count comes from the lengths; nothing is read or allocated)
    huge = nvbio_amd.PackedStringSet(torch.zeros(4, dtype=torch.int32), 2, True, torch.zeros(2, dtype=torch.int64), None, 0x7FFFFFFF)
    with pytest.raises(ValueError, match="slots"):
        nvbio_amd.set_suffix_sort(huge)
    with pytest.raises(ValueError, match="slots"):
        nvbio_amd.set_bwt(huge)
