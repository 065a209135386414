"""The `_host` twins of the suffix-sort entries against the CPU oracle, and the argument checks of the device entries (no GPU needed).

Convention (compat/nvbio/fmindex/bwt.h, oracle.pyoracle.suffix_array): SA has n + 1 rows, SA[0] = n, a suffix that is a proper prefix
of another sorts first; the BWT drops the '$' row; ssa[k] = SA[k * sa_int] with ssa[0] = 0xFFFFFFFF."""
import ctypes as C

import numpy as np
import pytest

import nvbio_amd
from oracle import pyoracle as O
from tests import sufsort_texts as T

INVALID = 1      # hipErrorInvalidValue


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def host_suffix_sort(text, big_endian=True, n_threads=2):
    words = T.pack(text, big_endian)
    sa = np.empty(len(text) + 1, dtype=np.uint32)
    err = nvbio_amd.lib().nvbio_hip_suffix_sort_host(_p(words), 2, int(big_endian), len(text), _p(sa), n_threads)
    assert err == 0
    return sa


def host_bwt(text, sa_int=16, big_endian=True, want_ssa=True, want_sa=True, n_threads=2):
    n = len(text)
    words = T.pack(text, big_endian)
    out = np.full(4 * ((n + 63) // 64), 0xDEADBEEF, dtype=np.uint32)
    ssa = np.empty((n + sa_int) // sa_int, dtype=np.uint32) if want_ssa else None
    sa = np.empty(n + 1, dtype=np.uint32) if want_sa else None
    primary = C.c_uint32(0)
    err = nvbio_amd.lib().nvbio_hip_bwt_host(_p(words), 2, int(big_endian), n, sa_int, _p(out), C.byref(primary), _p(ssa), _p(sa), n_threads)
    assert err == 0
    return out, int(primary.value), ssa, sa


def expected_bwt_words(host_index):
    n = host_index.length
    w = np.zeros(4 * ((n + 63) // 64), dtype=np.uint32)
    pw = T.pack(host_index.bwt, True)
    w[:pw.size] = pw
    return w


ALL = T.small_texts() + T.structured_texts()


@pytest.mark.parametrize("big_endian", [True, False], ids=["be", "le"])
@pytest.mark.parametrize("text", [t for _, t in ALL], ids=[i for i, _ in ALL])
def test_host_suffix_sort_equals_oracle(text, big_endian):
    assert (host_suffix_sort(text, big_endian) == O.suffix_array(text)).all()


@pytest.mark.parametrize("text", [t for _, t in ALL], ids=[i for i, _ in ALL])
def test_host_bwt_equals_oracle(text):
    host = O.FMIndex(text, sa_int=4)
    words, primary, ssa, sa = host_bwt(text, sa_int=4, big_endian=False)
    assert primary == host.primary
    assert (sa == host.sa).all()
    assert (ssa == host.ssa).all()
    assert (words == expected_bwt_words(host)).all()


def test_primary_at_its_extremes():
    texts = dict(T.structured_texts())
    assert host_bwt(texts["primary_first"])[1] == 1
    assert host_bwt(texts["primary_last"])[1] == len(texts["primary_last"])


@pytest.mark.parametrize("sa_int", [1, 4, 16, 64])
def test_host_bwt_sampling_and_optional_outputs(sa_int):
    text = dict(T.structured_texts())["unit301x17"]
    host = O.FMIndex(text, sa_int=sa_int)
    words, primary, ssa, sa = host_bwt(text, sa_int=sa_int)
    assert (ssa == host.ssa).all() and primary == host.primary
    words2, primary2, none_ssa, none_sa = host_bwt(text, sa_int=sa_int, want_ssa=False, want_sa=False)
    assert none_ssa is None and none_sa is None and primary2 == primary and (words2 == words).all()


def test_invalid_arguments_are_rejected_without_a_gpu():
    L = nvbio_amd.lib()
    n = 100
    words = T.pack(np.zeros(n, dtype=np.uint8), True)
    sa = np.zeros(n + 1, dtype=np.uint32)
    out = np.zeros(8, dtype=np.uint32)
    primary = C.c_uint32(0)
    temp = np.zeros(16, dtype=np.uint8)            # a non-null pointer; every call below is refused before anything touches it
    big = 1 << 40
    assert L.nvbio_hip_suffix_sort_temp_bytes(n) >= 36 * n and L.nvbio_hip_bwt_temp_bytes(n) >= L.nvbio_hip_suffix_sort_temp_bytes(n) + 4 * (n + 1)
    # device entries: null pointers, bits != 2, n == 0, n above the maximum, too little temp
    assert L.nvbio_hip_suffix_sort(None, 2, 1, n, _p(sa), _p(temp), big, None) == INVALID
    assert L.nvbio_hip_suffix_sort(_p(words), 2, 1, n, None, _p(temp), big, None) == INVALID
    assert L.nvbio_hip_suffix_sort(_p(words), 2, 1, n, _p(sa), None, big, None) == INVALID
    assert L.nvbio_hip_suffix_sort(_p(words), 4, 1, n, _p(sa), _p(temp), big, None) == INVALID
    assert L.nvbio_hip_suffix_sort(_p(words), 2, 1, 0, _p(sa), _p(temp), big, None) == INVALID
    assert L.nvbio_hip_suffix_sort(_p(words), 2, 1, 0xFFFFFFFF, _p(sa), _p(temp), big, None) == INVALID
    assert L.nvbio_hip_suffix_sort(_p(words), 2, 1, 1 << 33, _p(sa), _p(temp), big, None) == INVALID
    assert L.nvbio_hip_suffix_sort(_p(words), 2, 1, n, _p(sa), _p(temp), L.nvbio_hip_suffix_sort_temp_bytes(n) - 1, None) == INVALID
    assert L.nvbio_hip_bwt(None, 2, 1, n, 16, _p(out), C.byref(primary), None, None, _p(temp), big, None) == INVALID
    assert L.nvbio_hip_bwt(_p(words), 2, 1, n, 16, None, C.byref(primary), None, None, _p(temp), big, None) == INVALID
    assert L.nvbio_hip_bwt(_p(words), 2, 1, n, 16, _p(out), None, None, None, _p(temp), big, None) == INVALID
    assert L.nvbio_hip_bwt(_p(words), 2, 1, n, 16, _p(out), C.byref(primary), None, None, None, big, None) == INVALID
    assert L.nvbio_hip_bwt(_p(words), 8, 1, n, 16, _p(out), C.byref(primary), None, None, _p(temp), big, None) == INVALID
    assert L.nvbio_hip_bwt(_p(words), 2, 1, 0, 16, _p(out), C.byref(primary), None, None, _p(temp), big, None) == INVALID
    assert L.nvbio_hip_bwt(_p(words), 2, 1, 0xFFFFFFFF, 16, _p(out), C.byref(primary), None, None, _p(temp), big, None) == INVALID
    assert L.nvbio_hip_bwt(_p(words), 2, 1, n, 0, _p(out), C.byref(primary), _p(sa), None, _p(temp), big, None) == INVALID       # an SSA every 0 rows
    assert L.nvbio_hip_bwt(_p(words), 2, 1, n, 16, _p(out), C.byref(primary), None, None, _p(temp), L.nvbio_hip_bwt_temp_bytes(n) - 1, None) == INVALID
    # the host twins check the same
    assert L.nvbio_hip_suffix_sort_host(None, 2, 1, n, _p(sa), 1) == INVALID
    assert L.nvbio_hip_suffix_sort_host(_p(words), 2, 1, n, None, 1) == INVALID
    assert L.nvbio_hip_suffix_sort_host(_p(words), 4, 1, n, _p(sa), 1) == INVALID
    assert L.nvbio_hip_suffix_sort_host(_p(words), 2, 1, 0, _p(sa), 1) == INVALID
    assert L.nvbio_hip_suffix_sort_host(_p(words), 2, 1, 0xFFFFFFFF, _p(sa), 1) == INVALID
    assert L.nvbio_hip_bwt_host(_p(words), 2, 1, n, 16, None, C.byref(primary), None, None, 1) == INVALID
    assert L.nvbio_hip_bwt_host(_p(words), 2, 1, n, 16, _p(out), None, None, None, 1) == INVALID
    assert L.nvbio_hip_bwt_host(_p(words), 3, 1, n, 16, _p(out), C.byref(primary), None, None, 1) == INVALID


def test_python_layer_refuses_an_empty_text():
    import torch
    with pytest.raises(ValueError):
        nvbio_amd.suffix_sort(torch.zeros(0, dtype=torch.uint8))
