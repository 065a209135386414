"""The C++ host layer's WaveletTreeDevice and WaveletFMIndexDevice (include/nvbio_hip/wavelet.h, with suffix_sort_bytes / bwt_bytes of
sufsort.h underneath) through tests/cxx/wavelet_shim.cpp: byte for byte the reference arrays of tests/wavelet_reference.py and the
Python layer's answers."""
import ctypes as C
import os

import numpy as np
import pytest

import nvbio_amd as nvb
from tests import wavelet_cases as WC
from tests import wavelet_reference as R
from tests.wavelet_checks import u32, tree_expectation, fm_expectation, rank_queries

pytestmark = pytest.mark.gpu

SHIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx", "libwavelet_shim.so")


def _p(a):
    return C.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def shim():
    assert os.path.exists(SHIM), "build with python -c 'import __graft_entry__ as g; g.build()'"
    return C.CDLL(SHIM)


@pytest.mark.parametrize("case_id", ["s1_n33", "s5_n33", "s8_two_values", "s5_24values", "s8_n20011"])
def test_tree(shim, case_id):
    case, bits, splits, occ, counts = tree_expectation(case_id)
    n, S = case.text.size, case.S
    p, c = rank_queries(case)
    p, c = np.ascontiguousarray(p), np.ascontiguousarray(c)
    got = dict(bits=np.zeros_like(bits), splits=np.zeros_like(splits), occ=np.zeros_like(occ), text=np.zeros(n, dtype=np.uint8),
               rank=np.zeros(p.size, dtype=np.uint32), pairs=np.zeros(p.size & ~1, dtype=np.uint32))
    assert shim.wavelet_tree_host_layer(_p(case.text), S, C.c_uint64(n), _p(p), _p(c), C.c_uint64(p.size), _p(got["bits"]), _p(got["splits"]), _p(got["occ"]),
                                        _p(got["text"]), _p(got["rank"]), _p(got["pairs"])) == 0
    assert (got["bits"] == bits).all() and (got["splits"] == splits).all() and (got["occ"] == occ).all()
    assert (got["text"] == R.mask(case.text, S)).all()
    assert (got["rank"] == R.rank(counts, n, p, c, S)).all()
    m = p.size // 2
    assert (got["pairs"] == R.rank(counts, n, p[:2 * m], np.repeat(c[:m], 2), S)).all()
    tree = nvb.WaveletTree.build(case.text, S, device="cuda")
    assert (got["rank"] == u32(tree.rank(p, c))).all()


@pytest.mark.parametrize("case_id", ["protein24", "repeat13x400", "iid24_s5", "zero_runs"])
def test_fm_index(shim, case_id):
    case, sa, bwt, primary, L2, patterns, rows = fm_expectation(case_id)
    n, S, sa_int = case.text.size, case.S, 16
    psym = np.ascontiguousarray(np.concatenate(patterns)).astype(np.uint8)
    length = np.array([q.size for q in patterns], dtype=np.uint32)
    begin = (np.cumsum(length, dtype=np.uint64) - length).astype(np.uint64)
    fmi = nvb.WaveletFMIndex.build(case.text, S, sa_int, device="cuda")
    want_ranges = u32(fmi.match(patterns))
    found = want_ranges[:, 0] <= want_ranges[:, 1]
    srows = np.concatenate([np.arange(x, y + 1, dtype=np.uint32) for x, y in want_ranges[found]] + [np.array([0, n, n + 1], dtype=np.uint32)])[-5000:]
    srows = np.ascontiguousarray(srows)
    got_L2, got_primary = np.zeros_like(L2), C.c_uint32(0)
    got_ranges, got_pos = np.zeros_like(want_ranges), np.zeros(srows.size, dtype=np.uint32)
    assert shim.wavelet_fm_host_layer(_p(case.text), S, C.c_uint64(n), sa_int, _p(psym), C.c_uint64(psym.size), _p(begin), _p(length), C.c_uint64(length.size),
                                      _p(srows), C.c_uint64(srows.size), _p(got_L2), C.byref(got_primary), _p(got_ranges), _p(got_pos)) == 0
    assert (got_L2 == L2).all() and got_primary.value == primary
    assert (got_ranges == want_ranges).all()
    assert (got_pos == u32(fmi.locate(srows))).all()
    inside = (srows >= 1) & (srows <= n)
    assert (got_pos[inside] == sa[srows[inside]]).all()
