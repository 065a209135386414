"""The drop-in wavelet tree (compat/nvbio/strings/wavelet_tree.h, basic/packed_vector.h, strings/alphabet.h, the plain-string sorter on
wide alphabets) through tests/compat/wavelet_callers.hip, and the C++ host layer through tests/cxx/wavelet_shim.cpp: each byte for byte
the reference arrays of tests/wavelet_reference.py and the Python layer's answers."""
import ctypes as C
import os

import numpy as np
import pytest

import nvbio_amd as nvb
from tests import wavelet_cases as WC
from tests import wavelet_reference as R
from tests.wavelet_checks import u32, u8, tree_expectation, rank_queries

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CALLERS = os.path.join(HERE, "compat", "libwavelet_callers.so")
SHIM = os.path.join(HERE, "cxx", "libwavelet_shim.so")


def _p(a):
    return C.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def callers():
    assert os.path.exists(CALLERS), "build with python -c 'import __graft_entry__ as g; g.build()'"
    return C.CDLL(CALLERS)


def _queries(case):
    p, c = rank_queries(case)
    return np.ascontiguousarray(p), np.ascontiguousarray(c)


@pytest.mark.parametrize("case_id", ["s8_n64", "s8_two_values", "known_ranks", "s8_n20011"])
def test_abi_path_from_device_bytes(callers, case_id):
    case, bits, splits, occ, counts = tree_expectation(case_id)
    n = case.text.size
    p, c = _queries(case)
    got = dict(bits=np.zeros_like(bits), splits=np.zeros_like(splits), occ=np.zeros_like(occ), text=np.zeros(n, dtype=np.uint8), rank=np.zeros(p.size, dtype=np.uint32))
    path = C.create_string_buffer(32)
    assert callers.compat_wavelet_bytes(_p(case.text), n, _p(p), _p(c), p.size, _p(got["bits"]), _p(got["splits"]), _p(got["occ"]), _p(got["text"]), _p(got["rank"]), path) == 0
    assert path.value == b"bytes"
    assert (got["bits"] == bits).all() and (got["splits"] == splits).all() and (got["occ"] == occ).all()
    assert (got["text"] == case.text).all()
    assert (got["rank"] == R.rank(counts, n, p, c, 8)).all()
    tree = nvb.WaveletTree.build(case.text, 8, device="cuda")
    assert (got["bits"] == u32(tree.bits)).all() and (got["occ"] == u32(tree.occ)).all() and (got["rank"] == u32(tree.rank(p, c))).all()


@pytest.mark.parametrize("case_id", ["s5_n33", "s5_24values", "s5_high_bits"])
def test_generic_path_from_a_5bit_packed_vector_and_a_host_tree(callers, case_id):
    case, bits, splits, occ, counts = tree_expectation(case_id)
    n = case.text.size
    masked = R.mask(case.text, 5)               # a 5-bit vector holds the masked symbols
    p, c = _queries(case)
    dev = dict(bits=np.zeros_like(bits), splits=np.zeros_like(splits), occ=np.zeros_like(occ), text=np.zeros(n, dtype=np.uint8), rank=np.zeros(p.size, dtype=np.uint32))
    host = dict(bits=np.zeros_like(bits), splits=np.zeros_like(splits), occ=np.zeros_like(occ), text=np.zeros(n, dtype=np.uint8), rank=np.zeros(p.size, dtype=np.uint32),
                range=np.zeros(p.size, dtype=np.uint32))
    path = C.create_string_buffer(32)
    assert callers.compat_wavelet_packed5(_p(masked), n, _p(p), _p(c), p.size, _p(dev["bits"]), _p(dev["splits"]), _p(dev["occ"]), _p(dev["text"]), _p(dev["rank"]), path,
                                          _p(host["bits"]), _p(host["splits"]), _p(host["occ"]), _p(host["text"]), _p(host["rank"]), _p(host["range"])) == 0
    assert path.value == b"unpacked"
    want_rank = R.rank(counts, n, p, c, 5)
    for got in (dev, host):
        assert (got["bits"] == bits).all() and (got["splits"] == splits).all() and (got["occ"] == occ).all()
        assert (got["text"] == masked).all()
        assert (got["rank"] == want_rank).all()
    m = p.size & ~1
    assert (host["range"][:m] == R.rank(counts, n, p[:m], np.repeat(c[0:m:2], 2), 5)).all()
    tree = nvb.WaveletTree.build(case.text, 5, device="cuda")
    assert (dev["rank"] == u32(tree.rank(p, c))).all() and (dev["text"] == u8(tree.text())).all()


@pytest.mark.parametrize("case_id", ["protein24", "repeat13x400", "iid256", "zero_runs"])
def test_plain_string_sorter_on_an_8bit_packed_vector(callers, case_id):
    case = {c.id: c for c in WC.fm_cases()}[case_id]
    n = case.text.size
    sa, bwt = np.zeros(n + 1, dtype=np.uint32), np.zeros(n, dtype=np.uint8)
    primary, found = C.c_uint32(0), C.c_uint32(0)
    assert callers.compat_wavelet_bwt8(_p(case.text), n, _p(sa), _p(bwt), C.byref(primary), C.byref(found)) == 0
    want_bwt, want_primary, _, want_sa = nvb.bwt_bytes(case.text, 8, 16, keep_sa=True, device="cuda")
    assert (sa == u32(want_sa)).all() and (bwt == u8(want_bwt)).all() and primary.value == want_primary == found.value
    assert (sa == R.suffix_array(case.text, 8)).all()


def test_fm_index_over_the_tree_as_the_reference_example_builds_it(callers):
    text = WC.PROTEIN_TEXT.encode()
    n = len(text)
    out_bwt = C.create_string_buffer(n + 2)
    primary = C.c_uint32(0)
    ranges = np.zeros((n, 2), dtype=np.uint32)
    assert callers.compat_wavelet_fm(text, n, out_bwt, C.byref(primary), _p(ranges)) == 0
    sym = nvb.alphabet.encode(WC.PROTEIN_TEXT)
    sa = R.suffix_array(sym, 8)
    bwt, want_primary = R.bwt(sym, 8, sa)
    assert out_bwt.value.decode() == nvb.alphabet.decode(bwt) and primary.value == want_primary
    fmi = nvb.WaveletFMIndex.build(sym, 8, 4, device="cuda")
    assert (ranges == u32(fmi.match([sym[i:] for i in range(n)]))).all()
    assert (ranges[:, 0] == ranges[:, 1]).all()


def test_host_layer_shim_is_built():
    """the C++ host layer's classes are driven by tests/test_wavelet_shim_gpu.py; here only that build() made the shim"""
    assert os.path.exists(SHIM), "build with python -c 'import __graft_entry__ as g; g.build()'"
