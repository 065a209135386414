"""The device suffix sorter and BWT builder (nvbio_amd/csrc/sufsort.hip through nvbio_amd.sufsort) against the CPU oracle: the suffix
array equals oracle.pyoracle.suffix_array, and build_fm_index equals oracle.pyoracle.FMIndex field for field.  The suffix array of a
text is unique, so every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import nvbio_amd as nvb
from nvbio_amd import sufsort as S
from nvbio_amd import workloads as W
from oracle import pyoracle as O
from tests import sufsort_texts as T
from tests import test_sufsort_host as H

pytestmark = pytest.mark.gpu

ALL = T.small_texts() + T.structured_texts()


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def dev_words(text, big_endian, dev):
    return torch.from_numpy(T.pack(text, big_endian).view(np.int32)).to(dev)


def check_index(fmi, sa, host):
    assert fmi.length == host.length and fmi.primary == host.primary and fmi.L2 == [int(x) for x in host.L2]
    assert fmi.sa_int == host.sa_int
    assert (sa.cpu().numpy().astype(np.uint32) == host.sa).all()
    assert (u32(fmi.bwt_occ) == host.bwt_occ[: fmi.bwt_occ.numel()]).all()
    assert (u32(fmi.ssa) == host.ssa).all()


@pytest.mark.parametrize("big_endian", [True, False], ids=["be", "le"])
@pytest.mark.parametrize("text", [t for _, t in ALL], ids=[i for i, _ in ALL])
def test_suffix_array_equals_oracle(cuda, text, big_endian):
    sa = nvb.suffix_sort((dev_words(text, big_endian, cuda), len(text), big_endian))
    assert (u32(sa) == O.suffix_array(text)).all()


@pytest.mark.parametrize("text", [t for _, t in ALL], ids=[i for i, _ in ALL])
def test_built_index_equals_oracle(cuda, text):
    fmi, sa = nvb.build_fm_index(torch.from_numpy(text).to(cuda), keep_sa=True)
    check_index(fmi, sa, O.FMIndex(text))


def test_repetitive_texts_take_several_rounds(cuda):
    """all-A of 4 097 symbols is one group after round 0 that loses h suffixes a round: eight or more rounds, each smaller than the last"""
    nvb.suffix_sort(torch.zeros(4097, dtype=torch.uint8, device=cuda))
    rounds = S.last_rounds()
    assert len(rounds) >= 8 and rounds[-1] == 0
    assert all(a > b for a, b in zip(rounds, rounds[1:]))
    nvb.suffix_sort(torch.from_numpy(dict(T.structured_texts())["iid8191"]).to(cuda))
    assert S.last_rounds() == [0]


def test_big_text_equals_oracle_and_the_torch_builder(cuda):
    text = T.big_text()
    host = O.FMIndex(text)
    d_text = torch.from_numpy(text).to(cuda)
    fmi, sa = nvb.build_fm_index(d_text, keep_sa=True)
    check_index(fmi, sa, host)
    old, old_sa = W.build_fm_index(d_text, keep_sa=True)
    assert (fmi.length, fmi.primary, fmi.L2, fmi.sa_int) == (old.length, old.primary, old.L2, old.sa_int)
    assert torch.equal(sa, old_sa) and torch.equal(fmi.bwt_occ, old.bwt_occ) and torch.equal(fmi.ssa, old.ssa)
    seeds = W.make_seeds(d_text, 20000, 22)
    assert (u32(nvb.match(fmi, seeds)) == host.match(O.StringSet.from_device(seeds))).all()


def test_primary_at_its_extremes(cuda):
    texts = dict(T.structured_texts())
    lo, hi = texts["primary_first"], texts["primary_last"]
    assert nvb.bwt(torch.from_numpy(lo).to(cuda))[1] == 1 == O.FMIndex(lo).primary
    assert nvb.bwt(torch.from_numpy(hi).to(cuda))[1] == len(hi) == O.FMIndex(hi).primary


@pytest.mark.parametrize("sa_int", [1, 4, 16, 64])
def test_sampling_interval_and_optional_outputs(cuda, sa_int):
    text = dict(T.structured_texts())["unit301x17"]
    host = O.FMIndex(text, sa_int=sa_int)
    d_text = torch.from_numpy(text).to(cuda)
    fmi, sa = nvb.build_fm_index(d_text, sa_int=sa_int, keep_sa=True)
    check_index(fmi, sa, host)
    assert nvb.build_fm_index(d_text, sa_int=sa_int).primary == host.primary           # keep_sa=False: sa_out == NULL
    words, primary, ssa, sa_none = nvb.bwt(d_text, sa_int=sa_int, want_ssa=False)       # ssa_out == NULL
    assert ssa is None and sa_none is None and primary == host.primary
    assert (u32(words) == H.expected_bwt_words(host)).all()


@pytest.mark.parametrize("name", ["iid33", "allT65", "allA4097", "unit301x17", "fib5779"])
def test_host_twin_returns_the_same_bytes(cuda, name):
    text = dict(ALL)[name]
    for be in (True, False):
        words, primary, ssa, sa = nvb.bwt((dev_words(text, be, cuda), len(text), be), sa_int=4, keep_sa=True)
        h_words, h_primary, h_ssa, h_sa = H.host_bwt(text, sa_int=4, big_endian=be)
        assert primary == h_primary
        assert u32(words).tobytes() == h_words.tobytes() and u32(ssa).tobytes() == h_ssa.tobytes() and u32(sa).tobytes() == h_sa.tobytes()
        assert u32(nvb.suffix_sort((dev_words(text, be, cuda), len(text), be))).tobytes() == H.host_suffix_sort(text, be).tobytes()


def test_temp_one_byte_short_is_refused_and_temp_can_be_reused(cuda):
    text = dict(ALL)["unit301x17"]
    n = len(text)
    L = nvb.lib()
    words = dev_words(text, True, cuda)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda t: C.c_void_p(t.data_ptr())
    tb = int(L.nvbio_hip_suffix_sort_temp_bytes(n))
    temp = torch.empty(tb, dtype=torch.uint8, device=cuda)
    sa1 = torch.zeros(n + 1, dtype=torch.int32, device=cuda)
    sa2 = torch.zeros(n + 1, dtype=torch.int32, device=cuda)
    assert L.nvbio_hip_suffix_sort(vp(words), 2, 1, n, vp(sa1), vp(temp), tb - 1, stream) == 1
    assert not bool(sa1.any())                                                       # refused: nothing was launched
    assert L.nvbio_hip_suffix_sort(vp(words), 2, 1, n, vp(sa1), vp(temp), tb, stream) == 0
    assert L.nvbio_hip_suffix_sort(vp(words), 2, 1, n, vp(sa2), vp(temp), tb, stream) == 0       # the same scratch, as the first call left it
    assert torch.equal(sa1, sa2) and (u32(sa1) == O.suffix_array(text)).all()
    tb = int(L.nvbio_hip_bwt_temp_bytes(n))
    temp = torch.empty(tb, dtype=torch.uint8, device=cuda)
    primary = C.c_uint32(0)
    outs = [torch.zeros(4 * ((n + 63) // 64), dtype=torch.int32, device=cuda) for _ in range(2)]
    assert L.nvbio_hip_bwt(vp(words), 2, 1, n, 16, vp(outs[0]), C.byref(primary), None, None, vp(temp), tb - 1, stream) == 1
    assert not bool(outs[0].any())
    for o in outs:
        assert L.nvbio_hip_bwt(vp(words), 2, 1, n, 16, vp(o), C.byref(primary), None, None, vp(temp), tb, stream) == 0
    assert torch.equal(outs[0], outs[1]) and primary.value == O.FMIndex(text).primary
    assert nvb.lib().nvbio_hip_last_kernel() == b"sufsort_bwt_kernel"


@pytest.mark.parametrize("big_endian", [True, False], ids=["be", "le"])
def test_cxx_host_layer(cuda, big_endian):
    """nvbio::hip::suffix_sort / bwt of include/nvbio_hip/sufsort.h (tests/cxx/sufsort_shim.cpp) return the oracle's index"""
    import os
    shim = C.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx", "libsufsort_shim.so"))
    text = dict(ALL)["unit301x17"]
    n, sa_int = len(text), 4
    host = O.FMIndex(text, sa_int=sa_int)
    words = T.pack(text, big_endian)
    sa = np.empty(n + 1, dtype=np.uint32)
    bwt_words = np.empty(4 * ((n + 63) // 64), dtype=np.uint32)
    ssa = np.empty((n + sa_int) // sa_int, dtype=np.uint32)
    primary = C.c_uint32(0)
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert shim.sufsort_host_layer(p(words), int(big_endian), C.c_uint64(n), sa_int, p(sa), p(bwt_words), C.byref(primary), p(ssa)) == 0
    assert (sa == host.sa).all() and primary.value == host.primary and (ssa == host.ssa).all()
    assert (bwt_words == H.expected_bwt_words(host)).all()
