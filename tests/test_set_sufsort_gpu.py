"""The device string-set suffix sorter and BWT (the set entries of nvbio_amd/csrc/sufsort.hip through nvbio_amd.sufsort) against the
definition (tests/set_sufsort_reference.py) and against the host twins, byte for byte.  The order is total, so every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import nvbio_amd as nvb
from nvbio_amd import sufsort as SS
from tests import set_sufsort_reference as R
from tests import set_sufsort_sets as S
from tests import sufsort_texts as T
from tests import test_set_sufsort_host as H

pytestmark = pytest.mark.gpu

ALL = S.all_small()


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def dev_set(case, big_endian, dev):
    return nvb.PackedStringSet.from_host(case.words(big_endian), 2, big_endian, case.begin, case.length, case.fixed_length, device=dev)


def dev_sort(case, big_endian, dev):
    suffixes, ids, cum = nvb.set_suffix_sort(dev_set(case, big_endian, dev))
    return u32(suffixes), u32(ids), u32(cum)


def dev_bwt(case, big_endian, dev, keep=True):
    bwt, rows, ids, pairs = nvb.set_bwt(dev_set(case, big_endian, dev), keep_suffixes=keep)
    return bwt.cpu().numpy(), u32(rows), u32(ids), u32(pairs).reshape(-1) if keep else None


@pytest.mark.parametrize("big_endian", [True, False], ids=["be", "le"])
@pytest.mark.parametrize("case", ALL, ids=[c.id for c in ALL])
def test_device_equals_the_definition_and_the_host_twins(cuda, case, big_endian):
    e = R.expected(case)
    sort, bwt = dev_sort(case, big_endian, cuda), dev_bwt(case, big_endian, cuda)
    H.check_sort(sort, e)                               # rows 0 .. N - 1 = the empty suffixes in id order is part of it
    H.check_bwt(bwt, e)
    for got, twin in zip(sort + bwt, H.host_set_suffix_sort(case, big_endian) + H.host_set_bwt(case, big_endian)):
        assert got.tobytes() == twin.tobytes()


@pytest.mark.parametrize("text", [t for _, t in T.small_texts()], ids=[i for i, _ in T.small_texts()])
def test_one_string_is_the_plain_suffix_array(cuda, text):
    suffixes, _, _ = nvb.set_suffix_sort([torch.from_numpy(text).to(cuda)])
    assert torch.equal(suffixes, nvb.suffix_sort(torch.from_numpy(text).to(cuda)))


def test_medium_set_and_its_rounds(cuda):
    """duplicates of length 100 need orders of 29, 58 and 116 symbols: three rounds or more, the last leaving nothing"""
    case = S.medium_case()
    e = R.expected(case)
    H.check_sort(dev_sort(case, True, cuda), e)
    rounds = SS.last_rounds()
    assert len(rounds) >= 3 and rounds[-1] == 0 and all(r > 0 for r in rounds[:-1])
    got = dev_bwt(case, False, cuda)
    H.check_bwt(got, e)
    assert SS.last_rounds() == rounds
    assert nvb.lib().nvbio_hip_last_kernel() == b"sufsort_set_bwt_kernel"
    for a, b in zip(got, H.host_set_bwt(case, False, n_threads=0)):
        assert a.tobytes() == b.tobytes()


def test_short_strings_take_one_round(cuda):
    case = S.short_iid_case()
    H.check_sort(dev_sort(case, True, cuda), R.expected(case))
    assert SS.last_rounds() == [0]


def test_lists_of_symbol_arrays_are_packed_first(cuda):
    case = dict((c.id, c) for c in ALL)["prefixes_and_suffixes"]
    e = R.expected(case)
    suffixes, ids, cum = nvb.set_suffix_sort([torch.from_numpy(t).to(cuda) for t in case.strings])
    H.check_sort((u32(suffixes), u32(ids), u32(cum)), e)
    bwt, rows, dids, none = nvb.set_bwt(case.strings)                   # host arrays go to the default device
    assert none is None
    H.check_bwt((bwt.cpu().numpy(), u32(rows), u32(dids), None), e)


class Raw:
    """the C-ABI called directly on one case"""

    def __init__(self, case, dev, big_endian=True):
        self.L = nvb.lib()
        self.set = dev_set(case, big_endian, dev)
        self.struct = self.set.struct()
        self.n, self.N, self.dev = case.n_suffixes, case.n_strings, dev
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def zeros(self, count, dtype=torch.int32):
        return torch.zeros(count, dtype=dtype, device=self.dev)

    def sort(self, out, ids, cum, temp, tb, n=None):
        vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        return self.L.nvbio_hip_set_suffix_sort(C.byref(self.struct), self.N, self.n if n is None else n, vp(out), vp(ids), vp(cum), vp(temp), tb, self.stream)

    def bwt(self, out, rows, ids, pairs, temp, tb, n=None):
        vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        return self.L.nvbio_hip_set_bwt(C.byref(self.struct), self.N, self.n if n is None else n, vp(out), vp(rows), vp(ids), vp(pairs), vp(temp), tb, self.stream)


def test_refusals_leave_the_outputs_untouched_and_temp_can_be_reused(cuda):
    case = dict((c.id, c) for c in ALL)["overlapping"]
    e = R.expected(case)
    r = Raw(case, cuda)
    n, N = r.n, r.N
    tb = int(r.L.nvbio_hip_set_suffix_sort_temp_bytes(n + 1, N))        # room for the call that says one slot too many
    temp = torch.empty(tb, dtype=torch.uint8, device=cuda)
    out, ids, cum = r.zeros(n + 1), r.zeros(n + 1), r.zeros(N)
    exact = int(r.L.nvbio_hip_set_suffix_sort_temp_bytes(n, N))
    assert r.sort(out, ids, cum, temp, exact - 1) == 1                  # temp one byte short
    assert r.sort(out, ids, cum, temp, tb, n=n + 1) == 1                # one slot too many
    assert r.sort(out, ids, cum, temp, tb, n=n - 1) == 1                # one too few
    assert r.sort(out, ids, cum, temp, tb, n=N) == 1                    # as if every string were empty: most first slots lie past it
    assert not bool(out.any()) and not bool(ids.any()) and not bool(cum.any())
    assert r.sort(out, ids, cum, temp, tb) == 0
    out2 = r.zeros(n)
    assert r.sort(out2, None, None, temp, tb) == 0                      # the same scratch as the first call left it; optional outputs NULL
    assert torch.equal(out[:n], out2)
    H.check_sort((u32(out[:n]), u32(ids[:n]), u32(cum)), e)

    tb = int(r.L.nvbio_hip_set_bwt_temp_bytes(n + 1, N))
    temp = torch.empty(tb, dtype=torch.uint8, device=cuda)
    exact = int(r.L.nvbio_hip_set_bwt_temp_bytes(n, N))
    bwt, rows, dids, pairs = r.zeros(n + 1, torch.uint8), r.zeros(N), r.zeros(N), r.zeros(2 * n + 2)
    assert r.bwt(bwt, rows, dids, pairs, temp, exact - 1) == 1
    assert r.bwt(bwt, rows, dids, pairs, temp, tb, n=n + 1) == 1
    assert r.bwt(bwt, rows, dids, pairs, temp, tb, n=n - 1) == 1
    assert r.bwt(bwt, rows, dids, pairs, temp, tb, n=N) == 1
    assert not bool(bwt.any()) and not bool(rows.any()) and not bool(dids.any()) and not bool(pairs.any())
    assert r.bwt(bwt, rows, dids, pairs, temp, tb) == 0
    H.check_bwt((bwt[:n].cpu().numpy(), u32(rows), u32(dids), u32(pairs[:2 * n])), e)
    assert not bool(bwt[n:].any()) and not bool(pairs[2 * n:].any())   # nothing past the last row
    bwt2, rows2, dids2 = r.zeros(n, torch.uint8), r.zeros(N), r.zeros(N)
    assert r.bwt(bwt2, rows2, dids2, None, temp, tb) == 0               # the scratch again, without the pairs
    assert torch.equal(bwt[:n], bwt2) and torch.equal(rows, rows2) and torch.equal(dids, dids2)


def test_bwt_into_an_unaligned_buffer(cuda):
    """bwt_out one byte into a word: the kernel's word stores give way to byte stores, and nothing outside [0, n) is written"""
    case = dict((c.id, c) for c in ALL)["out_of_stream_order"]
    e = R.expected(case)
    r = Raw(case, cuda)
    n, N = r.n, r.N
    tb = int(r.L.nvbio_hip_set_bwt_temp_bytes(n, N))
    temp = torch.empty(tb, dtype=torch.uint8, device=cuda)
    buf = torch.full((n + 8,), 0xEE, dtype=torch.uint8, device=cuda)
    rows, dids = r.zeros(N), r.zeros(N)
    assert r.bwt(buf[1:], rows, dids, None, temp, tb) == 0
    got = buf.cpu().numpy()
    assert got[0] == 0xEE and (got[1 + n:] == 0xEE).all() and (got[1:1 + n] == e.bwt).all()


@pytest.mark.parametrize("big_endian", [True, False], ids=["be", "le"])
def test_cxx_host_layer(cuda, big_endian):
    """nvbio::hip::set_suffix_sort / set_bwt of include/nvbio_hip/sufsort.h (tests/cxx/set_sufsort_shim.cpp) return the same results"""
    shim = C.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx", "libset_sufsort_shim.so"))
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    for name in ("overlapping", "fixed29", "same100x3"):
        case = dict((c.id, c) for c in ALL)[name]
        e = R.expected(case)
        n, N = case.n_suffixes, case.n_strings
        words = case.words(big_endian)
        suffixes, ids, cum = np.empty(n, np.uint32), np.empty(n, np.uint32), np.empty(N, np.uint32)
        bwt, rows, dids, pairs = np.empty(n, np.uint8), np.empty(N, np.uint32), np.empty(N, np.uint32), np.empty(2 * n, np.uint32)
        assert shim.set_sufsort_host_layer(p(words), C.c_uint64(words.size), int(big_endian), p(case.begin), p(case.length), case.fixed_length, N,
                                           p(suffixes), p(ids), p(cum), p(bwt), p(rows), p(dids), p(pairs)) == 0
        H.check_sort((suffixes, ids, cum), e)
        H.check_bwt((bwt, rows, dids, pairs), e)
