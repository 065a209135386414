"""The temp contract of the two device rank entries, nvbio_hip_fm_mem_rank and nvbio_hip_fm_mem_rank_split: what the size queries
answer is exactly what the entries need.  The helpers are those of tests/test_mem_split_gpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import nvbio_amd as nvb
from nvbio_amd import _lib
from oracle import pyoracle as O
from tests import mem_reference as M
from tests import test_mem_host as H
from tests import test_mem_split_host as HS
from tests.test_mem_split_gpu import device_indices, device_set

pytestmark = pytest.mark.gpu


def test_both_rank_entries_take_exactly_their_temp_bytes_and_refuse_one_byte_less(cuda):
    """the 77-symbol text's patterns, (1, NO_MAX, 1) and split (8, 3): each entry, given a temp of exactly what its size query answers,
    gives the host twin's table and stays inside it; told of one byte less it returns 1 and has written nothing"""
    L = nvb.lib()
    t, f, r = M.indices_of(77)
    df, dr = device_indices(77, cuda)
    hs = O.StringSet.from_lists(M.patterns_of(77), 4, True)
    ds, n, max_len, symbols = device_set(hs, cuda), len(hs), int(hs.length.max()), int(hs.length.sum())
    params, split = (1, M.NO_MAX, 1), (8, 3)
    fs, rs, ss = df.struct(), dr.struct(), ds.struct()
    cases = ((L.nvbio_hip_fm_mem_rank, (), symbols, int(L.nvbio_hip_fm_mem_temp_bytes(n, max_len)), H.host_rank(f, r, hs, params)),
             (L.nvbio_hip_fm_mem_rank_split, split, 16 * symbols, int(L.nvbio_hip_fm_mem_split_temp_bytes(n, max_len, 16 * symbols)),
              HS.host_rank_split(f, r, hs, params, split)))
    for entry, extra, cap, tb, want in cases:
        k = want[4]
        assert want[0] == 0 and 0 < k <= cap and tb > 256
        for given in (tb - 1, tb):
            temp = torch.full((tb + 256,), 0xA5, dtype=torch.uint8, device=cuda)
            ranges = torch.full((cap, 4), -1, dtype=torch.int32, device=cuda)
            slots = torch.full((cap,), -1, dtype=torch.int64, device=cuda)
            index = torch.full((n + 1,), -1, dtype=torch.int64, device=cuda)
            found = C.c_uint64(7)
            err = entry(C.byref(fs), C.byref(rs), C.byref(ss), n, max_len, *params, *extra, C.c_void_p(ranges.data_ptr()), cap, C.c_void_p(index.data_ptr()),
                        C.c_void_p(slots.data_ptr()), C.byref(found), C.c_void_p(temp.data_ptr()), given, _lib.current_stream_ptr())
            torch.cuda.synchronize()
            assert bool((temp[tb:] == 0xA5).all()), (entry.__name__, given)                        # nothing past the temp, whatever happened
            if given < tb:
                assert err == 1 and found.value == 0
                assert bool((temp == 0xA5).all()) and bool((ranges == -1).all()) and bool((slots == -1).all()) and bool((index == -1).all())
            else:
                assert err == 0 and found.value == k
                assert (ranges[:k].cpu().numpy().view(np.uint32) == want[1]).all() and bool((ranges[k:] == -1).all())
                assert (slots[:k].cpu().numpy().view(np.uint64) == want[3]).all() and bool((slots[k:] == -1).all())
                assert (index.cpu().numpy().view(np.uint64) == want[2]).all()
