"""MEM re-seeding on the GPU: nvbio_hip_fm_mem_rank_split and the layers above it (nvbio_amd.MEMFilter, the C++ host class, the
drop-in filters) against the host twin and model (a) of tests/mem_split_reference.py, on the grid of tests/test_mem_split_host.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import nvbio_amd as nvb
from nvbio_amd import _lib
from oracle import pyoracle as O
from tests import mem_reference as M
from tests import mem_split_reference as S
from tests import test_mem_host as H
from tests import test_mem_split_host as HS

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_dev = {}


def device_indices(n_text, cuda):
    if n_text not in _dev:
        t, f, r = M.indices_of(n_text)
        _dev[n_text] = (nvb.FMIndexDevice.from_host(f, cuda), nvb.FMIndexDevice.from_host(r, cuda))
    return _dev[n_text]


def device_set(hs, cuda, fixed_length=0):
    return nvb.PackedStringSet.from_host(hs.words, hs.bits, hs.big_endian, hs.begin, None if fixed_length else hs.length, fixed_length, device=cuda)


def device_rank_split(df, dr, ds, params, split, capacity, max_len):
    """the ABI entry itself -> (error, ranges [k, 4], index [n + 1], slots [k], number reported), as numpy; k = the records stored"""
    L = nvb.lib()
    n = len(ds)
    dev = ds.words.device
    tb = int(L.nvbio_hip_fm_mem_split_temp_bytes(n, max_len, capacity))
    temp = torch.empty(tb, dtype=torch.uint8, device=dev)
    ranges = torch.full((capacity + 1, 4), -1, dtype=torch.int32, device=dev)
    slots = torch.full((capacity + 1,), -1, dtype=torch.int64, device=dev)
    index = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    found = C.c_uint64(0)
    fs, rs, ss = df.struct(), dr.struct(), ds.struct()
    err = L.nvbio_hip_fm_mem_rank_split(C.byref(fs), C.byref(rs), C.byref(ss), n, max_len, params[0], params[1], params[2], split[0], split[1],
                                        C.c_void_p(ranges.data_ptr()), capacity, C.c_void_p(index.data_ptr()), C.c_void_p(slots.data_ptr()), C.byref(found),
                                        C.c_void_p(temp.data_ptr()), tb, _lib.current_stream_ptr())
    torch.cuda.synchronize()
    k = min(int(found.value), capacity)
    assert bool((ranges[capacity:] == -1).all()) and bool((slots[capacity:] == -1).all())          # nothing past the capacity, whatever happened
    if err == 0:
        assert bool((ranges[k:] == -1).all()) and bool((slots[k:] == -1).all())                    # nor past what was stored
    elif split[0] != M.NO_MAX:
        k = 0
    return err, ranges[:k].cpu().numpy().view(np.uint32), index.cpu().numpy().view(np.uint64), slots[:k].cpu().numpy().view(np.uint64), int(found.value)


def same(got, want):
    return got[0] == want[0] and got[4] == want[4] and (got[1] == want[1]).all() and (got[2] == want[2]).all() and (got[3] == want[3]).all()


@pytest.mark.parametrize("n_text", S.TEXTS)
def test_rank_split_device_equals_host_twin_on_the_grid(cuda, n_text):
    """every cell (the one the brute model skips too: the twin is quick), every format: table, index, slots and reported count"""
    t, f, r = M.indices_of(n_text)
    df, dr = device_indices(n_text, cuda)
    for bits, be in H.FORMATS:
        hs = O.StringSet.from_lists(M.patterns_of(n_text, with_n=bits == 4), bits, be)
        ds, max_len = device_set(hs, cuda), int(hs.length.max())
        for params in S.PARAMS:
            for split in S.SPLITS:
                want = HS.host_rank_split(f, r, hs, params, split)
                assert want[0] == 0
                cap = want[4] + 40 if split[0] == M.NO_MAX else 16 * int(hs.length.sum())
                got = device_rank_split(df, dr, ds, params, split, cap, max_len)
                assert same(got, want), (n_text, params, split, bits, be)


@pytest.mark.parametrize("n_text", S.TEXTS)
def test_rank_split_device_equals_the_definition(cuda, n_text):
    """model (a) on the (4, big-endian) format: the cell that exercises everything on this text, and nvmem's own (28, 10) at min_span 19"""
    t, f, r = M.indices_of(n_text)
    df, dr = device_indices(n_text, cuda)
    pats = M.patterns_of(n_text)
    hs = O.StringSet.from_lists(pats, 4, True)
    ds, max_len = device_set(hs, cuda), int(hs.length.max())
    busy = ((1, M.NO_MAX, 1), (1, M.NO_MAX)) if n_text == 77 else ((1, 5, 1), (8, 3))
    for params, split in (busy, ((1, M.NO_MAX, 19), (28, 10))):
        exp, stats = S.expected(n_text, params, split)
        got = device_rank_split(df, dr, ds, params, split, 16 * int(hs.length.sum()), max_len)
        assert got[0] == 0 and got[4] == len(got[3])
        HS.check_table(got[1], got[2], got[3], pats, exp, f)
        if (params, split) == busy:
            assert all(stats[key] > 0 for key in ("candidates", "added", "duplicates", "empty")), stats


@pytest.mark.parametrize("n_text", S.TEXTS)
def test_no_split_sentinel_equals_the_plain_device_entry(cuda, n_text):
    from tests import test_mem_gpu as G
    t, f, r = M.indices_of(n_text)
    df, dr = device_indices(n_text, cuda)
    for bits, be in ((4, True), (2, False)):
        hs = O.StringSet.from_lists(M.patterns_of(n_text, with_n=bits == 4), bits, be)
        ds, max_len = device_set(hs, cuda), int(hs.length.max())
        for params in S.PARAMS:
            cap = int(hs.length.sum())
            want = G.device_rank(df, dr, ds, params, cap, max_len)
            assert same(device_rank_split(df, dr, ds, params, (M.NO_MAX, M.NO_MAX), cap, max_len), want)
            short_want = G.device_rank(df, dr, ds, params, want[4] - 1, max_len)           # too little room: the plain protocol
            short = device_rank_split(df, dr, ds, params, (M.NO_MAX, 3), want[4] - 1, max_len)
            assert short[0] == _lib.ERROR_CAPACITY and same(short, short_want)


def test_capacity_fixed_length_and_empty_batch_on_the_device(cuda):
    t, f, r = M.indices_of(1003)
    df, dr = device_indices(1003, cuda)
    params, split = (1, 5, 1), (8, 3)
    hs = O.StringSet.from_lists(M.patterns_of(1003), 4, True)
    ds, max_len = device_set(hs, cuda), int(hs.length.max())
    want = HS.host_rank_split(f, r, hs, params, split)
    total = want[4]
    # one short of the final count: the error of its own with the host twin's number, nothing past the capacity; that number then suffices
    short = device_rank_split(df, dr, ds, params, split, total - 1, max_len)
    short_want = HS.host_rank_split(f, r, hs, params, split, capacity=total - 1)
    assert short[0] == short_want[0] == _lib.ERROR_CAPACITY and short[4] == short_want[4] > total
    assert device_rank_split(df, dr, ds, params, split, short[4] - 1, max_len)[0] == _lib.ERROR_CAPACITY
    assert same(device_rank_split(df, dr, ds, params, split, short[4], max_len), want)
    # the Python layer does that retry itself
    flt = nvb.MEMFilter()
    flt.rank(df, dr, ds, *params, capacity=total - 1, split_len=split[0], split_width=split[1])
    assert flt.n_ranges() == total and (flt.ranges.cpu().numpy().view(np.uint32) == want[1]).all()
    # a string longer than max_pattern_len: refused after the first pass, nothing reported
    bad = device_rank_split(df, dr, ds, params, split, short[4], max_len - 1)
    assert bad[0] == 1 and bad[4] == 0
    # fixed-length sets
    pats = [M.patterns_of(1003)[2], t[100:119].copy(), t[-19:].copy()]
    hs3 = O.StringSet.from_lists(pats, 2, False)
    want3 = HS.host_rank_split(f, r, hs3, (1, M.NO_MAX, 1), split)
    a = device_rank_split(df, dr, device_set(hs3, cuda), (1, M.NO_MAX, 1), split, 200, 19)
    b = device_rank_split(df, dr, device_set(hs3, cuda, fixed_length=19), (1, M.NO_MAX, 1), split, 200, 19)          # length == NULL
    assert same(a, want3) and same(b, want3)
    # n = 0
    fs, rs, ss = df.struct(), dr.struct(), ds.struct()
    index = torch.full((1,), -1, dtype=torch.int64, device=cuda)
    found = C.c_uint64(5)
    assert nvb.lib().nvbio_hip_fm_mem_rank_split(C.byref(fs), C.byref(rs), C.byref(ss), 0, 19, 1, 5, 1, 8, 3, None, 0, C.c_void_p(index.data_ptr()), None, C.byref(found),
                                                 None, 0, _lib.current_stream_ptr()) == 0
    torch.cuda.synchronize()
    assert int(index[0]) == 0 and found.value == 0
    # a batch in which nothing matches: an index of zeros
    none = O.StringSet.from_lists([np.full(9, 4, np.uint8), np.full(3, 4, np.uint8)], 4, True)
    got = device_rank_split(df, dr, device_set(none, cuda), params, split, 8, 9)
    assert got[0] == 0 and got[4] == 0 and (got[2] == 0).all()


@pytest.mark.parametrize("n_text", S.TEXTS)
def test_memfilter_keywords_first_hit_and_locate(cuda, n_text):
    t, f, r = M.indices_of(n_text)
    df, dr = device_indices(n_text, cuda)
    params, split = (1, 5, 1), (8, 3)
    pats = M.patterns_of(n_text)
    hs = O.StringSet.from_lists(pats, 4, True)
    err, ranges, index, slots, found = HS.host_rank_split(f, r, hs, params, split)
    total = int(slots[-1])
    want_hits = H.host_locate(f, ranges, slots, 0, total)
    ds = device_set(hs, cuda)
    flt = nvb.MEMFilter()
    assert flt.rank(df, dr, ds, *params, split_len=split[0], split_width=split[1]) == total and flt.n_mems() == total and flt.n_ranges() == found
    assert (flt.ranges.cpu().numpy().view(np.uint32) == ranges).all() and (flt.index.cpu().numpy().view(np.uint64) == index).all()
    assert (flt.locate(0, total).cpu().numpy().view(np.uint32) == want_hits).all()
    for begin, end in ((1, total - 1), (total // 3, total // 3 + 2)):               # sub-ranges that cut a MEM's rows
        assert (flt.locate(begin, end).cpu().numpy().view(np.uint32) == want_hits[begin:end]).all()
    for i in range(len(pats)):
        assert flt.first_hit(i) == (int(slots[int(index[i]) - 1]) if int(index[i]) else 0)
    # the defaults are today's path
    plain = nvb.MEMFilter()
    plain.rank(df, dr, ds, *params)
    assert (plain.ranges.cpu().numpy().view(np.uint32) == H.host_rank(f, r, hs, params)[1]).all()


CXX_CASES = ((1003, (1, M.NO_MAX, 1), (8, 3)), (20000, (1, 5, 1), (8, 3)), (77, (1, M.NO_MAX, 1), (1, M.NO_MAX)))


def test_cxx_host_layer_memfilter_with_split(cuda):
    """include/nvbio_hip/fmindex.h: MEMFilterDevice::rank(..., split_len, split_width) behind tests/cxx/mem_split_shim.cpp"""
    shim = C.CDLL(os.path.join(HERE, "cxx", "libmem_split_shim.so"))
    for n_text, params, split in CXX_CASES:
        t, f, r = M.indices_of(n_text)
        df, dr = device_indices(n_text, cuda)
        pats = M.patterns_of(n_text)
        hs = O.StringSet.from_lists(pats, 4, False)
        err, ranges, index, slots, found = HS.host_rank_split(f, r, hs, params, split)
        total = int(slots[-1])
        begin, end = total // 4, total - 1
        want_hits = H.host_locate(f, ranges, slots, begin, end)
        ds = device_set(hs, cuda)
        fs, rs, ss = df.struct(), dr.struct(), ds.struct()
        n = len(pats)
        g_ranges, g_slots = np.zeros((found + 8, 4), np.uint32), np.zeros(found + 8, np.uint64)
        g_index, g_first = np.zeros(n + 1, np.uint64), np.zeros(n, np.uint64)
        n_ranges, n_mems = C.c_uint64(0), C.c_uint64(0)
        d_hits = torch.zeros((end - begin, 4), dtype=torch.int32, device=cuda)
        rc = shim.mem_split_host_class(C.byref(fs), C.byref(rs), C.byref(ss), n, params[0], params[1], params[2], split[0], split[1], C.c_uint64(found + 8),
                                       g_ranges.ctypes.data_as(C.c_void_p), g_slots.ctypes.data_as(C.c_void_p), g_index.ctypes.data_as(C.c_void_p),
                                       g_first.ctypes.data_as(C.c_void_p), C.byref(n_ranges), C.byref(n_mems), C.c_uint64(begin), C.c_uint64(end), C.c_void_p(d_hits.data_ptr()))
        assert rc == 0 and n_ranges.value == found and n_mems.value == total
        assert (g_ranges[:found] == ranges).all() and (g_slots[:found] == slots).all() and (g_index == index).all()
        assert [int(v) for v in g_first] == [int(slots[int(index[i]) - 1]) if int(index[i]) else 0 for i in range(n)]
        assert (d_hits.cpu().numpy().view(np.uint32) == want_hits).all()


def _index_args(host, to):
    return (host.primary, to(np.asarray(host.L2, np.uint32)), to(host.bwt_occ), to(host.ssa))


def test_compat_filters_with_split(cuda):
    """tests/compat/mem_split_callers.hip: MEMFilterHost, and MEMFilterDevice in its three executions -- 4-bit packed reads take the
    C-ABI, one byte a symbol the per-lane templates, and so does set_tuned(false); all give the host twin's table, index, first hits
    and a cut of the hits, and last_path() says which ran"""
    lib = C.CDLL(os.path.join(HERE, "compat", "libmem_split_callers.so"))
    for n_text, params, split in CXX_CASES:
        t, f, r = M.indices_of(n_text)
        pats = M.patterns_of(n_text)
        hs = O.StringSet.from_lists(pats, 4, True)
        err, ranges, index, slots, found = HS.host_rank_split(f, r, hs, params, split)
        total, n = int(slots[-1]), len(pats)
        begin, end = min(1, total), total - 1
        want_hits = H.host_locate(f, ranges, slots, begin, end)
        first = [int(slots[int(index[i]) - 1]) if int(index[i]) else 0 for i in range(n)]
        spans = np.stack([hs.begin, hs.begin + hs.length], axis=1).astype(np.uint32)
        # ---- host filter
        keep = []
        host_ptr = lambda a: (keep.append(np.ascontiguousarray(a)), keep[-1].ctypes.data_as(C.c_void_p))[1]
        g_ranges, g_slots, g_first = np.zeros((found + 4, 4), np.uint32), np.zeros(found + 4, np.uint64), np.zeros(n, np.uint64)
        g_hits = np.zeros((end - begin, 4), np.uint32)
        n_mems, n_ranges = C.c_uint64(0), C.c_uint64(0)
        rc = lib.compat_mem_split_host(f.length, *_index_args(f, host_ptr), *_index_args(r, host_ptr), host_ptr(hs.words), host_ptr(spans), n, params[0], params[1], params[2],
                                       split[0], split[1], C.byref(n_mems), C.byref(n_ranges), host_ptr(g_ranges), host_ptr(g_slots), found + 4, host_ptr(g_first),
                                       C.c_uint64(begin), C.c_uint64(end), host_ptr(g_hits))
        g_ranges, g_slots, g_first, g_hits = keep[-4], keep[-3], keep[-2], keep[-1]
        assert rc == 0 and n_mems.value == total and n_ranges.value == found
        assert (g_ranges[:found] == ranges).all() and (g_slots[:found] == slots).all() and [int(v) for v in g_first] == first
        assert (g_hits == want_hits).all()
        # ---- device filter
        dkeep = []
        dev_ptr = lambda a: (dkeep.append(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).to(cuda)), C.c_void_p(dkeep[-1].data_ptr()))[1]
        for bits, tuned, want_path, want_locate in ((4, 1, b"tuned", b"tuned"), (8, 1, b"generic", b"tuned"), (4, 0, b"generic", b"generic")):
            symbols = hs.words if bits == 4 else np.concatenate(pats).astype(np.uint8)
            d_ranges = torch.zeros((found + 4, 4), dtype=torch.int32, device=cuda)
            d_slots = torch.zeros(found + 4, dtype=torch.int64, device=cuda)
            d_index = torch.zeros(n + 1, dtype=torch.int64, device=cuda)
            d_hits = torch.zeros((end - begin, 4), dtype=torch.int32, device=cuda)
            d_first = np.zeros(n, np.uint64)
            path, locate_path = C.create_string_buffer(16), C.create_string_buffer(16)
            rc = lib.compat_mem_split_filter_device(bits, tuned, f.length, *_index_args(f, dev_ptr), *_index_args(r, dev_ptr), dev_ptr(symbols), dev_ptr(spans), n,
                                                    params[0], params[1], params[2], split[0], split[1], C.byref(n_mems), C.byref(n_ranges), C.c_void_p(d_ranges.data_ptr()),
                                                    C.c_void_p(d_slots.data_ptr()), C.c_void_p(d_index.data_ptr()), found + 4, d_first.ctypes.data_as(C.c_void_p),
                                                    C.c_uint64(begin), C.c_uint64(end), C.c_void_p(d_hits.data_ptr()), path, locate_path)
            assert rc == 0 and path.value == want_path and locate_path.value == want_locate, (n_text, bits, tuned, rc, path.value)
            assert n_mems.value == total and n_ranges.value == found
            assert (d_ranges[:found].cpu().numpy().view(np.uint32) == ranges).all() and (d_slots[:found].cpu().numpy().view(np.uint64) == slots).all()
            assert (d_index.cpu().numpy().view(np.uint64) == index).all() and [int(v) for v in d_first] == first
            assert (d_hits.cpu().numpy().view(np.uint32) == want_hits).all()


def test_a_batch_across_waves_and_blocks_equals_the_host_twin(cuda):
    """1 000 reads of 100 symbols cut from the 20 000-symbol text with 2 % substitutions, (1, NO_MAX, 1) and split (8, 3): four blocks,
    sixteen waves, segments of different sizes side by side in the staging table"""
    t, f, r = M.indices_of(20000)
    df, dr = device_indices(20000, cuda)
    rng = np.random.default_rng(2024)
    n, ln = 1000, 100
    at = rng.integers(0, 20000 - ln, n)
    reads = t[at[:, None] + np.arange(ln)[None, :]].copy()
    flips = rng.random(reads.shape) < 0.02
    reads[flips] = (reads[flips] + rng.integers(1, 4, int(flips.sum()))) & 3
    hs = O.StringSet(O.pack(reads.reshape(-1), 4, True), 4, True, np.arange(n, dtype=np.uint64) * ln, np.full(n, ln, np.uint32))
    params, split = (1, M.NO_MAX, 1), (8, 3)
    want = HS.host_rank_split(f, r, hs, params, split, capacity=n * 200)
    plain = H.host_rank(f, r, hs, params)
    assert want[0] == 0 and want[4] > plain[4] > n                     # re-seeding adds spans here
    got = device_rank_split(df, dr, device_set(hs, cuda), params, split, n * 200, ln)
    assert same(got, want)
    counts = np.diff(want[2].astype(np.int64))
    assert counts.min() != counts.max()
