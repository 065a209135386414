"""MEM seeding on the GPU: nvbio_hip_fm_extend / nvbio_hip_fm_mem_rank / nvbio_hip_fm_mem_locate and nvbio_amd.MEMFilter against their
`_host` twins and the two models of tests/mem_reference.py, on the cases of tests/test_mem_host.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import nvbio_amd as nvb
from nvbio_amd import _lib
from oracle import pyoracle as O
from tests import mem_reference as M
from tests import test_mem_host as H

pytestmark = pytest.mark.gpu

_dev = {}


def device_indices(n_text, cuda):
    if n_text not in _dev:
        t, f, r = M.indices_of(n_text)
        _dev[n_text] = (nvb.FMIndexDevice.from_host(f, cuda), nvb.FMIndexDevice.from_host(r, cuda))
    return _dev[n_text]


def device_set(hs, cuda, fixed_length=0):
    return nvb.PackedStringSet.from_host(hs.words, hs.bits, hs.big_endian, hs.begin, None if fixed_length else hs.length, fixed_length, device=cuda)


def device_rank(df, dr, ds, params, capacity, max_len):
    """the ABI entry itself -> (error, ranges [k, 4], index [n + 1], slots [k], number found), as numpy"""
    L = nvb.lib()
    n = len(ds)
    dev = ds.words.device
    tb = int(L.nvbio_hip_fm_mem_temp_bytes(n, max_len))
    temp = torch.empty(tb, dtype=torch.uint8, device=dev)
    ranges = torch.full((max(capacity, 1), 4), -1, dtype=torch.int32, device=dev)
    slots = torch.full((max(capacity, 1),), -1, dtype=torch.int64, device=dev)
    index = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    found = C.c_uint64(0)
    fs, rs, ss = df.struct(), dr.struct(), ds.struct()
    err = L.nvbio_hip_fm_mem_rank(C.byref(fs), C.byref(rs), C.byref(ss), n, max_len, params[0], params[1], params[2],
                                  C.c_void_p(ranges.data_ptr()), capacity, C.c_void_p(index.data_ptr()), C.c_void_p(slots.data_ptr()), C.byref(found),
                                  C.c_void_p(temp.data_ptr()), tb, _lib.current_stream_ptr())
    torch.cuda.synchronize()
    k = min(int(found.value), capacity)
    assert bool((ranges[k:] == -1).all()) and bool((slots[k:] == -1).all())                # nothing past what was found, or past the capacity
    return err, ranges[:k].cpu().numpy().view(np.uint32), index.cpu().numpy().view(np.uint64), slots[:k].cpu().numpy().view(np.uint64), int(found.value)


@pytest.mark.parametrize("n_text", H.TEXTS)
def test_rank_device_equals_host_twin_and_models(cuda, n_text):
    t, f, r = M.indices_of(n_text)
    df, dr = device_indices(n_text, cuda)
    for params in M.PARAMS:
        for bits, be in H.FORMATS:
            pats = M.patterns_of(n_text, with_n=bits == 4)
            hs = O.StringSet.from_lists(pats, bits, be)
            want = H.host_rank(f, r, hs, params)
            got = device_rank(df, dr, device_set(hs, cuda), params, int(hs.length.sum()), int(hs.length.max()))
            assert got[0] == 0 and got[4] == want[4]
            assert (got[1] == want[1]).all() and (got[2] == want[2]).all() and (got[3] == want[3]).all(), (n_text, params, bits, be)
            if (bits, be) == (4, True):
                H.check_against_models(n_text, params, got[1], got[2], got[3], pats, M.expected(n_text, params), f, r, bidir=False)


def test_fixed_length_capacity_and_empty_batch_on_the_device(cuda):
    t, f, r = M.indices_of(1003)
    df, dr = device_indices(1003, cuda)
    pats = [M.patterns_of(1003)[2], t[100:119].copy(), t[-19:].copy()]
    hs = O.StringSet.from_lists(pats, 2, False)
    a = device_rank(df, dr, device_set(hs, cuda), M.PARAMS[0], 57, 19)
    b = device_rank(df, dr, device_set(hs, cuda, fixed_length=19), M.PARAMS[0], 57, 19)            # length == NULL
    want = H.host_rank(f, r, hs, M.PARAMS[0])
    assert a[0] == 0 and b[0] == 0 and (a[1] == want[1]).all() and (b[1] == want[1]).all() and (b[2] == want[2]).all()
    # one short of the total: the true count, the error of its own, nothing past the capacity; the retry then succeeds
    hs = O.StringSet.from_lists(M.patterns_of(1003), 4, True)
    want = H.host_rank(f, r, hs, M.PARAMS[0])
    ds, total, max_len = device_set(hs, cuda), want[4], int(hs.length.max())
    short = device_rank(df, dr, ds, M.PARAMS[0], total - 1, max_len)
    assert short[0] == _lib.ERROR_CAPACITY and short[4] == total and (short[1] == want[1][:-1]).all() and (short[3] == want[3][:-1]).all()
    again = device_rank(df, dr, ds, M.PARAMS[0], short[4], max_len)
    assert again[0] == 0 and (again[1] == want[1]).all()
    # the Python layer does that retry itself
    flt = nvb.MEMFilter()
    flt.rank(df, dr, ds, capacity=total - 1)
    assert flt.n_ranges() == total and (flt.ranges.cpu().numpy().view(np.uint32) == want[1]).all()
    # a string longer than max_pattern_len: refused after the first pass, nothing stored (the kernel walks max_pattern_len symbols of it)
    bad = device_rank(df, dr, ds, M.PARAMS[0], total, max_len - 1)
    assert bad[0] == 1 and bad[4] == 0
    # n = 0
    fs, rs, ss = df.struct(), dr.struct(), ds.struct()
    index = torch.full((1,), -1, dtype=torch.int64, device=cuda)
    found = C.c_uint64(5)
    assert nvb.lib().nvbio_hip_fm_mem_rank(C.byref(fs), C.byref(rs), C.byref(ss), 0, 19, 1, 5, 1, None, 0, C.c_void_p(index.data_ptr()), None, C.byref(found),
                                           None, 0, _lib.current_stream_ptr()) == 0
    torch.cuda.synchronize()
    assert int(index[0]) == 0 and found.value == 0


@pytest.mark.parametrize("n_text", H.TEXTS)
def test_memfilter_locate_first_hit_and_accelerated_indices(cuda, n_text):
    t, f, r = M.indices_of(n_text)
    df, dr = device_indices(n_text, cuda)
    params = (1, 5, 1) if n_text == 20000 else M.PARAMS[0]
    pats = M.patterns_of(n_text)
    hs = O.StringSet.from_lists(pats, 4, True)
    err, ranges, index, slots, found = H.host_rank(f, r, hs, params)
    total = int(slots[-1])
    want_hits = H.host_locate(f, ranges, slots, 0, total)
    ds = device_set(hs, cuda)
    flt = nvb.MEMFilter()
    assert flt.rank(df, dr, ds, *params) == total and flt.n_mems() == total and flt.n_ranges() == found
    assert (flt.ranges.cpu().numpy().view(np.uint32) == ranges).all() and (flt.index.cpu().numpy().view(np.uint64) == index).all()
    assert (flt.locate(0, total).cpu().numpy().view(np.uint32) == want_hits).all()
    for begin, end in ((1, total - 1), (total // 3, total // 3 + 2), (total // 2, total // 2)):       # sub-ranges that cut a MEM's rows
        if 0 <= begin <= end <= total:
            assert (flt.locate(begin, end).cpu().numpy().view(np.uint32) == want_hits[begin:end]).all()
    for i in range(len(pats)):
        first = int(slots[int(index[i]) - 1]) if int(index[i]) else 0
        assert flt.first_hit(i) == first
        if int(index[i + 1]) > int(index[i]):
            assert int(want_hits[first, 1]) == i
    # the line-native index and the k-mer table are ignored by rank, used by locate: same results
    acc = nvb.MEMFilter()
    assert acc.rank(df.with_dimer().with_ktab(4), dr.with_dimer().with_ktab(4), ds, *params) == total
    assert (acc.ranges.cpu().numpy().view(np.uint32) == ranges).all()
    assert (acc.locate(0, total).cpu().numpy().view(np.uint32) == want_hits).all()


@pytest.mark.parametrize("n_text", H.TEXTS)
def test_extend_device_equals_host_twin(cuda, n_text):
    """every (string, prefix length) and (string, suffix length) of the host test as one batch each way"""
    t, f, r = M.indices_of(n_text)
    df, dr = device_indices(n_text, cuda)
    for direction in (0, 1):
        strings = H.extend_strings(n_text)
        fr = np.tile(np.array([0, f.length], np.uint32), (len(strings), 1))
        rr = np.tile(np.array([0, r.length], np.uint32), (len(strings), 1))
        for step in range(max(len(s) for s in strings) + 1):
            c = np.array([(s[step] if direction == 0 else s[len(s) - 1 - step]) if step < len(s) else 4 for s in strings], np.uint8)
            want_f, want_r = H.host_extend(direction, f, r, fr, rr, c)
            fn = nvb.extend_forward if direction == 0 else nvb.extend_backwards
            got_f, got_r = fn(df, dr, torch.from_numpy(fr.view(np.int32)).to(cuda), torch.from_numpy(rr.view(np.int32)).to(cuda), torch.from_numpy(c).to(cuda))
            assert (got_f.cpu().numpy().view(np.uint32) == want_f).all() and (got_r.cpu().numpy().view(np.uint32) == want_r).all()
            live = want_f[:, 0] <= want_f[:, 1]
            fr, rr = np.where(live[:, None], want_f, fr), np.where(live[:, None], want_r, rr)         # an emptied job keeps its last range


def test_large_agreement_with_the_host_twin(cuda):
    """2^20-symbol text, 20 000 reads of 150 with planted substitutions and Ns: device == host twin (ranks and a slice of the hits)"""
    rng = np.random.default_rng(99)
    n_text, n, ln = 1 << 20, 20000, 150
    text = rng.integers(0, 4, n_text, dtype=np.uint8)
    text[5000:5400] = 0
    f, r = O.FMIndex(text), O.FMIndex(np.ascontiguousarray(text[::-1]))
    at = rng.integers(0, n_text - ln, n)
    reads = text[at[:, None] + np.arange(ln)[None, :]]
    flips = rng.random(reads.shape) < 0.02
    reads[flips] = rng.integers(0, 4, int(flips.sum()))
    reads[rng.random(reads.shape) < 0.002] = 4
    reads[:50] = 0                                         # inside the run
    hs = O.StringSet(O.pack(reads.reshape(-1), 4, True), 4, True, np.arange(n, dtype=np.uint64) * ln, np.full(n, ln, np.uint32))
    df, dr = nvb.FMIndexDevice.from_host(f, cuda), nvb.FMIndexDevice.from_host(r, cuda)
    ds = device_set(hs, cuda)
    for params in ((1, M.NO_MAX, 1), (2, 10000, 19), (1, 10000, 19)):
        want = H.host_rank(f, r, hs, params, capacity=n * 40)
        got = device_rank(df, dr, ds, params, n * 40, ln)
        assert want[0] == 0 and got[0] == 0 and got[4] == want[4] >= 50       # the reads inside the run, whatever the parameters
        assert params[0] != 1 or want[4] > n
        assert (got[1] == want[1]).all() and (got[2] == want[2]).all() and (got[3] == want[3]).all()
    flt = nvb.MEMFilter()
    total = flt.rank(df, dr, ds, *params)
    assert total == int(want[3][-1])
    lo = total // 2
    assert (flt.locate(lo, lo + 5000).cpu().numpy().view(np.uint32) == H.host_locate(f, want[1], want[3], lo, lo + 5000)).all()


def test_cxx_host_layer_memfilter_equals_the_abi(cuda):
    """include/nvbio_hip/fmindex.h: MEMFilterDevice behind tests/cxx/mem_shim.cpp -- rank table, index, first hits, a cut of the hits"""
    import os
    shim = C.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx", "libmem_shim.so"))
    for n_text, params in ((1003, M.PARAMS[0]), (20000, (1, 5, 19))):
        t, f, r = M.indices_of(n_text)
        df, dr = device_indices(n_text, cuda)
        pats = M.patterns_of(n_text)
        hs = O.StringSet.from_lists(pats, 4, False)
        err, ranges, index, slots, found = H.host_rank(f, r, hs, params)
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
        rc = shim.mem_host_class(C.byref(fs), C.byref(rs), C.byref(ss), n, params[0], params[1], params[2], C.c_uint64(found + 8),
                                 g_ranges.ctypes.data_as(C.c_void_p), g_slots.ctypes.data_as(C.c_void_p), g_index.ctypes.data_as(C.c_void_p),
                                 g_first.ctypes.data_as(C.c_void_p), C.byref(n_ranges), C.byref(n_mems), C.c_uint64(begin), C.c_uint64(end), C.c_void_p(d_hits.data_ptr()))
        assert rc == 0 and n_ranges.value == found and n_mems.value == total
        assert (g_ranges[:found] == ranges).all() and (g_slots[:found] == slots).all() and (g_index == index).all()
        assert [int(v) for v in g_first] == [int(slots[int(index[i]) - 1]) if int(index[i]) else 0 for i in range(n)]
        assert (d_hits.cpu().numpy().view(np.uint32) == want_hits).all()


def _index_args(host, to):
    return (host.primary, to(np.asarray(host.L2, np.uint32)), to(host.bwt_occ), to(host.ssa))


def test_compat_callers_agree_with_the_abi(cuda):
    """tests/compat/mem_callers.hip: MEMFilterHost (rank, first_hit, string_batch_bound, locate over a range that cuts MEMs) and a kernel
    whose threads run find_kmems / extend_forward / extend_backwards themselves"""
    import os
    lib = C.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "compat", "libmem_callers.so"))
    for n_text, params in ((77, M.PARAMS[0]), (1003, M.PARAMS[1]), (20000, (1, 5, 19))):
        t, f, r = M.indices_of(n_text)
        pats = M.patterns_of(n_text)
        hs = O.StringSet.from_lists(pats, 4, True)
        err, ranges, index, slots, found = H.host_rank(f, r, hs, params)
        total, n = int(slots[-1]), len(pats)
        begin, end = min(1, total), total - 1
        want_hits = H.host_locate(f, ranges, slots, begin, end)
        first = [int(slots[int(index[i]) - 1]) if int(index[i]) else 0 for i in range(n)] + [total]
        spans = np.stack([hs.begin, hs.begin + hs.length], axis=1).astype(np.uint32)
        # ---- host filter
        keep = []
        host_ptr = lambda a: (keep.append(np.ascontiguousarray(a)), keep[-1].ctypes.data_as(C.c_void_p))[1]
        g_ranges, g_slots, g_first = np.zeros((found + 4, 4), np.uint32), np.zeros(found + 4, np.uint64), np.zeros(n, np.uint64)
        g_hits = np.zeros((end - begin, 4), np.uint32)
        n_mems, n_ranges, bound = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
        count = first[n // 2] + 1
        rc = lib.compat_mem_host(f.length, *_index_args(f, host_ptr), *_index_args(r, host_ptr), host_ptr(hs.words), host_ptr(spans), n, params[0], params[1], params[2],
                                 C.byref(n_mems), C.byref(n_ranges), host_ptr(g_ranges), host_ptr(g_slots), found + 4, host_ptr(g_first), count, C.byref(bound),
                                 C.c_uint64(begin), C.c_uint64(end), host_ptr(g_hits))
        g_ranges, g_slots, g_first, g_hits = keep[-4], keep[-3], keep[-2], keep[-1]
        assert rc == 0 and n_mems.value == total and n_ranges.value == found
        assert (g_ranges[:found] == ranges).all() and (g_slots[:found] == slots).all() and [int(v) for v in g_first] == first[:n]
        assert bound.value == max(i for i in range(n + 1) if first[i] <= count)
        assert (g_hits == want_hits).all()
        # ---- the templates inside a kernel
        dev_ptr_keep = []
        dev_ptr = lambda a: (dev_ptr_keep.append(torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(cuda)), C.c_void_p(dev_ptr_keep[-1].data_ptr()))[1]
        max_len = per_read = int(hs.length.max())            # a string has at most as many MEMs as symbols
        store = torch.zeros((n * max_len, 4), dtype=torch.int32, device=cuda)
        out = torch.zeros((n, per_read, 4), dtype=torch.int32, device=cuda)
        counts = torch.zeros(n, dtype=torch.int32, device=cuda)
        ext = torch.zeros((n, 4, 2), dtype=torch.int32, device=cuda)
        rc = lib.compat_mem_device(f.length, *_index_args(f, dev_ptr), *_index_args(r, dev_ptr), dev_ptr(hs.words), dev_ptr(spans), n, params[0], params[1], params[2],
                                   C.c_void_p(store.data_ptr()), max_len, C.c_void_p(out.data_ptr()), per_read, C.c_void_p(counts.data_ptr()), C.c_void_p(ext.data_ptr()))
        assert rc == 0
        counts_h, out_h, ext_h = counts.cpu().numpy(), out.cpu().numpy().view(np.uint32), ext.cpu().numpy().view(np.uint32)
        assert (counts_h == np.diff(index.astype(np.int64))).all() and counts_h.max() <= per_read
        for i in range(n):
            assert (out_h[i, :counts_h[i]] == ranges[int(index[i]):int(index[i + 1])]).all()
        want_f, want_r = f.match(hs), r.match(O.StringSet.from_lists([p[::-1] for p in pats], 4, True))
        for i in range(n):
            if want_f[i, 0] <= want_f[i, 1]:
                assert (ext_h[i, 0] == want_f[i]).all() and (ext_h[i, 1] == want_r[i]).all() and (ext_h[i, 2] == want_f[i]).all() and (ext_h[i, 3] == want_r[i]).all()
            else:
                assert ext_h[i, 0, 0] == ext_h[i, 0, 1] + 1 and ext_h[i, 2, 0] == ext_h[i, 2, 1] + 1


def test_compat_device_filter_both_executions(cuda):
    """MEMFilterDevice of the drop-in layer (tests/compat/mem_callers.hip): 4-bit packed reads take the C-ABI, one byte a symbol the
    per-lane templates, and so does set_tuned(false); all give the host twin's rank table, index, first hits and a cut of the hits"""
    import os
    lib = C.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "compat", "libmem_callers.so"))
    for n_text, params in ((77, M.PARAMS[0]), (1003, M.PARAMS[1]), (20000, (1, 5, 19))):
        t, f, r = M.indices_of(n_text)
        pats = M.patterns_of(n_text)
        hs = O.StringSet.from_lists(pats, 4, True)
        err, ranges, index, slots, found = H.host_rank(f, r, hs, params)
        total, n = int(slots[-1]), len(pats)
        begin, end = min(1, total), total - 1
        want_hits = H.host_locate(f, ranges, slots, begin, end)
        first = [int(slots[int(index[i]) - 1]) if int(index[i]) else 0 for i in range(n)]
        spans = np.stack([hs.begin, hs.begin + hs.length], axis=1).astype(np.uint32)
        keep = []
        dev_ptr = lambda a: (keep.append(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).to(cuda)), C.c_void_p(keep[-1].data_ptr()))[1]
        for bits, tuned, want_path, want_locate in ((4, 1, b"tuned", b"tuned"), (8, 1, b"generic", b"tuned"), (4, 0, b"generic", b"generic")):
            symbols = hs.words if bits == 4 else np.concatenate(pats).astype(np.uint8)
            g_ranges = torch.zeros((found + 4, 4), dtype=torch.int32, device=cuda)
            g_slots = torch.zeros(found + 4, dtype=torch.int64, device=cuda)
            g_index = torch.zeros(n + 1, dtype=torch.int64, device=cuda)
            g_hits = torch.zeros((end - begin, 4), dtype=torch.int32, device=cuda)
            g_first = np.zeros(n, np.uint64)
            n_mems, n_ranges = C.c_uint64(0), C.c_uint64(0)
            path, locate_path = C.create_string_buffer(16), C.create_string_buffer(16)
            rc = lib.compat_mem_filter_device(bits, tuned, f.length, *_index_args(f, dev_ptr), *_index_args(r, dev_ptr), dev_ptr(symbols), dev_ptr(spans), n,
                                              params[0], params[1], params[2], C.byref(n_mems), C.byref(n_ranges), C.c_void_p(g_ranges.data_ptr()),
                                              C.c_void_p(g_slots.data_ptr()), C.c_void_p(g_index.data_ptr()), found + 4, g_first.ctypes.data_as(C.c_void_p),
                                              C.c_uint64(begin), C.c_uint64(end), C.c_void_p(g_hits.data_ptr()), path, locate_path)
            assert rc == 0 and path.value == want_path and locate_path.value == want_locate
            assert n_mems.value == total and n_ranges.value == found
            assert (g_ranges[:found].cpu().numpy().view(np.uint32) == ranges).all() and (g_slots[:found].cpu().numpy().view(np.uint64) == slots).all()
            assert (g_index.cpu().numpy().view(np.uint64) == index).all() and [int(v) for v in g_first] == first
            assert (g_hits.cpu().numpy().view(np.uint32) == want_hits).all()
