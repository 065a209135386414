"""MEM re-seeding on the CPU: nvbio_hip_fm_mem_rank_split_host against the two models of tests/mem_split_reference.py on the shared
grid, its capacity protocol, the no-split sentinel against the plain twin, and locate over its result."""
import ctypes as C

import numpy as np
import pytest

import nvbio_amd
from nvbio_amd import _lib
from oracle import pyoracle as O
from tests import mem_reference as M
from tests import mem_split_reference as S
from tests import test_mem_host as H

FORMATS = H.FORMATS


def host_rank_split(f, r, hs, params, split, capacity=None, fixed_length=0, want_records=False):
    """-> (error, ranges [k, 4], index [n + 1], slots [k], number reported); k = the records stored (none after an error)"""
    L = nvbio_amd.lib()
    n = len(hs)
    max_len = fixed_length or (int(hs.length.max()) if n else 0)
    cap = 16 * int(hs.length.sum()) if capacity is None else capacity
    ranges = np.full((max(cap, 1), 4), 0xDEADBEEF, np.uint32)
    slots = np.full(max(cap, 1), 0xDEADBEEF, np.uint64)
    index = np.zeros(n + 1, np.uint64)
    found, records = C.c_uint64(0), C.c_uint64(0)
    fs, rs, ss = H.fm_struct(f), H.fm_struct(r), H.sset(hs, fixed_length)
    err = L.nvbio_hip_fm_mem_rank_split_host(C.byref(fs), C.byref(rs), C.byref(ss), n, max_len, params[0], params[1], params[2], split[0], split[1],
                                             ranges.ctypes.data, cap, index.ctypes.data, slots.ctypes.data, C.byref(found), C.byref(records), 2)
    k = min(int(found.value), cap)
    assert (ranges[cap:] == 0xDEADBEEF).all() and (slots[cap:] == 0xDEADBEEF).all()         # nothing past the capacity, whatever happened
    if err == 0:
        assert (ranges[k:] == 0xDEADBEEF).all() and (slots[k:] == 0xDEADBEEF).all()         # nor past what was stored
    elif split[0] != M.NO_MAX:
        k = 0
    if want_records:
        return err, ranges[:k], index, slots[:k], int(found.value), int(records.value)
    return err, ranges[:k], index, slots[:k], int(found.value)


def check_table(ranges, index, slots, pats, exp, f):
    """the rank table of `pats` holds model (a)'s spans, in its order, with the SA ranges match() gives the substrings"""
    assert int(index[0]) == 0 and int(index[-1]) == len(slots) == len(ranges)
    assert (np.diff(index.astype(np.int64)) >= 0).all()
    for i, p in enumerate(pats):
        got = ranges[int(index[i]):int(index[i + 1])]
        assert [(int(g[3]) & 0xFFFF, int(g[3]) >> 16) for g in got] == [(b, e) for b, e, _ in exp[i]], i
        assert (got[:, 2] == i).all()                                           # string id, top bit clear
        assert [int(g[1]) - int(g[0]) + 1 for g in got] == [len(o) for _, _, o in exp[i]]
        if len(got):
            subs = O.StringSet.from_lists([p[b:e] for b, e, _ in exp[i]], 4, True)
            assert (got[:, :2] == f.match(subs)).all()
    assert (slots == np.cumsum(ranges[:, 1].astype(np.uint64) - ranges[:, 0] + 1)).all()


@pytest.mark.parametrize("n_text", S.TEXTS)
def test_rank_split_host_equals_both_models(n_text):
    t, f, r = M.indices_of(n_text)
    seen = {"candidates": False, "added": False, "duplicates": False, "empty": False, "all four": False, "nested": False}
    for params, split in S.cells(n_text):
        for bits, be in FORMATS:
            pats = M.patterns_of(n_text, with_n=bits == 4)
            exp, stats = S.expected(n_text, params, split, with_n=bits == 4)
            hs = O.StringSet.from_lists(pats, bits, be)
            err, ranges, index, slots, found = host_rank_split(f, r, hs, params, split)
            assert err == 0 and found == len(slots), (params, split, bits, be)
            check_table(ranges, index, slots, pats, exp, f)
            if (bits, be) != (4, True):
                continue
            for i, p in enumerate(pats):                                        # model (b)
                got = ranges[int(index[i]):int(index[i + 1])]
                assert [tuple(int(v) for v in (g[3] & 0xFFFF, g[3] >> 16, g[0], g[1])) for g in got] == S.split_bidir(f, r, p, params, split), (i, params, split)
                ends = [e for _, e, _ in exp[i]]
                seen["nested"] |= any(a > b for a, b in zip(ends, ends[1:]))
            # model (a) alone says whether the cell exercises re-seeding
            for key in ("candidates", "added", "duplicates", "empty"):
                seen[key] |= stats[key] > 0
            seen["all four"] |= all(stats[key] > 0 for key in ("candidates", "added", "duplicates", "empty"))
    assert all(seen.values()), seen          # the grid is not vacuous on this text; `nested`: some output's ends are not monotone


@pytest.mark.parametrize("n_text", S.TEXTS)
def test_no_split_sentinel_equals_the_plain_twin(n_text):
    t, f, r = M.indices_of(n_text)
    for params in S.PARAMS:
        for bits, be in FORMATS:
            hs = O.StringSet.from_lists(M.patterns_of(n_text, with_n=bits == 4), bits, be)
            want = H.host_rank(f, r, hs, params, want_records=True)
            cap = int(hs.length.sum())
            got = host_rank_split(f, r, hs, params, (M.NO_MAX, M.NO_MAX), capacity=cap, want_records=True)
            assert got[0] == want[0] == 0 and got[4:] == want[4:]
            assert (got[1] == want[1]).all() and (got[2] == want[2]).all() and (got[3] == want[3]).all()
            # and with too little room: the plain twin's protocol, the first records stored
            short_want = H.host_rank(f, r, hs, params, capacity=want[4] - 1)
            short = host_rank_split(f, r, hs, params, (M.NO_MAX, 3), capacity=want[4] - 1)
            assert short[0] == short_want[0] == _lib.ERROR_CAPACITY and short[4] == short_want[4]
            assert (short[1] == short_want[1]).all() and (short[2] == short_want[2]).all() and (short[3] == short_want[3]).all()


def test_at_min_span_19_on_text_77_every_candidate_is_empty():
    """the case for keeping the split MEM: at min_span 19 on the 77-symbol text no re-seed through a midpoint survives"""
    stats = {}
    for split in S.SPLITS[:-1]:
        stats[split] = S.expected(77, (1, M.NO_MAX, 19), split)[1]
    assert any(s["candidates"] > 0 for s in stats.values())
    assert all(s["empty"] == s["candidates"] and s["added"] == 0 for s in stats.values()), stats


def test_capacity_protocol():
    t, f, r = M.indices_of(1003)
    pats = M.patterns_of(1003)
    hs = O.StringSet.from_lists(pats, 4, True)
    params, split = (1, 5, 1), (8, 3)
    err, ranges, index, slots, found = host_rank_split(f, r, hs, params, split)
    stats = S.expected(1003, params, split)[1]
    assert err == 0 and found == len(slots) and stats["duplicates"] > 0
    # one short of the final count: the error of its own, nothing past the capacity, a number that suffices
    err2, _, _, _, reported = host_rank_split(f, r, hs, params, split, capacity=found - 1)
    assert err2 == _lib.ERROR_CAPACITY and reported >= found
    assert reported == found + stats["duplicates"]               # every span once for every way it was found
    err3, ranges3, index3, slots3, found3 = host_rank_split(f, r, hs, params, split, capacity=reported)
    assert err3 == 0 and found3 == found and (ranges3 == ranges).all() and (index3 == index).all() and (slots3 == slots).all()
    # one short of the reported number is refused as well: the spans are staged before duplicates go
    assert host_rank_split(f, r, hs, params, split, capacity=reported - 1)[0] == _lib.ERROR_CAPACITY


def test_fixed_length_empty_batch_and_refusals():
    L = nvbio_amd.lib()
    t, f, r = M.indices_of(1003)
    pats = [M.patterns_of(1003)[2], t[100:119].copy(), t[-19:].copy()]
    hs = O.StringSet.from_lists(pats, 2, False)
    a = host_rank_split(f, r, hs, (1, M.NO_MAX, 1), (8, 3))
    b = host_rank_split(f, r, hs, (1, M.NO_MAX, 1), (8, 3), fixed_length=19)          # length == NULL
    assert a[0] == 0 and b[0] == 0 and (a[1] == b[1]).all() and (a[2] == b[2]).all() and len(a[1]) > 3
    fs, rs, ss = H.fm_struct(f), H.fm_struct(r), H.sset(hs)
    index, found = np.full(1, 7, np.uint64), C.c_uint64(9)
    entry = L.nvbio_hip_fm_mem_rank_split_host
    assert entry(C.byref(fs), C.byref(rs), C.byref(ss), 0, 19, 1, 5, 1, 8, 3, None, 0, index.ctypes.data, None, C.byref(found), None, 0) == 0      # n = 0 is legal
    assert int(index[0]) == 0 and found.value == 0
    for dev_entry, tail in ((entry, (None, 0)), (L.nvbio_hip_fm_mem_rank_split, (None, 0, None))):
        args = lambda n, max_len, k: (C.byref(fs), C.byref(rs), C.byref(ss), n, max_len, k, 5, 1, 8, 3, None, 0, index.ctypes.data, None, C.byref(found)) + tail
        assert dev_entry(*args(3, 65536, 1)) == 1
        assert dev_entry(*args(1 << 31, 19, 1)) == 1
        assert dev_entry(*args(3, 19, 0)) == 1
    found.value = 9
    assert entry(C.byref(fs), C.byref(rs), C.byref(ss), 3, 18, 1, 5, 1, 8, 3, None, 0, index.ctypes.data, None, C.byref(found), None, 0) == 1       # a longer string
    assert found.value == 0
    assert L.nvbio_hip_fm_mem_split_temp_bytes(1000, 150, 5000) >= 2 * 1000 * 150 * 12 + 5000 * 16
    assert L.nvbio_hip_fm_mem_split_temp_bytes(1000, 150, 5000) >= L.nvbio_hip_fm_mem_temp_bytes(1000, 150)


def test_records_grow_by_the_reseed_walks():
    """out_records counts the re-seed walks too: more than the plain twin's whenever there is a candidate, equal when there is none"""
    t, f, r = M.indices_of(1003)
    hs = O.StringSet.from_lists(M.patterns_of(1003), 4, True)
    plain = H.host_rank(f, r, hs, (1, M.NO_MAX, 1), want_records=True)[5]
    assert host_rank_split(f, r, hs, (1, M.NO_MAX, 1), (8, 3), want_records=True)[5] > plain
    assert host_rank_split(f, r, hs, (1, M.NO_MAX, 1), (4000, 3), want_records=True)[5] == plain         # no MEM is that long


@pytest.mark.parametrize("n_text", S.TEXTS)
def test_locate_over_a_cut_of_the_result(n_text):
    t, f, r = M.indices_of(n_text)
    params, split = (1, 5, 1), (8, 3)
    pats, exp = M.patterns_of(n_text), S.expected(n_text, params, split)[0]
    hs = O.StringSet.from_lists(pats, 4, True)
    err, ranges, index, slots, found = host_rank_split(f, r, hs, params, split)
    assert err == 0
    total = int(slots[-1])
    hits = H.host_locate(f, ranges, slots, 0, total)
    at = 0
    for i, p in enumerate(pats):
        for b, e, occ in exp[i]:
            mine = hits[at:at + len(occ)]
            assert (mine[:, 1] == i).all() and (mine[:, 2] == b).all() and (mine[:, 3] == e).all()
            assert sorted(int(v) for v in mine[:, 0]) == occ
            at += len(occ)
    assert at == total
    for begin, end in ((1, total - 1), (total // 3, total // 3 + 2)):
        assert (H.host_locate(f, ranges, slots, begin, end) == hits[begin:end]).all()
