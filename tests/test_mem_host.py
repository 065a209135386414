"""MEM seeding on the CPU: the `_host` twins of nvbio_hip_fm_extend / nvbio_hip_fm_mem_rank / nvbio_hip_fm_mem_locate against the
two models of tests/mem_reference.py -- the definition by brute force, and the corrected bidirectional walk over the oracle."""
import ctypes as C

import numpy as np
import pytest

import nvbio_amd
from nvbio_amd import _lib
from oracle import pyoracle as O
from tests import mem_reference as M

TEXTS = [77, 1003, 20000]
FORMATS = [(4, True), (4, False), (2, True), (2, False)]       # (bits, big endian)


def fm_struct(host):
    f = _lib.FMIndexStruct()
    f.length, f.primary, f.sa_int = host.length, host.primary, host.sa_int
    for i in range(5):
        f.L2[i] = int(host.L2[i])
    f.bwt_occ, f.ssa = host.bwt_occ.ctypes.data, host.ssa.ctypes.data
    return f


def sset(hs, fixed_length=0):
    s = _lib.StringSetStruct()
    s.words, s.n_words, s.bits, s.big_endian = hs.words.ctypes.data, hs.words.size, hs.bits, hs.big_endian
    s.begin, s.length, s.fixed_length = hs.begin.ctypes.data, (None if fixed_length else hs.length.ctypes.data), fixed_length
    return s


def host_rank(f, r, hs, params, capacity=None, fixed_length=0, want_records=False):
    """-> (error, ranges [k, 4], index [n + 1], slots [k], number found)"""
    L = nvbio_amd.lib()
    n = len(hs)
    max_len = fixed_length or (int(hs.length.max()) if n else 0)
    cap = int(hs.length.sum()) if capacity is None else capacity
    ranges = np.full((max(cap, 1), 4), 0xDEADBEEF, np.uint32)
    slots = np.full(max(cap, 1), 0xDEADBEEF, np.uint64)
    index = np.zeros(n + 1, np.uint64)
    found, records = C.c_uint64(0), C.c_uint64(0)
    fs, rs, ss = fm_struct(f), fm_struct(r), sset(hs, fixed_length)
    err = L.nvbio_hip_fm_mem_rank_host(C.byref(fs), C.byref(rs), C.byref(ss), n, max_len, params[0], params[1], params[2],
                                       ranges.ctypes.data, cap, index.ctypes.data, slots.ctypes.data, C.byref(found), C.byref(records), 2)
    k = min(int(found.value), cap)
    assert (ranges[k:] == 0xDEADBEEF).all() and (slots[k:] == 0xDEADBEEF).all()        # nothing past what was found, or past the capacity
    if want_records:
        return err, ranges[:k], index, slots[:k], int(found.value), int(records.value)
    return err, ranges[:k], index, slots[:k], int(found.value)


def host_locate(f, ranges, slots, begin, end):
    hits = np.zeros((end - begin, 4), np.uint32)
    fs = fm_struct(f)
    assert nvbio_amd.lib().nvbio_hip_fm_mem_locate_host(C.byref(fs), ranges.ctypes.data, slots.ctypes.data, len(slots), begin, end, hits.ctypes.data, 2) == 0
    return hits


def check_against_models(n_text, params, ranges, index, slots, pats, exp, f, r, bidir=True):
    """the rank table of `pats` equals model (a)'s spans and, through match(), its SA ranges; model (b) agrees"""
    assert int(index[0]) == 0 and int(index[-1]) == len(slots)
    total = 0
    for i, p in enumerate(pats):
        got = ranges[int(index[i]):int(index[i + 1])]
        assert [(int(g[3]) & 0xFFFF, int(g[3]) >> 16) for g in got] == [(b, e) for b, e, _ in exp[i]], (i, params)
        assert (got[:, 2] == i).all()                                           # string id, group flag clear
        assert [int(g[1]) - int(g[0]) + 1 for g in got] == [len(o) for _, _, o in exp[i]]
        if len(got):
            subs = O.StringSet.from_lists([p[b:e] for b, e, _ in exp[i]], 4, True)
            assert (got[:, :2] == f.match(subs)).all()                          # the range nvbio_hip_fm_match gives the substring
        if bidir:
            walk, recorded = M.bidir_mems(f, r, p, *params)
            assert [tuple(int(v) for v in (g[3] & 0xFFFF, g[3] >> 16, g[0], g[1])) for g in got] == walk
            assert recorded <= len(p)
        total += sum(len(o) for _, _, o in exp[i])
    assert (slots == np.cumsum(ranges[:, 1].astype(np.uint64) - ranges[:, 0] + 1)).all()
    return total


@pytest.mark.parametrize("n_text", TEXTS)
@pytest.mark.parametrize("params", M.PARAMS)
def test_rank_host_equals_both_models(n_text, params):
    t, f, r = M.indices_of(n_text)
    for bits, be in FORMATS:
        pats = M.patterns_of(n_text, with_n=bits == 4)
        exp = M.expected(n_text, params, with_n=bits == 4)
        hs = O.StringSet.from_lists(pats, bits, be)
        err, ranges, index, slots, found = host_rank(f, r, hs, params)
        assert err == 0 and found == len(slots)
        check_against_models(n_text, params, ranges, index, slots, pats, exp, f, r, bidir=(bits, be) == (4, True))
    if params == M.PARAMS[0]:
        assert found > len(pats)                    # the cases do produce MEMs, several a string


@pytest.mark.parametrize("n_text", TEXTS)
def test_locate_host_gives_exactly_the_occurrences(n_text):
    t, f, r = M.indices_of(n_text)
    params = (1, 5, 1) if n_text == 20000 else M.PARAMS[0]        # every occurrence of a symbol in 20 000 is more than the point needs
    pats, exp = M.patterns_of(n_text), M.expected(n_text, params)
    hs = O.StringSet.from_lists(pats, 4, True)
    err, ranges, index, slots, found = host_rank(f, r, hs, params)
    assert err == 0
    total = int(slots[-1])
    hits = host_locate(f, ranges, slots, 0, total)
    at = 0
    for i, p in enumerate(pats):
        for b, e, occ in exp[i]:
            mine = hits[at:at + len(occ)]
            assert (mine[:, 1] == i).all() and (mine[:, 2] == b).all() and (mine[:, 3] == e).all()
            assert sorted(int(v) for v in mine[:, 0]) == occ
            for pos in mine[:, 0]:
                assert (t[int(pos):int(pos) + e - b] == p[b:e]).all()
            at += len(occ)
    assert at == total
    # sub-ranges that cut a MEM's rows, and the first hit of every string
    for begin, end in ((1, total - 1), (total // 3, total // 3 + 2), (total // 2, total // 2)):
        if 0 <= begin <= end <= total:
            assert (host_locate(f, ranges, slots, begin, end) == hits[begin:end]).all()


def test_capacity_one_short_reports_the_true_count_and_stores_nothing_past_it():
    t, f, r = M.indices_of(1003)
    pats = M.patterns_of(1003)
    hs = O.StringSet.from_lists(pats, 4, True)
    err, ranges, index, slots, found = host_rank(f, r, hs, M.PARAMS[0])
    assert err == 0
    err2, ranges2, index2, slots2, found2 = host_rank(f, r, hs, M.PARAMS[0], capacity=found - 1)
    assert err2 == _lib.ERROR_CAPACITY and found2 == found and len(slots2) == found - 1
    assert (ranges2 == ranges[:-1]).all() and (slots2 == slots[:-1]).all() and (index2 == index).all()
    err3, ranges3, _, _, found3 = host_rank(f, r, hs, M.PARAMS[0], capacity=found)
    assert err3 == 0 and (ranges3 == ranges).all()


def test_fixed_length_empty_batch_and_refusals():
    L = nvbio_amd.lib()
    t, f, r = M.indices_of(1003)
    pats = [p for p in (M.patterns_of(1003)[2], t[100:119].copy(), t[-19:].copy())]
    assert all(len(p) == 19 for p in pats)
    hs = O.StringSet.from_lists(pats, 2, False)
    a = host_rank(f, r, hs, M.PARAMS[0])
    b = host_rank(f, r, hs, M.PARAMS[0], fixed_length=19)           # length == NULL
    assert a[0] == 0 and b[0] == 0 and (a[1] == b[1]).all() and (a[2] == b[2]).all()
    # n = 0 is legal
    fs, rs, ss = fm_struct(f), fm_struct(r), sset(hs)
    index, found = np.full(1, 7, np.uint64), C.c_uint64(9)
    assert L.nvbio_hip_fm_mem_rank_host(C.byref(fs), C.byref(rs), C.byref(ss), 0, 19, 1, 5, 1, None, 0, index.ctypes.data, None, C.byref(found), None, 0) == 0
    assert int(index[0]) == 0 and found.value == 0
    assert L.nvbio_hip_fm_mem_rank(C.byref(fs), C.byref(rs), None, 0, 0, 1, 5, 1, None, 0, None, None, C.byref(found), None, 0, None) == 1     # no index array
    # argument errors, before anything runs: patterns of more than 65 535 symbols, 2^31 strings, min_intv 0, indices of two lengths
    for entry, tail in ((L.nvbio_hip_fm_mem_rank_host, (None, 0)), (L.nvbio_hip_fm_mem_rank, (None, 0, None))):
        args = lambda n, max_len, k: (C.byref(fs), C.byref(rs), C.byref(ss), n, max_len, k, 5, 1, None, 0, index.ctypes.data, None, C.byref(found)) + tail
        assert entry(*args(3, 65536, 1)) == 1
        assert entry(*args(1 << 31, 19, 1)) == 1
        assert entry(*args(3, 19, 0)) == 1
    # a length array that holds a string longer than max_pattern_len is refused too, and nothing is counted
    found.value = 9
    assert L.nvbio_hip_fm_mem_rank_host(C.byref(fs), C.byref(rs), C.byref(ss), 3, 18, 1, 5, 1, None, 0, index.ctypes.data, None, C.byref(found), None, 0) == 1
    assert found.value == 0
    short = fm_struct(M.indices_of(77)[1])
    assert L.nvbio_hip_fm_mem_rank_host(C.byref(fs), C.byref(short), C.byref(ss), 3, 19, 1, 5, 1, None, 0, index.ctypes.data, None, C.byref(found), None, 0) == 1
    assert L.nvbio_hip_fm_mem_temp_bytes(1000, 150) >= 1000 * 150 * 12
    assert L.nvbio_hip_fm_mem_locate(C.byref(fs), None, None, 0, 0, 5, None, None) == 1
    assert L.nvbio_hip_fm_extend(2, C.byref(fs), C.byref(rs), None, None, None, 0, None, None, None) == 1
    assert L.nvbio_hip_fm_extend(0, C.byref(fs), C.byref(rs), None, None, None, 0, None, None, None) == 0


def host_extend(direction, f, r, f_ranges, r_ranges, c):
    fs, rs = fm_struct(f), fm_struct(r)
    n = len(c)
    fr, rr = np.ascontiguousarray(f_ranges, np.uint32), np.ascontiguousarray(r_ranges, np.uint32)
    cc = np.ascontiguousarray(c, np.uint8)
    of, orr = np.zeros((n, 2), np.uint32), np.zeros((n, 2), np.uint32)
    assert nvbio_amd.lib().nvbio_hip_fm_extend_host(direction, C.byref(fs), C.byref(rs), fr.ctypes.data, rr.ctypes.data, cc.ctypes.data, n,
                                                    of.ctypes.data, orr.ctypes.data, 2) == 0
    return of, orr


def extend_strings(n_text):
    """strings to grow symbol by symbol: from the empty string; a suffix and a prefix of the text (the primary rows); one that dies"""
    t = M.text_of(n_text)
    rng = np.random.default_rng(5)
    out = [t[-12:].copy(), t[:12].copy(), t[n_text // 2:n_text // 2 + 25].copy(), rng.integers(0, 4, 14, dtype=np.uint8)]
    if n_text == 77:
        out.append(t.copy())
    return out


@pytest.mark.parametrize("n_text", TEXTS)
def test_extend_host_ranges_equal_match_of_the_extended_string(n_text):
    t, f, r = M.indices_of(n_text)
    for s in extend_strings(n_text):
        # forward: P -> Pc, from the empty string
        fr, rr = np.array([[0, f.length]], np.uint32), np.array([[0, r.length]], np.uint32)
        model = ((0, f.length), (0, r.length))
        for i in range(len(s)):
            fr, rr = host_extend(0, f, r, fr, rr, s[i:i + 1])
            want_f = f.match(O.StringSet.from_lists([s[:i + 1]], 4, True))
            want_r = r.match(O.StringSet.from_lists([s[:i + 1][::-1]], 4, True))
            if want_f[0, 0] > want_f[0, 1]:                 # emptied: both are empty, and stay so
                assert fr[0, 0] == fr[0, 1] + 1 and rr[0, 0] == rr[0, 1] + 1
                break
            assert (fr == want_f).all() and (rr == want_r).all(), (n_text, i)
            model = M.extend_forward(f, r, model[0], model[1], int(s[i]))          # model (b)'s step agrees too
            assert [tuple(int(v) for v in fr[0]), tuple(int(v) for v in rr[0])] == list(model)
        # backwards: P -> cP, from the empty string
        fr, rr = np.array([[0, f.length]], np.uint32), np.array([[0, r.length]], np.uint32)
        for i in range(len(s) - 1, -1, -1):
            fr, rr = host_extend(1, f, r, fr, rr, s[i:i + 1])
            want_f = f.match(O.StringSet.from_lists([s[i:]], 4, True))
            want_r = r.match(O.StringSet.from_lists([s[i:][::-1]], 4, True))
            if want_f[0, 0] > want_f[0, 1]:
                assert fr[0, 0] == fr[0, 1] + 1 and rr[0, 0] == rr[0, 1] + 1
                break
            assert (fr == want_f).all() and (rr == want_r).all(), (n_text, i)
    # a symbol past the alphabet empties both
    of, orr = host_extend(0, f, r, [[0, f.length]], [[0, r.length]], [4])
    assert (of == [[1, 0]]).all() and (orr == [[1, 0]]).all()


def records_of_step(index, rng):
    """32-byte records a step from the range reads: one per end of (x - 1, y) that is a BWT row, one when both share a 64-symbol block"""
    ks = []
    for k in ((rng[0] - 1) & 0xFFFFFFFF, rng[1]):
        if k in (0xFFFFFFFF, index.length):
            continue
        k -= 1 if k >= index.primary else 0
        if k >= 0:
            ks.append(k >> 6)
    return len(set(ks))


def test_records_counted_by_the_host_twin():
    """A^150 over the run walks right once, 150 steps on the reverse index, and never left: the twin counts the records of those steps"""
    t, f, r = M.indices_of(20000)
    hs = O.StringSet.from_lists([np.zeros(150, np.uint8)], 2, True)
    err, ranges, index, slots, found, records = host_rank(f, r, hs, M.PARAMS[0], want_records=True)
    want, fr, rr = 0, (0, f.length), (0, r.length)
    for _ in range(150):
        want += records_of_step(r, rr)
        fr, rr = M.extend_forward(f, r, fr, rr, 0)
    assert err == 0 and found == 1 and records == want and 150 <= want <= 300
    assert (int(ranges[0, 3]) & 0xFFFF, int(ranges[0, 3]) >> 16) == (0, 150) and int(ranges[0, 1]) - int(ranges[0, 0]) + 1 == 300 - 150 + 1
