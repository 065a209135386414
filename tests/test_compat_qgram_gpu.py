"""The upper layers of the q-gram module on the GPU, against the definitions (tests/qgram_reference.py) and against what the Python layer
returns on the same inputs, byte for byte:
- the drop-in layer (include/nvbio_hip/compat/nvbio/qgram/qgram.h, filter.h) through the caller translation unit
  tests/compat/qgram_callers.hip: an index built from a packed stream (the tuned execution) with a device filter on plain pointers, the
  same index built from 8-bit symbols with the filter forced generic, and the index copied to the host with a host filter;
- the C++ host layer (include/nvbio_hip/qgram.h) through tests/cxx/qgram_shim.cpp."""
import ctypes as C
import os

import numpy as np
import pytest

import nvbio_amd as nvb
from tests import qgram_cases as QC
from tests import qgram_checks as H
from tests import qgram_reference as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PACKED_DEVICE, BYTES_DEVICE_GENERIC, PACKED_HOST = 0, 1, 2


class Outputs(C.Structure):
    _fields_ = [("n_unique", C.c_void_p), ("n_qgrams", C.c_void_p), ("qgrams", C.c_void_p), ("slots", C.c_void_p), ("index", C.c_void_p), ("lut", C.c_void_p),
                ("ranges", C.c_void_p), ("total", C.c_void_p), ("hits_capacity", C.c_uint64), ("hits", C.c_void_p), ("n_merged", C.c_void_p),
                ("merged", C.c_void_p), ("counts", C.c_void_p)]


def p(x):
    return C.c_void_p(x.ctypes.data) if x is not None else None


def call(fn, args_before, args_after, is_set, ql, n_queries, capacity, n_max):
    """run one C entry point that fills an Outputs -> dict of numpy arrays, cut to what it reported"""
    w = 2 if is_set else 1
    a = dict(n_unique=np.zeros(1, np.uint32), n_qgrams=np.zeros(1, np.uint32), qgrams=np.zeros(n_max + 1, np.uint64), slots=np.zeros(n_max + 1, np.uint32),
             index=np.zeros(w * n_max + 1, np.uint32), lut=np.zeros(4 ** ql + 1, np.uint32), ranges=np.zeros(2 * n_queries, np.uint32),
             total=np.zeros(1, np.uint64), hits=np.zeros(2 * w * capacity + 1, np.uint32), n_merged=np.zeros(1, np.uint32),
             merged=np.zeros(w * capacity + 1, np.uint32), counts=np.zeros(capacity + 1, np.uint32))
    o = Outputs()
    for k, v in a.items():
        setattr(o, k, v.ctypes.data)
    o.hits_capacity = capacity
    assert fn(*args_before, *args_after, C.byref(o)) == 0
    nu, n, total, nm = int(a["n_unique"][0]), int(a["n_qgrams"][0]), int(a["total"][0]), int(a["n_merged"][0])
    return dict(n_unique=nu, n_qgrams=n, qgrams=a["qgrams"][:nu], slots=a["slots"][:nu + 1], index=a["index"][:w * n].reshape((n, 2) if is_set else (n,)),
                lut=a["lut"] if ql else a["lut"][:0], ranges=a["ranges"].reshape(-1, 2), total=total, hits=a["hits"][:2 * w * total].reshape(total, 2 * w),
                merged=a["merged"][:w * nm].reshape((nm, 2) if is_set else (nm,)), counts=a["counts"][:nm])


def check(got, e, ix, queries, indices, merge_interval):
    """against the reference `e` and the Python layer's index `ix`"""
    assert got["n_unique"] == e.n_unique and got["n_qgrams"] == e.n_qgrams
    assert (got["qgrams"] == e.qgrams).all() and (got["slots"] == e.slots).all() and (got["index"] == e.index).all()
    assert (got["lut"] == (e.lut if e.lut is not None else np.zeros(0, np.uint32))).all()
    for x, y in zip((got["qgrams"], got["slots"], got["index"], got["lut"]), H.index_arrays(ix)):
        assert y is None or x.tobytes() == y.tobytes()
    ranges, slots, total = R.rank(e, queries)
    assert (got["ranges"] == ranges).all() and got["total"] == total > 0
    expect = R.locate(e, ranges, slots, indices, 0, total)
    assert (got["hits"] == expect).all()
    em, ec = R.merge(expect, merge_interval)
    assert got["merged"].shape == em.shape and (got["merged"] == em).all() and (got["counts"] == ec).all()
    f = nvb.QGramFilter()
    assert f.rank(ix, queries, indices) == total
    hits = f.locate(0, total)
    merged, counts = f.merge(merge_interval, hits)
    assert H.u32(hits).tobytes() == got["hits"].tobytes() and H.u32(merged).tobytes() == got["merged"].tobytes() and H.u32(counts).tobytes() == got["counts"].tobytes()


def same(a, b):
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def string_inputs(q, ql):
    sym = dict(QC.strings(q))["iid4096"]
    e = R.string_index(sym, q, ql)
    rng = np.random.default_rng(q)
    queries = QC.queries_for(R.string_index(sym, q, 0), rng)
    indices = rng.integers(0, 300, queries.size).astype(np.uint32)
    return sym, e, queries, indices, R.rank(e, queries)[2]


def set_inputs(name, q, ql, interval):
    case = dict((c.id, c) for c in QC.sets())[name]
    e = R.set_index(case.strings, q, interval, ql)
    rng = np.random.default_rng(q)
    queries = QC.queries_for(R.set_index(case.strings, q, interval, 0), rng)
    indices = rng.integers(0, 300, queries.size).astype(np.uint32)
    return case, e, queries, indices, R.rank(e, queries)[2]


# ---- the drop-in layer ----

@pytest.mark.parametrize("big_endian", [True, False], ids=["be", "le"])
@pytest.mark.parametrize("q,ql", [(12, 6), (32, 0), (3, 3), (20, 1)])
def test_callers_string_index_and_filters(cuda, q, ql, big_endian):
    """device and host filters of the caller translation unit equal the Python layer; the 8-bit-symbol (generic) path equals the packed one"""
    lib = C.CDLL(os.path.join(HERE, "compat", "libqgram_callers.so"))
    sym, e, queries, indices, total = string_inputs(q, ql)
    words = H.packed(sym, big_endian, "cpu")[0].numpy().view(np.uint32)
    ix = nvb.QGramIndex.build(H.packed(sym, big_endian, cuda), q, ql)
    got = {}
    for mode in (PACKED_DEVICE, BYTES_DEVICE_GENERIC, PACKED_HOST):
        got[mode] = call(lib.compat_qgram_string, (p(words), words.size, int(big_endian), p(sym), len(sym), q, ql, mode),
                         (p(queries), p(indices), queries.size, 10), False, ql, queries.size, total, len(sym))
        check(got[mode], e, ix, queries, indices, 10)
    same(got[PACKED_DEVICE], got[BYTES_DEVICE_GENERIC])
    same(got[PACKED_DEVICE], got[PACKED_HOST])


@pytest.mark.parametrize("big_endian", [True, False], ids=["be", "le"])
@pytest.mark.parametrize("name,q,ql,interval", [("concatenated_with_empty_and_short", 12, 6, 3), ("same_read_x3", 20, 6, 1), ("concatenated_with_empty_and_short", 31, 0, 10)])
def test_callers_set_index_and_filters(cuda, name, q, ql, interval, big_endian):
    lib = C.CDLL(os.path.join(HERE, "compat", "libqgram_callers.so"))
    case, e, queries, indices, total = set_inputs(name, q, ql, interval)
    lens = np.array([len(t) for t in case.strings], dtype=np.uint64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    assert (offsets[:-1] == case.begin).all()                              # a concatenated set: begin is the running sum
    words = case.words(big_endian)
    ix = nvb.QGramSetIndex.build(H.packed_set(case, big_endian, cuda), q, interval, ql)
    got = {}
    for mode in (PACKED_DEVICE, BYTES_DEVICE_GENERIC, PACKED_HOST):
        got[mode] = call(lib.compat_qgram_set, (p(words), words.size, int(big_endian), p(case.stream), case.stream.size, p(offsets), case.n_strings, q, ql, interval, mode),
                         (p(queries), p(indices), queries.size, 16), True, ql, queries.size, total, e.n_qgrams)
        check(got[mode], e, ix, queries, indices, 16)
    same(got[PACKED_DEVICE], got[BYTES_DEVICE_GENERIC])
    same(got[PACKED_DEVICE], got[PACKED_HOST])


# ---- the C++ host layer ----

@pytest.mark.parametrize("big_endian", [True, False], ids=["be", "le"])
@pytest.mark.parametrize("q,ql", [(12, 6), (32, 0), (3, 3)])
def test_host_layer_string_index_and_filter(cuda, q, ql, big_endian):
    shim = C.CDLL(os.path.join(HERE, "cxx", "libqgram_shim.so"))
    sym, e, queries, indices, total = string_inputs(q, ql)
    words = H.packed(sym, big_endian, "cpu")[0].numpy().view(np.uint32)
    got = call(shim.qgram_host_layer, (p(words), C.c_uint64(words.size), int(big_endian), C.c_uint64(len(sym)), None, None, 0, 0, 0, q, ql, 1),
               (p(queries), p(indices), queries.size, 10), False, ql, queries.size, total, len(sym))
    check(got, e, nvb.QGramIndex.build(H.packed(sym, big_endian, cuda), q, ql), queries, indices, 10)


@pytest.mark.parametrize("big_endian", [True, False], ids=["be", "le"])
@pytest.mark.parametrize("name,q,ql,interval", [("unaligned_out_of_order_overlapping", 12, 6, 3), ("fixed40", 17, 1, 1), ("same_read_x3", 20, 6, 1)])
def test_host_layer_set_index_and_filter(cuda, name, q, ql, interval, big_endian):
    shim = C.CDLL(os.path.join(HERE, "cxx", "libqgram_shim.so"))
    case, e, queries, indices, total = set_inputs(name, q, ql, interval)
    words = case.words(big_endian)
    got = call(shim.qgram_host_layer, (p(words), C.c_uint64(words.size), int(big_endian), C.c_uint64(0), p(case.begin), p(case.length), case.fixed_length,
                                       case.n_strings, 1, q, ql, interval), (p(queries), p(indices), queries.size, 16), True, ql, queries.size, total, e.n_qgrams)
    check(got, e, nvb.QGramSetIndex.build(H.packed_set(case, big_endian, cuda), q, interval, ql), queries, indices, 16)
