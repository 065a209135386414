"""The `_host` twins of the byte-alphabet entries (suffix sort and BWT of a byte text, the wavelet tree, the FM-index over it), through the
Python layer on device="cpu" and directly, against the definitions in plain numpy (tests/wavelet_reference.py); the argument checks of
the device entries and the twins -- no GPU needed.  The checks themselves are in tests/wavelet_checks.py, and tests/test_wavelet_gpu.py
runs them again on the GPU."""
import ctypes as C

import numpy as np
import pytest

import nvbio_amd as nvb
from nvbio_amd import _lib
from tests import wavelet_cases as WC
from tests import wavelet_reference as R
from tests.wavelet_checks import check_tree, check_known_ranks, check_fm, check_fm_against_oracle, check_protein_example

INVALID = 1      # hipErrorInvalidValue
F = 0xDEADBEEF


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


@pytest.mark.parametrize("case_id", [c.id for c in WC.tree_cases()])
def test_tree(case_id):
    check_tree(case_id, "cpu")


def test_known_ranks_of_the_reference():
    check_known_ranks("cpu")


@pytest.mark.parametrize("case_id", [c.id for c in WC.fm_cases()])
def test_fm_index(case_id):
    check_fm(case_id, "cpu")


def test_fm_index_equals_the_2bit_oracle():
    check_fm_against_oracle("cpu")


def test_protein_example():
    check_protein_example("cpu")


def test_protein_alphabet():
    sym = nvb.alphabet.encode(WC.PROTEIN_TEXT)
    assert sym.tolist() == list(range(24)) and nvb.alphabet.decode(sym) == WC.PROTEIN_TEXT
    assert nvb.alphabet.encode("J?").tolist() == [23, 23] and nvb.alphabet.decode([24, 255]) == "XX"


def test_header_and_binding_agree_on_names_with_capitals():
    """tests/test_abi.py reads lower-case names; this reads every declared name and wants SYMBOLS + CAPITAL_SYMBOLS to be exactly those"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "nvbio_hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(nvbio_hip_[A-Za-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_lib.SYMBOLS + _lib.CAPITAL_SYMBOLS)
    L = C.CDLL(nvb.LIB_PATH)
    for s in _lib.CAPITAL_SYMBOLS:
        assert hasattr(L, s), s


def test_twin_called_directly():
    """the twins through ctypes, no Python layer: setup, rank, L2, match and locate of the protein text"""
    L = nvb.lib()
    text = nvb.alphabet.encode(WC.PROTEIN_TEXT)
    n, S, K = text.size, 8, 256
    sa = R.suffix_array(text, S)
    bwt = np.zeros(n, dtype=np.uint8)
    primary = C.c_uint32(0)
    ssa = np.zeros((n + 4) // 4, dtype=np.uint32)
    assert L.nvbio_hip_bwt_bytes_host(_p(text), S, n, 4, _p(bwt), C.byref(primary), _p(ssa), None, 1) == 0
    ebwt, eprimary = R.bwt(text, S, sa)
    assert (bwt == ebwt).all() and primary.value == eprimary and (ssa == R.ssa(sa, 4)).all()
    W = (n * S + 31) // 32
    bits, splits, occ = np.zeros(W, dtype=np.uint32), np.zeros(K, dtype=np.uint32), np.zeros(K + W, dtype=np.uint32)
    assert L.nvbio_hip_wavelet_setup_host(_p(bwt), S, n, _p(bits), _p(splits), _p(occ), 1) == 0
    eb, es, eo = R.tree_arrays(bwt, S)
    assert (bits == eb).all() and (splits == es).all() and (occ == eo).all()
    t = _lib.WaveletTreeStruct(bits.ctypes.data, splits.ctypes.data, occ.ctypes.data, S, n)
    L2 = np.zeros(K + 1, dtype=np.uint32)
    assert L.nvbio_hip_wavelet_fm_L2_host(C.byref(t), _p(L2), 1) == 0 and (L2 == R.L2(text, S)).all()
    f = _lib.WaveletFMIndexStruct(t, L2.ctypes.data, ssa.ctypes.data, n, primary.value, 4, 0)
    begin = np.arange(n, dtype=np.uint64)
    length = (n - np.arange(n)).astype(np.uint32)
    ps = _lib.ByteStringSetStruct(text.ctypes.data, n, begin.ctypes.data, length.ctypes.data, 0, 0)
    ranges = np.zeros((n, 2), dtype=np.uint32)
    assert L.nvbio_hip_wavelet_fm_match_host(C.byref(f), C.byref(ps), n, _p(ranges), 1) == 0
    assert (ranges[:, 0] == ranges[:, 1]).all()
    pos = np.zeros(n, dtype=np.uint32)
    assert L.nvbio_hip_wavelet_fm_locate_host(C.byref(f), _p(np.ascontiguousarray(ranges[:, 0])), n, _p(pos), 1) == 0
    assert (pos == np.arange(n)).all()
    # a fixed-length set that runs past the symbols it declares is clipped, not read
    ps2 = _lib.ByteStringSetStruct(text.ctypes.data, n, begin.ctypes.data, None, 5, 0)
    assert L.nvbio_hip_wavelet_fm_match_host(C.byref(f), C.byref(ps2), n, _p(ranges), 1) == 0
    assert (ranges[:, 0] == ranges[:, 1]).all()


def test_python_layer_raises_value_error():
    text = np.arange(10, dtype=np.uint8)
    for S in (0, 9):
        with pytest.raises(ValueError):
            nvb.WaveletTree.build(text, S, device="cpu")
        with pytest.raises(ValueError):
            nvb.suffix_sort_bytes(text, S, device="cpu")
        with pytest.raises(ValueError):
            nvb.bwt_bytes(text, S, device="cpu")
    with pytest.raises(ValueError):
        nvb.WaveletTree.build(np.zeros(0, dtype=np.uint8), 8, device="cpu")
    with pytest.raises(ValueError):
        nvb.WaveletTree.build(np.zeros(4, dtype=np.int32), 8, device="cpu")
    with pytest.raises(ValueError):
        nvb.bwt_bytes(text, 8, sa_int=0, device="cpu")
    tree = nvb.WaveletTree.build(text, 8, device="cpu")
    with pytest.raises(ValueError):
        tree.rank([1, 2], [1])
    fmi = nvb.WaveletFMIndex.build(text, 8, 4, device="cpu")
    fmi.ssa = None
    with pytest.raises(ValueError):
        fmi.locate([1])


def test_invalid_arguments_are_rejected_with_the_outputs_untouched():
    """a null pointer, symbol_size 0 and 9, n = 0, n S over the limit, temp one byte short, ssa == NULL for locate: hipErrorInvalidValue
    from the device entries (before anything is launched, so host arrays stand in for device memory) and from the host twins, and no
    output word changes"""
    L = nvb.lib()
    n, S, K = 100, 5, 32
    W = (n * S + 31) // 32
    text = np.random.default_rng(5).integers(0, 24, n, dtype=np.uint8)
    outs = dict(sa=np.full(n + 1, F, dtype=np.uint32), bwt=np.full(n, 0xEF, dtype=np.uint8), ssa=np.full(n + 1, F, dtype=np.uint32),
                bits=np.full(W, F, dtype=np.uint32), splits=np.full(K, F, dtype=np.uint32), occ=np.full(K + W, F, dtype=np.uint32),
                out=np.full(2 * n, F, dtype=np.uint32), out8=np.full(n, 0xEF, dtype=np.uint8), L2=np.full(K + 1, F, dtype=np.uint32))
    primary = C.c_uint32(F)
    temp = np.zeros(16, dtype=np.uint8)
    big = 1 << 40
    over = 0xFFFFFFFF // S + 1                                        # n S over the tree's limit
    over_sort = 0xFFFFFFFF                                            # n over the sorter's limit

    def untouched():
        return all((a == (0xEF if a.dtype == np.uint8 else F)).all() for a in outs.values()) and primary.value == F

    def sort(text=text, S=S, n=n, sa=outs["sa"], temp=temp, tb=big, host=False):
        if host:
            return L.nvbio_hip_suffix_sort_bytes_host(_p(text), S, n, _p(sa), 1)
        return L.nvbio_hip_suffix_sort_bytes(_p(text), S, n, _p(sa), _p(temp), tb, None)

    def bwt(text=text, S=S, n=n, sa_int=4, bwt=outs["bwt"], prim=primary, ssa=outs["ssa"], temp=temp, tb=big, host=False):
        pp = C.byref(prim) if prim is not None else None
        if host:
            return L.nvbio_hip_bwt_bytes_host(_p(text), S, n, sa_int, _p(bwt), pp, _p(ssa), _p(outs["sa"]), 1)
        return L.nvbio_hip_bwt_bytes(_p(text), S, n, sa_int, _p(bwt), pp, _p(ssa), _p(outs["sa"]), _p(temp), tb, None)

    def setup(text=text, S=S, n=n, bits=outs["bits"], splits=outs["splits"], occ=outs["occ"], temp=temp, tb=big, host=False):
        if host:
            return L.nvbio_hip_wavelet_setup_host(_p(text), S, n, _p(bits), _p(splits), _p(occ), 1)
        return L.nvbio_hip_wavelet_setup(_p(text), S, n, _p(bits), _p(splits), _p(occ), _p(temp), tb, None)

    for host in (False, True):
        for f in (sort, bwt, setup):
            assert f(S=0, host=host) == INVALID and f(S=9, host=host) == INVALID and f(n=0, host=host) == INVALID and f(text=None, host=host) == INVALID
        assert sort(n=over_sort, host=host) == INVALID and bwt(n=over_sort, host=host) == INVALID and setup(n=over, host=host) == INVALID
        assert sort(sa=None, host=host) == INVALID
        assert bwt(bwt=None, host=host) == INVALID and bwt(prim=None, host=host) == INVALID and bwt(sa_int=0, host=host) == INVALID
        assert setup(bits=None, host=host) == INVALID and setup(splits=None, host=host) == INVALID and setup(occ=None, host=host) == INVALID
        assert untouched()
    for f, tb in ((sort, L.nvbio_hip_suffix_sort_bytes_temp_bytes(n)), (bwt, L.nvbio_hip_bwt_bytes_temp_bytes(n)), (setup, L.nvbio_hip_wavelet_setup_temp_bytes(n, S))):
        assert tb >= n
        assert f(temp=None) == INVALID and f(tb=tb - 1) == INVALID and untouched()

    # the queries, on a tree that is valid but for the one field changed
    bits, splits, occ = R.tree_arrays(text, S)
    sa = R.suffix_array(text, S)
    good = _lib.WaveletTreeStruct(bits.ctypes.data, splits.ctypes.data, occ.ctypes.data, S, n)
    pos = np.arange(n, dtype=np.uint32)
    sym = text.copy()

    def tree(**kw):
        t = _lib.WaveletTreeStruct.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    bad_trees = [tree(bits=None), tree(splits=None), tree(occ=None), tree(symbol_size=0), tree(symbol_size=9), tree(size=0), tree(size=over)]
    L2 = R.L2(text, S)
    ssa = R.ssa(sa, 4)
    begin, length = np.array([0, 10], dtype=np.uint64), np.array([10, 10], dtype=np.uint32)
    ps = _lib.ByteStringSetStruct(text.ctypes.data, n, begin.ctypes.data, length.ctypes.data, 0, 0)

    def fmi(t=good, L2=L2, ssa=ssa, length=n, primary=3, sa_int=4):
        return _lib.WaveletFMIndexStruct(t, None if L2 is None else L2.ctypes.data, None if ssa is None else ssa.ctypes.data, length, primary, sa_int, 0)

    bad_fmis = [fmi(t=t) for t in bad_trees] + [fmi(L2=None), fmi(length=n - 1), fmi(primary=0), fmi(primary=n + 1)]
    for suffix, last in (("", None), ("_host", 1)):
        text_f, rank_f = getattr(L, "nvbio_hip_wavelet_text" + suffix), getattr(L, "nvbio_hip_wavelet_rank" + suffix)
        range_f, L2_f = getattr(L, "nvbio_hip_wavelet_rank_range" + suffix), getattr(L, "nvbio_hip_wavelet_fm_L2" + suffix)
        match_f, locate_f = getattr(L, "nvbio_hip_wavelet_fm_match" + suffix), getattr(L, "nvbio_hip_wavelet_fm_locate" + suffix)
        for t in bad_trees + [None]:
            tp = C.byref(t) if t is not None else None
            assert text_f(tp, _p(pos), n, _p(outs["out8"]), last) == INVALID
            assert rank_f(tp, _p(pos), _p(sym), n, _p(outs["out"]), last) == INVALID
            assert range_f(tp, _p(pos), _p(sym), n // 2, _p(outs["out"]), last) == INVALID
            assert L2_f(tp, _p(outs["L2"]), last) == INVALID
        g = C.byref(good)
        assert text_f(g, _p(pos), n, None, last) == INVALID
        assert rank_f(g, None, _p(sym), n, _p(outs["out"]), last) == INVALID and rank_f(g, _p(pos), None, n, _p(outs["out"]), last) == INVALID
        assert rank_f(g, _p(pos), _p(sym), n, None, last) == INVALID and rank_f(g, _p(pos), _p(sym), 1 << 32, _p(outs["out"]), last) == INVALID
        assert range_f(g, None, _p(sym), 2, _p(outs["out"]), last) == INVALID and range_f(g, _p(pos), _p(sym), 2, None, last) == INVALID
        assert L2_f(g, None, last) == INVALID
        for f in bad_fmis + [None]:
            fp = C.byref(f) if f is not None else None
            assert match_f(fp, C.byref(ps), 2, _p(outs["out"]), last) == INVALID
            assert locate_f(fp, _p(pos), n, _p(outs["out"]), last) == INVALID
        ok = fmi()
        assert match_f(C.byref(ok), None, 2, _p(outs["out"]), last) == INVALID and match_f(C.byref(ok), C.byref(ps), 2, None, last) == INVALID
        no_begin = _lib.ByteStringSetStruct(text.ctypes.data, n, None, length.ctypes.data, 0, 0)
        assert match_f(C.byref(ok), C.byref(no_begin), 2, _p(outs["out"]), last) == INVALID
        for f in (fmi(ssa=None), fmi(sa_int=0)):
            assert locate_f(C.byref(f), _p(pos), n, _p(outs["out"]), last) == INVALID
        assert locate_f(C.byref(ok), None, n, _p(outs["out"]), last) == INVALID and locate_f(C.byref(ok), _p(pos), n, None, last) == INVALID
        assert untouched()
