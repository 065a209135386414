"""The drop-in layer's nvbio/sufsort/sufsort.h through tests/compat/sufsort_callers.hip: cuda::suffix_sort, cuda::bwt and
cuda::find_primary on a packed device string equal the Python layer's results, in the reference's output convention:

  * cuda::suffix_sort writes string_len + 1 entries and emits the '$' row: output[0] = string_len, the sorted suffixes from output + 1
    on (nvbio/sufsort/sufsort_inl.h:155-162);
  * cuda::bwt writes string_len symbols: the symbol of the empty suffix's row first (sufsort_utils.h:330-331), nothing at the primary
    -- the '$' is removed and the symbols after it are shifted back (sufsort_inl.h:262-263, sufsort_utils.h:412-419) -- and returns the
    primary counted with the empty suffix's row ("+1u for the implicit empty suffix", sufsort_utils.h:358);
  * cuda::find_primary returns the same number (sufsort_inl.h:65-74: the suffixes smaller than suffix 0, + 1)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import nvbio_amd as nvb
from oracle import pyoracle as O
from tests import sufsort_texts as T

pytestmark = pytest.mark.gpu

LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "compat", "libsufsort_callers.so")

TEXTS = [(i, t) for i, t in T.small_texts() + T.structured_texts()
         if i in ("iid1", "iid17", "allT33", "iid129", "allA4097", "unit301x17", "fib5779", "primary_first", "primary_last")]


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "build with python -c 'import __graft_entry__ as g; g.build()'"
    L = C.CDLL(LIB)
    vp, u32 = C.c_void_p, C.c_uint32
    L.compat_sufsort.argtypes = [vp, u32, vp, vp, C.POINTER(u32), C.POINTER(u32)]
    L.compat_sufsort_generic.argtypes = [vp, u32, u32, vp, vp, vp, C.POINTER(u32)]
    return L


def _p(a):
    return C.c_void_p(a.ctypes.data)


@pytest.mark.parametrize("text", [t for _, t in TEXTS], ids=[i for i, _ in TEXTS])
def test_packed_device_string(cuda, lib, text):
    n = len(text)
    words = T.pack(text, True)
    sa = np.empty(n + 1, dtype=np.uint32)
    bwt_words = np.empty(words.size, dtype=np.uint32)
    primary, found = C.c_uint32(0), C.c_uint32(0)
    assert lib.compat_sufsort(_p(words), n, _p(sa), _p(bwt_words), C.byref(primary), C.byref(found)) == 0
    d_text = torch.from_numpy(text).to(cuda)
    py_words, py_primary, _, py_sa = nvb.bwt(d_text, keep_sa=True)
    assert (sa == py_sa.cpu().numpy().view(np.uint32)).all() and sa[0] == n
    assert primary.value == py_primary == found.value
    assert (O.unpack(bwt_words, 0, n, 2, True) == O.unpack(py_words.cpu().numpy().view(np.uint32), 0, n, 2, True)).all()
    host = O.FMIndex(text)
    assert (sa == host.sa).all() and primary.value == host.primary and (O.unpack(bwt_words, 0, n, 2, True) == host.bwt).all()


@pytest.mark.parametrize("skip", [0, 5, 16])
@pytest.mark.parametrize("name", ["iid129", "unit301x17"])
def test_generic_iterators(cuda, lib, name, skip):
    """a little-endian string `skip` symbols into its words (in place only when that is a word boundary), a 64-bit suffix array, the
    BWT as bytes and into a packed stream that starts 3 symbols into a word"""
    text = dict(TEXTS)[name]
    n = len(text)
    lead = np.random.default_rng(skip).integers(0, 4, skip, dtype=np.uint8)
    words = T.pack(np.concatenate([lead, text]), False)
    sa = np.empty(n + 1, dtype=np.uint64)
    bwt = np.empty(n, dtype=np.uint8)
    words3 = np.empty((3 + n + 15) // 16, dtype=np.uint32)
    primary = C.c_uint32(0)
    assert lib.compat_sufsort_generic(_p(words), skip, n, _p(sa), _p(bwt), _p(words3), C.byref(primary)) == 0
    host = O.FMIndex(text)
    assert (sa == host.sa).all() and primary.value == host.primary and (bwt == host.bwt).all()
    sym3 = O.unpack(words3, 0, words3.size * 16, 2, True)
    assert (sym3[:3] == 3).all() and (sym3[3:3 + n] == host.bwt).all() and (sym3[3 + n:] == 3).all()      # nothing outside [3, 3 + n) was touched
