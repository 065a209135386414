"""The drop-in layer's string-set overloads of nvbio/sufsort/sufsort.h through tests/compat/set_sufsort_callers.hip:
cuda::suffix_sort(string_set, handler) and cuda::bwt<2, BIG_ENDIAN>(string_set, handler) over a packed-concatenated device set.  What the
handlers are given, batch after batch, equals the C-ABI's arrays and the definition (tests/set_sufsort_reference.py):

  * the suffix handler gets device arrays: the sorted global suffix indices, the string of every index, the cumulative lengths
    (nvbio/sufsort/sufsort.h:207-233);
  * the BWT handler gets host arrays: one byte a row with 255 for '$', and the '$' rows as absolute positions with their string ids,
    both uint64 (nvbio/sufsort/sufsort_utils.h:75-80, sufsort_priv.cu:453-527)."""
import ctypes as C
import os

import numpy as np
import pytest

import nvbio_amd as nvb
from tests import set_sufsort_reference as R
from tests import set_sufsort_sets as S
from tests import sufsort_texts as T

pytestmark = pytest.mark.gpu

LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "compat", "libset_sufsort_callers.so")

NAMES = ("single_iid33", "single_allT65", "only_empty", "empty_A_empty_AA", "same28x2", "same29x3", "same30x2", "same100x3", "prefixes_and_suffixes",
         "allA27to31", "allT28to30", "short_iid")
CASES = [c for c in S.all_small() if c.id in NAMES]
assert len(CASES) == len(NAMES)


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "build with python -c 'import __graft_entry__ as g; g.build()'"
    L = C.CDLL(LIB)
    vp, u32 = C.c_void_p, C.c_uint32
    L.compat_set_sufsort.argtypes = [vp, u32, C.c_int, u32, vp, u32, u32, vp, vp, vp, vp, vp, vp]
    return L


def _p(a):
    return C.c_void_p(a.ctypes.data)


@pytest.mark.parametrize("skip", [0, 5])
@pytest.mark.parametrize("big_endian", [True, False], ids=["be", "le"])
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_concatenated_device_set(cuda, lib, case, big_endian, skip):
    e = R.expected(case)
    n, N = case.n_suffixes, case.n_strings
    lead = np.random.default_rng(skip).integers(0, 4, skip, dtype=np.uint8)
    stream = np.concatenate([lead, case.stream])
    words = T.pack(stream if stream.size else np.zeros(1, dtype=np.uint8), big_endian)
    offsets = np.concatenate([case.begin, [case.stream.size]]).astype(np.uint64)       # concatenated: begin[i + 1] = the end of string i
    suffixes, ids, cum = np.empty(n, np.uint32), np.empty(n, np.uint32), np.empty(N, np.uint32)
    bwt, pos, dids = np.empty(n, np.uint8), np.empty(N, np.uint64), np.empty(N, np.uint64)
    assert lib.compat_set_sufsort(_p(words), words.size, int(big_endian), skip, _p(offsets), N, n, _p(suffixes), _p(ids), _p(cum), _p(bwt), _p(pos), _p(dids)) == 0
    assert (suffixes == e.suffixes).all() and (ids == e.string_ids).all() and (cum == e.cum).all()
    assert (bwt == e.bwt).all() and (pos == e.dollar_rows).all() and (dids == e.dollar_ids).all()
    # and the C-ABI's arrays for the same strings
    d_set = nvb.PackedStringSet.from_host(case.words(big_endian), 2, big_endian, case.begin, case.length, device=cuda)
    a_suffixes, a_ids, a_cum = nvb.set_suffix_sort(d_set)
    a_bwt, a_rows, a_dids, _ = nvb.set_bwt(d_set)
    u32 = lambda t: t.cpu().numpy().view(np.uint32)
    assert suffixes.tobytes() == u32(a_suffixes).tobytes() and ids.tobytes() == u32(a_ids).tobytes() and cum.tobytes() == u32(a_cum).tobytes()
    assert bwt.tobytes() == a_bwt.cpu().numpy().tobytes() and (pos == u32(a_rows)).all() and (dids == u32(a_dids)).all()


def test_wider_alphabets_throw(cuda, lib):
    assert lib.compat_set_bwt_4bit_throws() == 1
