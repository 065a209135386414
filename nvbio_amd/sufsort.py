"""Suffix sorting and BWT construction on the device: the plain-string front door of the reference's nvbio/sufsort
(cuda::suffix_sort, cuda::bwt, cuda::find_primary; nvbio/sufsort/sufsort.h).  All compute happens in libnvbio_hip.so
(nvbio_amd/csrc/sufsort.hip).

A text is either a uint8 tensor / array of symbols 0..3, or a packed triple `(words, n)` / `(words, n, big_endian)` with `words`
an int32 tensor of 2-bit PackedStream words (big-endian by default)."""
import ctypes as C

import torch

from ._lib import lib, check, current_stream_ptr
from .strings import pack_symbols

MAX_LENGTH = 0xFFFFFFFE


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _pack_text(sym, chunk_syms=1 << 26):
    """2-bit big-endian words of a symbol tensor, packed in word-aligned chunks (bounds the temporaries)"""
    n = sym.numel()
    parts = [pack_symbols(sym[s:min(n, s + chunk_syms)], 2, True, pad_words=0) for s in range(0, n, chunk_syms)]
    return torch.cat(parts) if len(parts) > 1 else parts[0]


def _packed(text, device=None):
    """-> (words int32 device tensor, n, big_endian)"""
    if isinstance(text, (tuple, list)):
        words, n = text[0], int(text[1])
        be = bool(text[2]) if len(text) > 2 else True
        assert words.dtype == torch.int32 and words.is_contiguous() and words.numel() * 16 >= n
        return words, n, be
    if not torch.is_tensor(text):
        text = torch.as_tensor(text)
    if device is not None:
        text = text.to(device)
    assert text.dim() == 1
    if text.numel() == 0:
        raise ValueError("the text must hold between 1 and 2^32 - 2 symbols")
    return _pack_text(text.to(torch.uint8)), text.numel(), True


def suffix_sort(text):
    """The suffix array of `text` as a device int32 tensor [n + 1] holding uint32 values, in the convention of the reference's
    bwt.h: SA[0] = n is the empty suffix, and a suffix that is a proper prefix of another sorts first."""
    words, n, be = _packed(text)
    if not 1 <= n <= MAX_LENGTH:
        raise ValueError("suffix_sort: the text must hold between 1 and 2^32 - 2 symbols")
    L = lib()
    sa = torch.empty(n + 1, dtype=torch.int32, device=words.device)
    tb = int(L.nvbio_hip_suffix_sort_temp_bytes(n))
    temp = torch.empty(tb, dtype=torch.uint8, device=words.device)
    check(L.nvbio_hip_suffix_sort(_vp(words), 2, int(be), n, _vp(sa), _vp(temp), tb, current_stream_ptr()), "nvbio_hip_suffix_sort")
    return sa


def last_rounds():
    """[unresolved suffixes after round 0, after round 1, ...] of this thread's last suffix_sort / bwt call"""
    buf = (C.c_uint64 * 64)()
    r = int(lib().nvbio_hip_suffix_sort_last_rounds(buf, 64))
    return [int(buf[k]) for k in range(min(r, 64))]


def bwt(text, sa_int=16, keep_sa=False, want_ssa=True):
    """-> (bwt_words, primary, ssa, sa): the BWT of `text` with the '$' row dropped as big-endian 2-bit words (int32
    [4 * ceil(n / 64)], what build_bwt_occ takes), the row of suffix 0, the suffix array sampled every `sa_int` rows with
    ssa[0] = -1 (None unless want_ssa), and the whole suffix array (None unless keep_sa)."""
    words, n, be = _packed(text)
    if not 1 <= n <= MAX_LENGTH:
        raise ValueError("bwt: the text must hold between 1 and 2^32 - 2 symbols")
    if sa_int < 1:
        raise ValueError("bwt: sa_int must be at least 1")
    L = lib()
    dev = words.device
    out = torch.empty(4 * ((n + 63) // 64), dtype=torch.int32, device=dev)
    ssa = torch.empty((n + sa_int) // sa_int, dtype=torch.int32, device=dev) if want_ssa else None
    sa = torch.empty(n + 1, dtype=torch.int32, device=dev) if keep_sa else None
    tb = int(L.nvbio_hip_bwt_temp_bytes(n))
    temp = torch.empty(tb, dtype=torch.uint8, device=dev)
    primary = C.c_uint32(0)
    check(L.nvbio_hip_bwt(_vp(words), 2, int(be), n, int(sa_int), _vp(out), C.byref(primary), _vp(ssa), _vp(sa), _vp(temp), tb,
                          current_stream_ptr()), "nvbio_hip_bwt")
    return out, int(primary.value), ssa, sa


def build_fm_index(text, sa_int=16, keep_sa=False):
    """FM-index of a text in the reference's production layout, field for field what workloads.build_fm_index returns:
    nvbio_amd.FMIndexDevice (and the suffix array, int64 [n + 1], if keep_sa)."""
    from .fmindex import FMIndexDevice, build_bwt_occ
    words, n, be = _packed(text)
    bwt_words, primary, ssa, sa = bwt((words, n, be), sa_int, keep_sa)
    bwt_occ, L2 = build_bwt_occ(n, bwt_words)
    fmi = FMIndexDevice(n, primary, L2, bwt_occ, ssa, sa_int)
    if keep_sa:
        return fmi, sa.to(torch.int64) & 0xFFFFFFFF
    return fmi
