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


# ---- string sets (nvbio_hip_set_suffix_sort / nvbio_hip_set_bwt): the suffixes of every string of a set, the empty ones included ----

def _string_set(string_set, what):
    """-> (PackedStringSet, n_strings, n_suffixes) of a 2-bit PackedStringSet or a list of uint8 symbol arrays (packed first)"""
    from .strings import PackedStringSet
    if not isinstance(string_set, PackedStringSet):
        strings = [torch.as_tensor(t).to(torch.uint8).reshape(-1) for t in string_set]
        if not strings:
            raise ValueError(what + ": the set must hold at least one string")
        dev = next((t.device for t in strings if t.is_cuda), torch.device("cuda"))
        length = torch.tensor([t.numel() for t in strings], dtype=torch.int64)
        begin = torch.cumsum(length, 0) - length
        words = pack_symbols(torch.cat(strings).to(dev), 2, True, pad_words=1)
        string_set = PackedStringSet(words, 2, True, begin.to(dev), length.to(torch.int32).to(dev))
    n_strings = len(string_set)
    if n_strings == 0:
        raise ValueError(what + ": the set must hold at least one string")
    if string_set.bits != 2:
        raise ValueError(what + ": only 2-bit string sets are supported, this one has %d bits a symbol" % string_set.bits)
    if string_set.length is not None:
        n_suffixes = int((string_set.length.to(torch.int64) & 0xFFFFFFFF).sum()) + n_strings
    else:
        n_suffixes = n_strings * (string_set.fixed_length + 1)
    if n_suffixes > MAX_LENGTH:
        raise ValueError(what + ": the set has %d slots (symbols + strings), more than 2^32 - 2" % n_suffixes)
    return string_set, n_strings, n_suffixes


def set_suffix_sort(string_set):
    """The suffixes of all the strings of a set, sorted: -> (suffixes, string_ids, cum_lengths), device int32 tensors holding uint32
    values.  String s contributes the len[s] + 1 slots (s, p), 0 <= p <= len[s] (the empty suffix included); slot (s, p) has the global
    index cum_lengths[s - 1] + p, cum_lengths = the inclusive sums of len + 1.  suffixes[row] = the global index on that row, in the
    order of the symbols with a proper prefix first and equal suffixes by string id; string_ids[g] = the string of global index g.
    `string_set`: a PackedStringSet with bits == 2, or a list of uint8 symbol arrays."""
    ss, n_strings, n = _string_set(string_set, "set_suffix_sort")
    L = lib()
    dev = ss.words.device
    suffixes = torch.empty(n, dtype=torch.int32, device=dev)
    string_ids = torch.empty(n, dtype=torch.int32, device=dev)
    cum = torch.empty(n_strings, dtype=torch.int32, device=dev)
    tb = int(L.nvbio_hip_set_suffix_sort_temp_bytes(n, n_strings))
    temp = torch.empty(tb, dtype=torch.uint8, device=dev)
    s = ss.struct()
    check(L.nvbio_hip_set_suffix_sort(C.byref(s), n_strings, n, _vp(suffixes), _vp(string_ids), _vp(cum), _vp(temp), tb, current_stream_ptr()),
          "nvbio_hip_set_suffix_sort")
    return suffixes, string_ids, cum


def set_bwt(string_set, keep_suffixes=False):
    """The BWT of a string set: -> (bwt, dollar_rows, dollar_ids, suffixes).  bwt: uint8 [n_suffixes], the symbol before the suffix on
    each row, 255 where the suffix is a whole string; dollar_rows: those rows, ascending, and dollar_ids: the string each starts (int32
    tensors holding uint32 values); suffixes: int32 [n_suffixes, 2], the (position, string) of every row (None unless keep_suffixes)."""
    ss, n_strings, n = _string_set(string_set, "set_bwt")
    L = lib()
    dev = ss.words.device
    out = torch.empty(n, dtype=torch.uint8, device=dev)
    rows = torch.empty(n_strings, dtype=torch.int32, device=dev)
    ids = torch.empty(n_strings, dtype=torch.int32, device=dev)
    pairs = torch.empty((n, 2), dtype=torch.int32, device=dev) if keep_suffixes else None
    tb = int(L.nvbio_hip_set_bwt_temp_bytes(n, n_strings))
    temp = torch.empty(tb, dtype=torch.uint8, device=dev)
    s = ss.struct()
    check(L.nvbio_hip_set_bwt(C.byref(s), n_strings, n, _vp(out), _vp(rows), _vp(ids), _vp(pairs), _vp(temp), tb, current_stream_ptr()),
          "nvbio_hip_set_bwt")
    return out, rows, ids, pairs
