"""Byte alphabets: suffix sort and BWT of a byte text, the wavelet tree (the reference's nvbio/strings/wavelet_tree.h) and an FM-index over
the wavelet tree of a BWT (its fm_index<WaveletTree, ..>, as examples/waveletfm uses it).  All compute happens in libnvbio_hip.so
(nvbio_amd/csrc/wavelet.hip and sufsort.hip); with device="cpu" the same calls go through the library's host twins and
return the same bytes in host tensors.

A text is a uint8 tensor / array with one symbol per byte, of which the low `symbol_size` bits (1 to 8) are read.  Unsigned 32-bit words
live in int32 tensors."""
import ctypes as C

import torch

from ._lib import lib, check, current_stream_ptr, WaveletTreeStruct, WaveletFMIndexStruct, ByteStringSetStruct

MAX_LENGTH = 0xFFFFFFFE       # of a text to sort
MAX_BITS = 0xFFFFFFFF         # size * symbol_size of a tree


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _device(device, *tensors):
    if device is not None:
        return torch.device(device)
    for t in tensors:
        if torch.is_tensor(t) and t.is_cuda:
            return t.device
    return torch.device("cuda")


def _as(t, dtype, dev):
    """a contiguous tensor of that width on the device; unsigned numpy input keeps its bits"""
    if not torch.is_tensor(t):
        import numpy as np
        a = np.ascontiguousarray(t)
        if a.dtype.kind == "u" and a.dtype.itemsize > 1:
            a = a.view({2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])
        t = torch.from_numpy(a)
    return t.to(dev).to(dtype).contiguous()


def _text(text, symbol_size, device, what, max_len):
    if not 1 <= int(symbol_size) <= 8:
        raise ValueError("%s: symbol_size must be between 1 and 8, not %d" % (what, symbol_size))
    sym = torch.as_tensor(text)
    if sym.dim() != 1 or sym.dtype not in (torch.uint8, torch.int8):
        raise ValueError("%s: the text must be a one-dimensional array of bytes" % what)
    dev = _device(device, sym)
    sym = sym.to(dev).view(torch.uint8).contiguous()
    if not 1 <= sym.numel() <= max_len:
        raise ValueError("%s: the text must hold between 1 and %d symbols, not %d" % (what, max_len, sym.numel()))
    return sym, dev


def _run(dev, name, device_args, host_args):
    """the device entry with the current stream, or its host twin"""
    if dev.type == "cpu":
        check(getattr(lib(), name + "_host")(*host_args, 0), name + "_host")
    else:
        check(getattr(lib(), name)(*device_args, current_stream_ptr()), name)


def suffix_sort_bytes(text, symbol_size=8, device=None):
    """The suffix array of a byte text: int32 [n + 1] holding uint32 values, SA[0] = n, a proper prefix first (as suffix_sort)."""
    sym, dev = _text(text, symbol_size, device, "suffix_sort_bytes", MAX_LENGTH)
    n = sym.numel()
    sa = torch.empty(n + 1, dtype=torch.int32, device=dev)
    if dev.type == "cpu":
        check(lib().nvbio_hip_suffix_sort_bytes_host(_vp(sym), symbol_size, n, _vp(sa), 0), "nvbio_hip_suffix_sort_bytes_host")
    else:
        tb = int(lib().nvbio_hip_suffix_sort_bytes_temp_bytes(n))
        temp = torch.empty(tb, dtype=torch.uint8, device=dev)
        check(lib().nvbio_hip_suffix_sort_bytes(_vp(sym), symbol_size, n, _vp(sa), _vp(temp), tb, current_stream_ptr()), "nvbio_hip_suffix_sort_bytes")
    return sa


def bwt_bytes(text, symbol_size=8, sa_int=16, keep_sa=False, device=None):
    """-> (bwt, primary, ssa, sa): the BWT of a byte text with the '$' row dropped (uint8 [n]), the row of suffix 0, the suffix array
    sampled every `sa_int` rows with ssa[0] = -1, and the whole suffix array (None unless keep_sa)."""
    sym, dev = _text(text, symbol_size, device, "bwt_bytes", MAX_LENGTH)
    if sa_int < 1:
        raise ValueError("bwt_bytes: sa_int must be at least 1")
    n = sym.numel()
    out = torch.empty(n, dtype=torch.uint8, device=dev)
    ssa = torch.empty((n + sa_int) // sa_int, dtype=torch.int32, device=dev)
    sa = torch.empty(n + 1, dtype=torch.int32, device=dev) if keep_sa else None
    primary = C.c_uint32(0)
    if dev.type == "cpu":
        check(lib().nvbio_hip_bwt_bytes_host(_vp(sym), symbol_size, n, int(sa_int), _vp(out), C.byref(primary), _vp(ssa), _vp(sa), 0), "nvbio_hip_bwt_bytes_host")
    else:
        tb = int(lib().nvbio_hip_bwt_bytes_temp_bytes(n))
        temp = torch.empty(tb, dtype=torch.uint8, device=dev)
        check(lib().nvbio_hip_bwt_bytes(_vp(sym), symbol_size, n, int(sa_int), _vp(out), C.byref(primary), _vp(ssa), _vp(sa), _vp(temp), tb,
                                        current_stream_ptr()), "nvbio_hip_bwt_bytes")
    return out, int(primary.value), ssa, sa


class WaveletTree:
    """The wavelet tree of `size` symbols of `symbol_size` bits: `bits` (int32 [W], W = ceil(size * symbol_size / 32)), `splits`
    (int32 [K], K = 2^symbol_size) and `occ` (int32 [K + W]), in the reference's layout (include/nvbio_hip.h)."""

    def __init__(self, symbol_size, size, bits, splits, occ):
        self.symbol_size, self.size = int(symbol_size), int(size)
        self.bits, self.splits, self.occ = bits, splits, occ

    @property
    def device(self):
        return self.bits.device

    def struct(self):
        s = WaveletTreeStruct()
        s.bits, s.splits, s.occ = self.bits.data_ptr(), self.splits.data_ptr(), self.occ.data_ptr()
        s.symbol_size, s.size = self.symbol_size, self.size
        return s

    @staticmethod
    def build(symbols, symbol_size, device=None):
        if 1 <= int(symbol_size) <= 8:
            max_len = MAX_BITS // int(symbol_size)
        else:
            max_len = MAX_BITS
        sym, dev = _text(symbols, symbol_size, device, "WaveletTree.build", max_len)
        n, K = sym.numel(), 1 << symbol_size
        W = (n * symbol_size + 31) // 32
        bits = torch.empty(W, dtype=torch.int32, device=dev)
        splits = torch.empty(K, dtype=torch.int32, device=dev)
        occ = torch.empty(K + W, dtype=torch.int32, device=dev)
        if dev.type == "cpu":
            check(lib().nvbio_hip_wavelet_setup_host(_vp(sym), symbol_size, n, _vp(bits), _vp(splits), _vp(occ), 0), "nvbio_hip_wavelet_setup_host")
        else:
            tb = int(lib().nvbio_hip_wavelet_setup_temp_bytes(n, symbol_size))
            temp = torch.empty(tb, dtype=torch.uint8, device=dev)
            check(lib().nvbio_hip_wavelet_setup(_vp(sym), symbol_size, n, _vp(bits), _vp(splits), _vp(occ), _vp(temp), tb, current_stream_ptr()),
                  "nvbio_hip_wavelet_setup")
        return WaveletTree(symbol_size, n, bits, splits, occ)

    def text(self, positions=None):
        """uint8 [n]: the symbols at `positions` (None: the whole text); a position past the end gives 0"""
        dev = self.device
        if positions is not None:
            positions = _as(positions, torch.int32, dev).reshape(-1)
        n = self.size if positions is None else positions.numel()
        out = torch.empty(n, dtype=torch.uint8, device=dev)
        s = self.struct()
        args = (C.byref(s), _vp(positions), n, _vp(out))
        _run(dev, "nvbio_hip_wavelet_text", args, args)
        return out

    def rank(self, positions, symbols):
        """int32 [n]: the occurrences of symbols[i] in [0, positions[i]]; a position past the end counts as the last, -1 gives 0"""
        dev = self.device
        positions = _as(positions, torch.int32, dev).reshape(-1)
        symbols = _as(symbols, torch.uint8, dev).reshape(-1)
        n = positions.numel()
        if symbols.numel() != n:
            raise ValueError("WaveletTree.rank: %d positions but %d symbols" % (n, symbols.numel()))
        out = torch.empty(n, dtype=torch.int32, device=dev)
        s = self.struct()
        args = (C.byref(s), _vp(positions), _vp(symbols), n, _vp(out))
        _run(dev, "nvbio_hip_wavelet_rank", args, args)
        return out

    def rank_range(self, ranges, symbols):
        """int32 [n, 2]: rank at both ends (x, y) of every range, for symbols[i]"""
        dev = self.device
        ranges = _as(ranges, torch.int32, dev).reshape(-1, 2)
        symbols = _as(symbols, torch.uint8, dev).reshape(-1)
        n = ranges.shape[0]
        if symbols.numel() != n:
            raise ValueError("WaveletTree.rank_range: %d ranges but %d symbols" % (n, symbols.numel()))
        out = torch.empty((n, 2), dtype=torch.int32, device=dev)
        s = self.struct()
        args = (C.byref(s), _vp(ranges), _vp(symbols), n, _vp(out))
        _run(dev, "nvbio_hip_wavelet_rank_range", args, args)
        return out


class ByteStringSet:
    """A set of byte strings over one array of symbols: `begin` (int64 [n]) and `length` (int32 [n], or None with `fixed_length`)."""

    def __init__(self, symbols, begin, length=None, fixed_length=0):
        self.symbols, self.begin, self.length, self.fixed_length = symbols, begin, length, int(fixed_length)

    def __len__(self):
        return self.begin.numel()

    @staticmethod
    def from_lists(strings, device=None):
        strings = [torch.as_tensor(t).reshape(-1) for t in strings]
        for t in strings:
            if t.numel() and t.dtype not in (torch.uint8, torch.int8):
                raise ValueError("ByteStringSet: every string must be an array of bytes")
        dev = _device(device, *strings)
        length = torch.tensor([t.numel() for t in strings], dtype=torch.int64)
        begin = torch.cumsum(length, 0) - length
        parts = [t.view(torch.uint8).to(dev) for t in strings if t.numel()]
        symbols = torch.cat(parts) if parts else torch.zeros(0, dtype=torch.uint8, device=dev)
        return ByteStringSet(symbols, begin.to(dev), length.to(torch.int32).to(dev))

    def to(self, dev):
        return ByteStringSet(self.symbols.to(dev), self.begin.to(dev), None if self.length is None else self.length.to(dev), self.fixed_length)

    def struct(self):
        s = ByteStringSetStruct()
        s.symbols = self.symbols.data_ptr() if self.symbols.numel() else None
        s.n_symbols = self.symbols.numel()
        s.begin = self.begin.data_ptr() if self.begin.numel() else None
        s.length = self.length.data_ptr() if self.length is not None and self.length.numel() else None
        s.fixed_length = self.fixed_length
        return s


class WaveletFMIndex:
    """An FM-index over the wavelet tree of a byte text's BWT: `bwt` (a WaveletTree of the n BWT symbols), `L2` (int32 [K + 1]), `ssa`,
    `primary`, `length`, `sa_int`."""

    def __init__(self, bwt, L2, ssa, primary, sa_int):
        self.bwt, self.L2, self.ssa = bwt, L2, ssa
        self.primary, self.sa_int, self.length = int(primary), int(sa_int), bwt.size

    @property
    def device(self):
        return self.bwt.device

    def struct(self):
        s = WaveletFMIndexStruct()
        s.bwt = self.bwt.struct()
        s.L2 = self.L2.data_ptr()
        s.ssa = self.ssa.data_ptr() if self.ssa is not None else None
        s.length, s.primary, s.sa_int = self.length, self.primary, self.sa_int
        return s

    @staticmethod
    def build(text, symbol_size=8, sa_int=16, device=None):
        max_len = min(MAX_LENGTH, MAX_BITS // int(symbol_size)) if 1 <= int(symbol_size) <= 8 else MAX_LENGTH
        sym, dev = _text(text, symbol_size, device, "WaveletFMIndex.build", max_len)
        bwt, primary, ssa, _ = bwt_bytes(sym, symbol_size, sa_int, device=dev)
        tree = WaveletTree.build(bwt, symbol_size, device=dev)
        L2 = torch.empty((1 << symbol_size) + 1, dtype=torch.int32, device=dev)
        s = tree.struct()
        args = (C.byref(s), _vp(L2))
        _run(dev, "nvbio_hip_wavelet_fm_L2", args, args)
        return WaveletFMIndex(tree, L2, ssa, primary, sa_int)

    def match(self, patterns):
        """int32 [n, 2]: the SA range (x, y), inclusive, of every pattern; x > y where it does not occur.  `patterns`: a ByteStringSet
        or a list of uint8 arrays."""
        dev = self.device
        ps = patterns.to(dev) if isinstance(patterns, ByteStringSet) else ByteStringSet.from_lists(patterns, dev)
        n = len(ps)
        out = torch.empty((n, 2), dtype=torch.int32, device=dev)
        s, p = self.struct(), ps.struct()
        args = (C.byref(s), C.byref(p), n, _vp(out))
        _run(dev, "nvbio_hip_wavelet_fm_match", args, args)
        return out

    def locate(self, rows):
        """int32 [n]: the text position of the suffix on each SA row (row 0, the empty suffix, gives -1 as locate does)"""
        dev = self.device
        if self.ssa is None:
            raise ValueError("WaveletFMIndex.locate: the index has no sampled suffix array")
        rows = _as(rows, torch.int32, dev).reshape(-1)
        n = rows.numel()
        out = torch.empty(n, dtype=torch.int32, device=dev)
        s = self.struct()
        args = (C.byref(s), _vp(rows), n, _vp(out))
        _run(dev, "nvbio_hip_wavelet_fm_locate", args, args)
        return out
