// include/nvbio_hip/wavelet.h -- the C++ host layer of the wavelet tree and the FM-index over it (nvbio/strings/wavelet_tree.h and
// fm_index<WaveletTree, ..>): thin callers of nvbio_hip_wavelet_* (include/nvbio_hip.h) that own their arrays and scratch.
// No HIP headers are needed to include it.
//
//   WaveletTreeDevice      setup(symbols, symbol_size, n): bits / splits / occ in the reference's layout; text, rank, rank_range
//   WaveletFMIndexDevice   build(text, symbol_size, n, sa_int): BWT (bwt_bytes of sufsort.h), its tree, L2, the sampled SA; match, locate
//
// Every pointer argument is device memory.  A text holds one symbol per byte, of which the low symbol_size bits are read.
#pragma once
#include "types.h"
#include "sufsort.h"

namespace nvbio {
namespace hip {

struct WaveletTreeDevice
{
    WaveletTreeDevice() : symbol_size(0), size(0) {}

    /// build the tree of n symbols; asynchronous on `stream` (the scratch is kept in the object)
    void setup(const uint8* symbols, const uint32 symbol_size_, const uint64 n, void* stream = nullptr)
    {
        const uint64 tb = nvbio_hip_wavelet_setup_temp_bytes(n, symbol_size_);
        if (temp.size() < tb) temp.resize(tb);
        if (symbol_size_ >= 1u && symbol_size_ <= 8u)
        {
            const uint64 K = 1ull << symbol_size_, W = (n * symbol_size_ + 31u) / 32u;
            bits.resize(W); splits.resize(K); occ.resize(K + W);
        }
        hip_check(nvbio_hip_wavelet_setup(symbols, symbol_size_, n, bits.data(), splits.data(), occ.data(), temp.data(), temp.size(), stream),
                  "nvbio_hip_wavelet_setup");
        symbol_size = symbol_size_; size = uint32(n);
    }
    nvbio_hip_wavelet_tree abi() const
    {
        nvbio_hip_wavelet_tree t;
        t.bits = bits.data(); t.splits = splits.data(); t.occ = occ.data(); t.symbol_size = symbol_size; t.size = size;
        return t;
    }
    /// out[i] = the symbol at positions[i] (positions == NULL: at i), 0 past the end
    void text(const uint32* positions, const uint64 n_queries, uint8* out, void* stream = nullptr) const
    {
        const nvbio_hip_wavelet_tree t = abi();
        hip_check(nvbio_hip_wavelet_text(&t, positions, n_queries, out, stream), "nvbio_hip_wavelet_text");
    }
    /// out[i] = the occurrences of symbols[i] in [0, positions[i]]
    void rank(const uint32* positions, const uint8* symbols, const uint64 n_queries, uint32* out, void* stream = nullptr) const
    {
        const nvbio_hip_wavelet_tree t = abi();
        hip_check(nvbio_hip_wavelet_rank(&t, positions, symbols, n_queries, out, stream), "nvbio_hip_wavelet_rank");
    }
    /// the same at both ends (x, y) of n_queries ranges
    void rank_range(const uint32* ranges, const uint8* symbols, const uint64 n_queries, uint32* out, void* stream = nullptr) const
    {
        const nvbio_hip_wavelet_tree t = abi();
        hip_check(nvbio_hip_wavelet_rank_range(&t, ranges, symbols, n_queries, out, stream), "nvbio_hip_wavelet_rank_range");
    }

    uint32                 symbol_size, size;
    device_vector<uint32>  bits, splits, occ;
    device_vector<uint8>   temp;
};

struct WaveletFMIndexDevice
{
    WaveletFMIndexDevice() : length(0), primary(0), sa_int(0) {}

    /// index a text of n symbols: its BWT, the BWT's tree, L2 and the suffix array sampled every sa_int_ rows.  The sorter waits for
    /// the stream once per round; the tree and L2 are queued behind it.
    void build(const uint8* text, const uint32 symbol_size, const uint64 n, const uint32 sa_int_, void* stream = nullptr)
    {
        bwt_bytes(text, symbol_size, n, sa_int_, sorted, bwt.temp, true, false, stream);
        bwt.setup(sorted.bwt.data(), symbol_size, n, stream);
        L2.resize((1u << symbol_size) + 1u);
        const nvbio_hip_wavelet_tree t = bwt.abi();
        hip_check(nvbio_hip_wavelet_fm_L2(&t, L2.data(), stream), "nvbio_hip_wavelet_fm_L2");
        length = uint32(n); primary = sorted.primary; sa_int = sa_int_;
    }
    nvbio_hip_wavelet_fmindex abi() const
    {
        nvbio_hip_wavelet_fmindex f;
        f.bwt = bwt.abi(); f.L2 = L2.data(); f.ssa = sorted.ssa.size() ? sorted.ssa.data() : nullptr;
        f.length = length; f.primary = primary; f.sa_int = sa_int; f._pad = 0u;
        return f;
    }
    /// ranges_out[i] = the inclusive SA range (x, y) of pattern i, x > y where it does not occur
    void match(const nvbio_hip_byte_string_set& patterns, const uint64 n, uint32* ranges_out, void* stream = nullptr) const
    {
        const nvbio_hip_wavelet_fmindex f = abi();
        hip_check(nvbio_hip_wavelet_fm_match(&f, &patterns, n, ranges_out, stream), "nvbio_hip_wavelet_fm_match");
    }
    /// positions_out[i] = SA[rows[i]]
    void locate(const uint32* rows, const uint64 n_rows, uint32* positions_out, void* stream = nullptr) const
    {
        const nvbio_hip_wavelet_fmindex f = abi();
        hip_check(nvbio_hip_wavelet_fm_locate(&f, rows, n_rows, positions_out, stream), "nvbio_hip_wavelet_fm_locate");
    }

    uint32                 length, primary, sa_int;
    WaveletTreeDevice      bwt;
    device_vector<uint32>  L2;
    ByteBWTResult          sorted;         ///< the BWT symbols the tree was built from, and the sampled suffix array
};

} // namespace hip
} // namespace nvbio
