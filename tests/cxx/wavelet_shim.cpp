// tests/cxx/wavelet_shim.cpp -- the C++ host layer's WaveletTreeDevice / WaveletFMIndexDevice (include/nvbio_hip/wavelet.h) behind C entry
// points that tests/test_wavelet_shim_gpu.py calls.  g++, no HIP.
#include "nvbio_hip/wavelet.h"
#include <stdio.h>
#include <exception>
#include <vector>

using namespace nvbio;

template <typename T>
static void to_host(T* out, const hip::device_vector<T>& v)
{
    hip_check(nvbio_hip_memcpy(out, v.data(), uint64(v.size()) * sizeof(T), 2, nullptr), "nvbio_hip_memcpy");
}

/// host text -> the tree's three arrays, the whole text read back and the rank of every (position, symbol) query
extern "C" __attribute__((visibility("default")))
int wavelet_tree_host_layer(const unsigned char* h_text, unsigned symbol_size, unsigned long long n, const unsigned* h_positions, const unsigned char* h_symbols,
                            unsigned long long n_queries, unsigned* out_bits, unsigned* out_splits, unsigned* out_occ, unsigned char* out_text,
                            unsigned* out_rank, unsigned* out_rank_range)
{
    try {
        hip::device_vector<uint8> text(std::vector<uint8>(h_text, h_text + n));
        hip::WaveletTreeDevice tree;
        tree.setup(text.data(), symbol_size, n);
        if (tree.size != n || tree.bits.size() != (n * symbol_size + 31u) / 32u || tree.splits.size() != (1u << symbol_size)) return -2;
        to_host(out_bits, tree.bits); to_host(out_splits, tree.splits); to_host(out_occ, tree.occ);
        hip::device_vector<uint8>  read_back(n), symbols(std::vector<uint8>(h_symbols, h_symbols + n_queries));
        hip::device_vector<uint32> positions(std::vector<uint32>(h_positions, h_positions + n_queries)), ranks(n_queries), pairs(n_queries & ~1ull);
        tree.text(nullptr, n, read_back.data());
        tree.rank(positions.data(), symbols.data(), n_queries, ranks.data());
        tree.rank_range(positions.data(), symbols.data(), n_queries / 2u, pairs.data());     // the positions two by two as ranges
        to_host(out_text, read_back); to_host(out_rank, ranks); to_host(out_rank_range, pairs);
        hip::synchronize();
        return 0;
    } catch (const std::exception& e) { fprintf(stderr, "wavelet_tree_host_layer: %s\n", e.what()); return -1; }
}

/// host text and patterns -> L2, primary, the ranges of the patterns and the positions of the rows
extern "C" __attribute__((visibility("default")))
int wavelet_fm_host_layer(const unsigned char* h_text, unsigned symbol_size, unsigned long long n, unsigned sa_int, const unsigned char* h_pattern_symbols,
                          unsigned long long n_pattern_symbols, const unsigned long long* h_begin, const unsigned* h_length, unsigned long long n_patterns,
                          const unsigned* h_rows, unsigned long long n_rows, unsigned* out_L2, unsigned* out_primary, unsigned* out_ranges, unsigned* out_positions)
{
    try {
        hip::device_vector<uint8> text(std::vector<uint8>(h_text, h_text + n));
        hip::WaveletFMIndexDevice fmi;
        fmi.build(text.data(), symbol_size, n, sa_int);
        if (fmi.length != n || fmi.L2.size() != (1u << symbol_size) + 1u) return -2;
        hip::device_vector<uint8>  psym(std::vector<uint8>(h_pattern_symbols, h_pattern_symbols + n_pattern_symbols));
        hip::device_vector<uint64> begin(std::vector<uint64>(h_begin, h_begin + n_patterns));
        hip::device_vector<uint32> length(std::vector<uint32>(h_length, h_length + n_patterns)), rows(std::vector<uint32>(h_rows, h_rows + n_rows));
        hip::device_vector<uint32> ranges(2u * n_patterns), positions(n_rows);
        nvbio_hip_byte_string_set ps;
        ps.symbols = psym.data(); ps.n_symbols = n_pattern_symbols; ps.begin = begin.data(); ps.length = length.data(); ps.fixed_length = 0u; ps._pad = 0u;
        fmi.match(ps, n_patterns, ranges.data());
        fmi.locate(rows.data(), n_rows, positions.data());
        to_host(out_L2, fmi.L2); to_host(out_ranges, ranges); to_host(out_positions, positions);
        hip::synchronize();
        *out_primary = fmi.primary;
        return 0;
    } catch (const std::exception& e) { fprintf(stderr, "wavelet_fm_host_layer: %s\n", e.what()); return -1; }
}
