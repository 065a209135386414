// tests/cxx/set_sufsort_shim.cpp -- the C++ host layer's set_suffix_sort / set_bwt (include/nvbio_hip/sufsort.h) behind one C entry point
// that tests/test_set_sufsort_gpu.py calls.  g++, no HIP.
#include "nvbio_hip/sufsort.h"
#include <stdio.h>
#include <exception>
#include <vector>

using namespace nvbio;

template <typename T>
static void to_host(T* out, const hip::device_vector<T>& v) { hip_check(nvbio_hip_memcpy(out, v.data(), v.size() * sizeof(T), 2, nullptr), "nvbio_hip_memcpy"); }

/// a string set in host memory -> everything the two calls return, through device vectors
template <bool BE>
static int run(const unsigned* h_words, unsigned long long n_words, const unsigned long long* h_begin, const unsigned* h_length, unsigned fixed_length, unsigned n_strings,
               unsigned* out_suffixes, unsigned* out_string_ids, unsigned* out_cum, unsigned char* out_bwt, unsigned* out_dollar_rows, unsigned* out_dollar_ids,
               unsigned* out_pairs)
{
    hip::device_vector<uint32> words(std::vector<uint32>(h_words, h_words + n_words));
    hip::device_vector<uint64> begin(std::vector<uint64>(h_begin, h_begin + n_strings));
    hip::device_vector<uint32> length;
    if (h_length) length.assign(h_length, n_strings);
    const PackedStringSetView<2, BE> set(n_strings, words.data(), n_words, begin.data(), h_length ? length.data() : nullptr, fixed_length);
    const uint64 n = hip::set_slot_count(set);
    hip::device_vector<uint8> temp;
    hip::SetSuffixSortResult sorted;
    hip::set_suffix_sort(set, n, sorted, temp);
    if (sorted.suffixes.size() != n || sorted.string_ids.size() != n || sorted.cum_lengths.size() != n_strings) return -2;
    to_host(out_suffixes, sorted.suffixes); to_host(out_string_ids, sorted.string_ids); to_host(out_cum, sorted.cum_lengths);
    hip::SetBWTResult plain, r;
    hip::set_bwt(set, n, plain);                          // a scratch of its own, no pairs
    if (plain.suffixes.size() != 0u) return -3;
    hip::set_bwt(set, n, r, temp, true);                  // the sorter's scratch, grown
    if (r.bwt.size() != n || r.dollar_rows.size() != n_strings || r.suffixes.size() != 2u * n) return -4;
    const std::vector<uint8> a = plain.bwt.to_host(), b = r.bwt.to_host();
    if (a != b || plain.dollar_rows.to_host() != r.dollar_rows.to_host()) return -5;
    to_host(out_bwt, r.bwt); to_host(out_dollar_rows, r.dollar_rows); to_host(out_dollar_ids, r.dollar_ids); to_host(out_pairs, r.suffixes);
    hip_check(nvbio_hip_stream_synchronize(nullptr), "nvbio_hip_stream_synchronize");
    // a wrong slot count is an exception
    try { hip::set_suffix_sort(set, n + 1u, sorted, temp); return -6; } catch (const hip_error& e) { if (e.code != 1) return -7; }
    return 0;
}

extern "C" __attribute__((visibility("default")))
int set_sufsort_host_layer(const unsigned* h_words, unsigned long long n_words, int big_endian, const unsigned long long* h_begin, const unsigned* h_length,
                           unsigned fixed_length, unsigned n_strings, unsigned* out_suffixes, unsigned* out_string_ids, unsigned* out_cum, unsigned char* out_bwt,
                           unsigned* out_dollar_rows, unsigned* out_dollar_ids, unsigned* out_pairs)
{
    try {
        return big_endian ? run<true>(h_words, n_words, h_begin, h_length, fixed_length, n_strings, out_suffixes, out_string_ids, out_cum, out_bwt, out_dollar_rows, out_dollar_ids, out_pairs)
                          : run<false>(h_words, n_words, h_begin, h_length, fixed_length, n_strings, out_suffixes, out_string_ids, out_cum, out_bwt, out_dollar_rows, out_dollar_ids, out_pairs);
    } catch (const std::exception& e) { fprintf(stderr, "set_sufsort_host_layer: %s\n", e.what()); return -1; }
}
