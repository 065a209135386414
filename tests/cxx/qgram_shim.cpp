// tests/cxx/qgram_shim.cpp -- the C++ host layer's q-gram index and filter (include/nvbio_hip/qgram.h) behind one C entry point that
// tests/test_compat_qgram_gpu.py calls.  g++, no HIP.
#include "nvbio_hip/qgram.h"
#include <stdio.h>
#include <exception>
#include <vector>

using namespace nvbio;

template <typename T, typename U>
static void to_host(U* out, const hip::device_vector<T>& v, const size_t n)
{
    if (n) hip_check(nvbio_hip_memcpy(out, v.data(), n * sizeof(T), 2, nullptr), "nvbio_hip_memcpy");
}

struct Outputs
{
    unsigned* n_unique; unsigned* n_qgrams; unsigned long long* qgrams; unsigned* slots; unsigned* index; unsigned* lut;
    unsigned* ranges; unsigned long long* total; unsigned long long hits_capacity; unsigned* hits; unsigned* n_merged; unsigned* merged; unsigned* counts;
};

/// a built index -> its arrays, the ranges of the queries, and the filter's hits (located in two uneven batches) and merged diagonals
template <typename index_type>
static int run_filter(const index_type& ix, const unsigned long long* h_queries, const unsigned* h_indices, unsigned n_queries, unsigned merge_interval, const Outputs& o)
{
    typedef hip::QGramFilterDevice<index_type> filter_type;
    typedef typename filter_type::hit_type      hit_type;
    typedef typename filter_type::diagonal_type diagonal_type;
    *o.n_unique = ix.n_unique_qgrams; *o.n_qgrams = ix.n_qgrams;
    to_host(o.qgrams, ix.qgrams, ix.n_unique_qgrams); to_host(o.slots, ix.slots, ix.n_unique_qgrams + 1u); to_host(o.index, ix.index, ix.n_qgrams);
    to_host(o.lut, ix.lut, ix.lut.size());
    hip::device_vector<uint64> queries(std::vector<uint64>(h_queries, h_queries + n_queries));
    hip::device_vector<uint32> indices(std::vector<uint32>(h_indices, h_indices + n_queries));
    hip::device_vector<uint2> ranges;
    ix.range(queries.data(), n_queries, ranges);
    to_host(o.ranges, ranges, n_queries);
    filter_type filter;
    const uint64 total = filter.rank(ix, n_queries, queries.data(), indices.data());
    *o.total = total;
    if (total != filter.n_hits() || total > o.hits_capacity) return -2;
    hip::device_vector<hit_type> hits(total);
    const uint64 cut = total / 3u;
    filter.locate(0u, cut, hits.data());
    filter.locate(cut, total, hits.data() + cut);
    to_host(o.hits, hits, total);
    hip::device_vector<diagonal_type> merged(total);
    hip::device_vector<uint32> counts(total);
    *o.n_merged = filter.merge(merge_interval, uint32(total), hits.data(), merged.data(), counts.data());
    to_host(o.merged, merged, *o.n_merged); to_host(o.counts, counts, *o.n_merged);
    hip_check(nvbio_hip_stream_synchronize(nullptr), "nvbio_hip_stream_synchronize");
    return 0;
}

template <bool BE>
static int run(const unsigned* h_words, unsigned long long n_words, unsigned long long len, const unsigned long long* h_begin, const unsigned* h_length,
               unsigned fixed_length, unsigned n_strings, int is_set, unsigned q, unsigned ql, unsigned seed_interval,
               const unsigned long long* h_queries, const unsigned* h_indices, unsigned n_queries, unsigned merge_interval, const Outputs& o)
{
    hip::device_vector<uint32> words(std::vector<uint32>(h_words, h_words + n_words));
    if (!is_set)
    {
        const hip::PackedTextView<BE> text(words.data(), len);
        hip::device_vector<uint64> all;
        hip::generate_qgrams(text, q, nullptr, len, all);                      // the first q-gram of the index's smallest slot must be among them
        hip::QGramIndexDevice ix;
        ix.build(q, text, ql);
        if (all.size() != len) return -3;
        // an illegal q is an exception
        try { hip::QGramIndexDevice bad; bad.build(33u, text, 0u); return -4; } catch (const hip_error& e) { if (e.code != 1) return -5; }
        return run_filter(ix, h_queries, h_indices, n_queries, merge_interval, o);
    }
    hip::device_vector<uint64> begin(std::vector<uint64>(h_begin, h_begin + n_strings));
    hip::device_vector<uint32> length;
    if (h_length) length.assign(h_length, n_strings);
    const PackedStringSetView<2, BE> set(n_strings, words.data(), n_words, begin.data(), h_length ? length.data() : nullptr, fixed_length);
    hip::QGramSetIndexDevice ix;
    ix.build(q, set, seed_interval, ql);
    return run_filter(ix, h_queries, h_indices, n_queries, merge_interval, o);
}

extern "C" __attribute__((visibility("default")))
int qgram_host_layer(const unsigned* h_words, unsigned long long n_words, int big_endian, unsigned long long len, const unsigned long long* h_begin,
                     const unsigned* h_length, unsigned fixed_length, unsigned n_strings, int is_set, unsigned q, unsigned ql, unsigned seed_interval,
                     const unsigned long long* h_queries, const unsigned* h_indices, unsigned n_queries, unsigned merge_interval, const Outputs* out)
{
    try {
        return big_endian ? run<true>(h_words, n_words, len, h_begin, h_length, fixed_length, n_strings, is_set, q, ql, seed_interval, h_queries, h_indices, n_queries, merge_interval, *out)
                          : run<false>(h_words, n_words, len, h_begin, h_length, fixed_length, n_strings, is_set, q, ql, seed_interval, h_queries, h_indices, n_queries, merge_interval, *out);
    } catch (const std::exception& e) { fprintf(stderr, "qgram_host_layer: %s\n", e.what()); return -1; }
}
