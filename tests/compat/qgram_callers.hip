// tests/compat/qgram_callers.hip -- callers of the q-gram module written in the reference's vocabulary (nvbio/qgram/qgram.h, filter.h):
// a QGramIndexDevice / QGramSetIndexDevice built from a packed 2-bit stream or from 8-bit symbols, the index's plain view as the functor
// of a thrust::transform, the index copied to the host with operator=, and QGramFilterDevice / QGramFilterHost ranking, locating and
// merging.  It includes the reference's header names and is compiled with `hipcc -I include/nvbio_hip/compat`.  The extern "C" entry
// points take and return host memory so that the Python tests can drive it.
#include <nvbio/basic/types.h>
#include <nvbio/basic/packedstream.h>
#include <nvbio/basic/vector.h>
#include <nvbio/strings/string_set.h>
#include <nvbio/strings/seeds.h>
#include <nvbio/qgram/qgram.h>
#include <nvbio/qgram/filter.h>
#include <thrust/device_vector.h>
#include <thrust/host_vector.h>
#include <thrust/transform.h>
#include <thrust/copy.h>
#include <stdio.h>
#include <string.h>
#include <exception>
#include <vector>

using namespace nvbio;

#define API extern "C" __attribute__((visibility("default")))

// what a call returns, all host memory sized by the caller (the layout of tests/cxx/qgram_shim.cpp)
struct Outputs
{
    uint32* n_unique; uint32* n_qgrams; uint64* qgrams; uint32* slots; uint32* index; uint32* lut;
    uint32* ranges; uint64* total; uint64 hits_capacity; uint32* hits; uint32* n_merged; uint32* merged; uint32* counts;
};

enum Mode { PACKED_DEVICE = 0, BYTES_DEVICE_GENERIC = 1, PACKED_HOST = 2 };

template <typename T, typename V>
static void to_host(T* out, const V& v, const size_t n) { if (n) thrust::copy(v.begin(), v.begin() + n, reinterpret_cast<typename V::value_type*>(out)); }

template <typename index_type>
static void copy_index(const index_type& ix, const Outputs& o)
{
    *o.n_unique = ix.n_unique_qgrams; *o.n_qgrams = ix.n_qgrams;
    to_host(o.qgrams, ix.qgrams, ix.qgrams.size()); to_host(o.slots, ix.slots, ix.slots.size()); to_host(o.index, ix.index, ix.index.size());
    to_host(o.lut, ix.lut, ix.lut.size());
}

// rank, locate in two uneven batches, merge: on the device, with plain pointers (the tuned execution) or forced generic
template <typename index_type>
static int device_filter(const index_type& ix, const uint64* h_queries, const uint32* h_indices, const uint32 n_queries, const uint32 interval, const bool generic,
                         const char* want_path, const Outputs& o)
{
    typedef QGramFilterDevice<index_type, const uint64*, const uint32*> filter_type;
    typedef typename filter_type::hit_type      hit_type;
    typedef typename filter_type::diagonal_type diagonal_type;

    thrust::device_vector<uint64> queries(h_queries, h_queries + n_queries);
    thrust::device_vector<uint32> indices(h_indices, h_indices + n_queries);

    // the index's view is a functor from q-grams to slot ranges
    thrust::device_vector<uint2> ranges(n_queries);
    thrust::transform(queries.begin(), queries.end(), ranges.begin(), plain_view(ix));
    to_host(o.ranges, ranges, n_queries);

    filter_type filter;
    filter.set_generic(generic);
    const uint64 total = filter.rank(ix, n_queries, thrust::raw_pointer_cast(queries.data()), thrust::raw_pointer_cast(indices.data()));
    *o.total = total;
    if (total != filter.n_hits() || total > o.hits_capacity) return -2;
    if (strcmp(filter.last_path(), want_path) != 0) return -3;
    thrust::device_vector<hit_type> hits(total);
    const uint64 cut = total / 3u;
    filter.locate(0u, cut, hits.begin());
    filter.locate(cut, total, hits.begin() + cut);
    if (total && strcmp(filter.last_path(), want_path) != 0) return -4;
    to_host(o.hits, hits, total);
    thrust::device_vector<diagonal_type> merged(total);
    thrust::device_vector<uint32>        counts(total);
    *o.n_merged = filter.merge(interval, uint32(total), hits.begin(), merged.begin(), counts.begin());
    if (total && strcmp(filter.last_path(), want_path) != 0) return -5;
    to_host(o.merged, merged, *o.n_merged); to_host(o.counts, counts, *o.n_merged);
    return 0;
}

// the same on the host, on an index copied from the device
template <typename host_index_type, typename device_index_type>
static int host_filter(const device_index_type& d_ix, const uint64* h_queries, const uint32* h_indices, const uint32 n_queries, const uint32 interval, const Outputs& o)
{
    typedef QGramFilterHost<host_index_type, const uint64*, const uint32*> filter_type;
    typedef typename filter_type::hit_type      hit_type;
    typedef typename filter_type::diagonal_type diagonal_type;

    host_index_type ix;
    ix = d_ix;                                          // the cross-system copy
    copy_index(ix, o);
    thrust::host_vector<uint2> ranges(n_queries);
    thrust::transform(h_queries, h_queries + n_queries, ranges.begin(), plain_view(ix));
    to_host(o.ranges, ranges, n_queries);

    filter_type filter;
    const uint64 total = filter.rank(ix, n_queries, h_queries, h_indices);
    *o.total = total;
    if (total != filter.n_hits() || total > o.hits_capacity) return -2;
    std::vector<hit_type> hits(total);
    const uint64 cut = total / 3u;
    filter.locate(0u, cut, hits.begin());
    filter.locate(cut, total, hits.begin() + cut);
    if (total) memcpy(o.hits, hits.data(), total * sizeof(hit_type));
    std::vector<diagonal_type> merged(total);
    std::vector<uint32>        counts(total);
    *o.n_merged = filter.merge(interval, uint32(total), hits.begin(), merged.begin(), counts.begin());
    if (*o.n_merged) { memcpy(o.merged, merged.data(), *o.n_merged * sizeof(diagonal_type)); memcpy(o.counts, counts.data(), *o.n_merged * 4u); }
    return 0;
}

template <bool BE>
static int run_string(const uint32* h_words, const uint32 n_words, const uint8* h_symbols, const uint32 len, const uint32 q, const uint32 ql, const int mode,
                      const uint64* h_queries, const uint32* h_indices, const uint32 n_queries, const uint32 interval, const Outputs& o)
{
    QGramIndexDevice ix;
    thrust::device_vector<uint32> d_words(h_words, h_words + n_words);
    thrust::device_vector<uint8>  d_symbols(h_symbols, h_symbols + len);
    if (mode == BYTES_DEVICE_GENERIC)
    {
        // 2-bit symbols kept one a byte: any iterator builds an index
        ix.build(q, 2u, len, (const uint8*)thrust::raw_pointer_cast(d_symbols.data()), ql);
        if (strcmp(ix.last_path(), "generic") != 0) return -6;
    }
    else
    {
        typedef PackedStream<const uint32*, uint8, 2, BE, uint64> stream_type;
        ix.build(q, 2u, len, stream_type(thrust::raw_pointer_cast(d_words.data())), ql);
        if (strcmp(ix.last_path(), "tuned") != 0) return -6;
        // generate_qgrams at the first and the last position: the q-grams of the index's coordinates must be sorted
        thrust::device_vector<uint64> sorted(ix.n_qgrams);
        generate_qgrams(q, 2u, len, stream_type(thrust::raw_pointer_cast(d_words.data())), ix.n_qgrams, ix.index.begin(), sorted.begin());
        if (!thrust::is_sorted(sorted.begin(), sorted.end())) return -7;
    }
    if (mode == PACKED_HOST) return host_filter<QGramIndexHost>(ix, h_queries, h_indices, n_queries, interval, o);
    copy_index(ix, o);
    return device_filter(ix, h_queries, h_indices, n_queries, interval, mode == BYTES_DEVICE_GENERIC, mode == BYTES_DEVICE_GENERIC ? "generic" : "tuned", o);
}

template <bool BE>
static int run_set(const uint32* h_words, const uint32 n_words, const uint8* h_symbols, const uint32 n_symbols, const uint64* h_offsets, const uint32 n_strings,
                   const uint32 q, const uint32 ql, const uint32 seed_interval, const int mode,
                   const uint64* h_queries, const uint32* h_indices, const uint32 n_queries, const uint32 interval, const Outputs& o)
{
    QGramSetIndexDevice ix;
    thrust::device_vector<uint32> d_words(h_words, h_words + n_words);
    thrust::device_vector<uint8>  d_symbols(h_symbols, h_symbols + n_symbols);
    thrust::device_vector<uint64> d_offsets(h_offsets, h_offsets + n_strings + 1u);
    if (mode == BYTES_DEVICE_GENERIC)
    {
        typedef ConcatenatedStringSet<const uint8*, const uint64*> string_set_type;
        const string_set_type set(n_strings, thrust::raw_pointer_cast(d_symbols.data()), thrust::raw_pointer_cast(d_offsets.data()));
        ix.build(q, 2u, set, uniform_seeds_functor<>(q, seed_interval), ql);
        if (strcmp(ix.last_path(), "generic") != 0) return -6;
    }
    else
    {
        typedef PackedStream<const uint32*, uint8, 2, BE, uint64> stream_type;
        typedef ConcatenatedStringSet<stream_type, uint64*>       string_set_type;
        const string_set_type set(n_strings, stream_type(thrust::raw_pointer_cast(d_words.data())), thrust::raw_pointer_cast(d_offsets.data()));
        if (seed_interval == 1u) ix.build(q, 2u, set, ql);                     // the overload without a seeder
        else                     ix.build(q, 2u, set, uniform_seeds_functor<>(q, seed_interval), ql);
        if (strcmp(ix.last_path(), "tuned") != 0) return -6;
    }
    if (mode == PACKED_HOST) return host_filter<QGramSetIndexHost>(ix, h_queries, h_indices, n_queries, interval, o);
    copy_index(ix, o);
    return device_filter(ix, h_queries, h_indices, n_queries, interval, mode == BYTES_DEVICE_GENERIC, mode == BYTES_DEVICE_GENERIC ? "generic" : "tuned", o);
}

API int compat_qgram_string(const uint32* h_words, uint32 n_words, int big_endian, const uint8* h_symbols, uint32 len, uint32 q, uint32 ql, int mode,
                            const uint64* h_queries, const uint32* h_indices, uint32 n_queries, uint32 interval, const Outputs* out)
{
    try {
        return big_endian ? run_string<true>(h_words, n_words, h_symbols, len, q, ql, mode, h_queries, h_indices, n_queries, interval, *out)
                          : run_string<false>(h_words, n_words, h_symbols, len, q, ql, mode, h_queries, h_indices, n_queries, interval, *out);
    } catch (const std::exception& e) { fprintf(stderr, "compat_qgram_string: %s\n", e.what()); return -1; }
}

API int compat_qgram_set(const uint32* h_words, uint32 n_words, int big_endian, const uint8* h_symbols, uint32 n_symbols, const uint64* h_offsets, uint32 n_strings,
                         uint32 q, uint32 ql, uint32 seed_interval, int mode, const uint64* h_queries, const uint32* h_indices, uint32 n_queries, uint32 interval,
                         const Outputs* out)
{
    try {
        return big_endian ? run_set<true>(h_words, n_words, h_symbols, n_symbols, h_offsets, n_strings, q, ql, seed_interval, mode, h_queries, h_indices, n_queries, interval, *out)
                          : run_set<false>(h_words, n_words, h_symbols, n_symbols, h_offsets, n_strings, q, ql, seed_interval, mode, h_queries, h_indices, n_queries, interval, *out);
    } catch (const std::exception& e) { fprintf(stderr, "compat_qgram_set: %s\n", e.what()); return -1; }
}
