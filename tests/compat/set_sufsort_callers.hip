// tests/compat/set_sufsort_callers.hip -- callers of the string-set half of the suffix sorting front door, written in the reference's
// vocabulary (nvbio/sufsort/sufsort.h): cuda::suffix_sort over a packed-concatenated device string set with a handler that receives
// device arrays, and cuda::bwt<SYMBOL_SIZE,BIG_ENDIAN> with a handler derived from SetBWTHandler that receives host arrays.  It
// includes the reference's header names and is compiled with `hipcc -I include/nvbio_hip/compat`.  The extern "C" entry points take
// and return host memory so that the Python tests can drive it.
#include <nvbio/basic/types.h>
#include <nvbio/basic/packedstream.h>
#include <nvbio/basic/vector.h>
#include <nvbio/strings/string_set.h>
#include <nvbio/sufsort/sufsort.h>
#include <nvbio/sufsort/sufsort_utils.h>
#include <thrust/device_vector.h>
#include <thrust/copy.h>
#include <stdio.h>
#include <exception>
#include <vector>

using namespace nvbio;

#define API extern "C" __attribute__((visibility("default")))

// keeps every batch it is given, one after another
struct CollectSuffixes
{
    void process(const uint32 n_suffixes, const uint32* d_suffixes, const uint32* d_string_ids, const uint32* d_cum_lengths)
    {
        const size_t old = suffixes.size();
        suffixes.resize(old + n_suffixes);
        string_ids.resize(n_suffixes);
        cum_lengths.resize(n_strings);
        typedef thrust::device_ptr<const uint32> ptr;
        thrust::copy(ptr(d_suffixes), ptr(d_suffixes) + n_suffixes, suffixes.begin() + old);
        thrust::copy(ptr(d_string_ids), ptr(d_string_ids) + n_suffixes, string_ids.begin());
        thrust::copy(ptr(d_cum_lengths), ptr(d_cum_lengths) + n_strings, cum_lengths.begin());
        ++calls;
    }
    uint32 n_strings = 0, calls = 0;
    std::vector<uint32> suffixes, string_ids, cum_lengths;
};

struct CollectBWT : public SetBWTHandler
{
    void process(const uint32 n_suffixes, const uint8* bwt, const uint32 n_dollars, const uint64* dollar_pos, const uint64* dollar_ids)
    {
        symbols.insert(symbols.end(), bwt, bwt + n_suffixes);
        pos.insert(pos.end(), dollar_pos, dollar_pos + n_dollars);
        ids.insert(ids.end(), dollar_ids, dollar_ids + n_dollars);
        ++calls;
    }
    uint32 calls = 0;
    std::vector<uint8>  symbols;
    std::vector<uint64> pos, ids;
};

template <bool BE>
static int run(const uint32* h_words, const uint32 n_words, const uint32 skip, const uint64* h_offsets, const uint32 n_strings, const uint32 n_suffixes,
               uint32* out_suffixes, uint32* out_string_ids, uint32* out_cum, uint8* out_bwt, uint64* out_dollar_pos, uint64* out_dollar_ids)
{
    typedef PackedStream<const uint32*, uint8, 2, BE, uint64> stream_type;
    typedef ConcatenatedStringSet<stream_type, uint64*>       string_set_type;

    thrust::device_vector<uint32> d_words(h_words, h_words + n_words);
    thrust::device_vector<uint64> d_offsets(h_offsets, h_offsets + n_strings + 1u);

    // the strings start `skip` symbols into the words
    const stream_type     d_stream = stream_type(thrust::raw_pointer_cast(d_words.data())) + skip;
    const string_set_type d_set(n_strings, d_stream, thrust::raw_pointer_cast(d_offsets.data()));

    BWTParams params;
    CollectSuffixes sorted;
    sorted.n_strings = n_strings;
    cuda::suffix_sort(d_set, sorted, &params);
    if (sorted.calls == 0u || sorted.suffixes.size() != n_suffixes) return -2;
    std::copy(sorted.suffixes.begin(), sorted.suffixes.end(), out_suffixes);
    std::copy(sorted.string_ids.begin(), sorted.string_ids.end(), out_string_ids);
    std::copy(sorted.cum_lengths.begin(), sorted.cum_lengths.end(), out_cum);

    CollectBWT collected;
    cuda::bwt<2, BE>(d_set, collected);
    if (collected.calls == 0u || collected.symbols.size() != n_suffixes || collected.pos.size() != n_strings || collected.ids.size() != n_strings) return -3;
    std::copy(collected.symbols.begin(), collected.symbols.end(), out_bwt);
    std::copy(collected.pos.begin(), collected.pos.end(), out_dollar_pos);
    std::copy(collected.ids.begin(), collected.ids.end(), out_dollar_ids);
    return 0;
}

// ---- a concatenated set of n_strings 2-bit strings, offsets[0 .. n_strings], `skip` symbols into `words`: everything the two set
// overloads hand their handlers
API int compat_set_sufsort(const uint32* h_words, uint32 n_words, int big_endian, uint32 skip, const uint64* h_offsets, uint32 n_strings, uint32 n_suffixes,
                           uint32* out_suffixes, uint32* out_string_ids, uint32* out_cum, uint8* out_bwt, uint64* out_dollar_pos, uint64* out_dollar_ids)
{
    try {
        return big_endian ? run<true>(h_words, n_words, skip, h_offsets, n_strings, n_suffixes, out_suffixes, out_string_ids, out_cum, out_bwt, out_dollar_pos, out_dollar_ids)
                          : run<false>(h_words, n_words, skip, h_offsets, n_strings, n_suffixes, out_suffixes, out_string_ids, out_cum, out_bwt, out_dollar_pos, out_dollar_ids);
    } catch (const std::exception& e) { fprintf(stderr, "compat_set_sufsort: %s\n", e.what()); return -1; }
}

// ---- a 4-bit set is refused with an exception, as the plain overloads refuse wider alphabets
API int compat_set_bwt_4bit_throws(void)
{
    typedef PackedStream<const uint32*, uint8, 4, true, uint64> stream_type;
    typedef ConcatenatedStringSet<stream_type, uint64*>         string_set_type;
    thrust::device_vector<uint32> d_words(4, 0u);
    thrust::device_vector<uint64> d_offsets(2, 0u);
    d_offsets[1] = 8u;
    const string_set_type d_set(1u, stream_type(thrust::raw_pointer_cast(d_words.data())), thrust::raw_pointer_cast(d_offsets.data()));
    CollectBWT collected;
    try { cuda::bwt<4, true>(d_set, collected); } catch (const std::exception&) { return collected.calls == 0u ? 1 : -1; }
    return 0;
}
