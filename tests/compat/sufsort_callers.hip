// tests/compat/sufsort_callers.hip -- callers of the suffix sorting front door written in the reference's vocabulary
// (nvbio/sufsort/sufsort.h, as sufsort-test/sufsort_test.cu and examples/waveletfm/waveletfm.cu use it): cuda::suffix_sort over a
// packed device string into a thrust device vector, cuda::bwt into a packed device stream, cuda::find_primary.  It includes the
// reference's header names and is compiled with `hipcc -I include/nvbio_hip/compat`.  The extern "C" entry points take and return
// host memory so that the Python tests can drive it.
#include <nvbio/basic/types.h>
#include <nvbio/basic/packedstream.h>
#include <nvbio/basic/vector.h>
#include <nvbio/sufsort/sufsort.h>
#include <thrust/device_vector.h>
#include <thrust/copy.h>
#include <stdio.h>
#include <exception>

using namespace nvbio;

#define API extern "C" __attribute__((visibility("default")))

typedef PackedStream<uint32*, uint8, 2, true>        packed_stream_type;
typedef PackedStream<const uint32*, uint8, 2, true>  const_packed_stream_type;
typedef PackedStream<const uint32*, uint8, 2, false> const_le_stream_type;

// ---- the packed string of n symbols in `words` (big-endian): its suffix array, BWT and primary through the three entry points
API int compat_sufsort(const uint32* h_words, uint32 n, uint32* out_sa, uint32* out_bwt_words, uint32* out_primary, uint32* out_found_primary)
{
    try {
        const uint32 n_words = (n + 15u) / 16u;
        thrust::device_vector<uint32> d_string(h_words, h_words + n_words);
        thrust::device_vector<uint32> d_sa(n + 1u);
        thrust::device_vector<uint32> d_bwt((n + 1u + 15u) / 16u, 0u);

        BWTParams params;
        packed_stream_type d_packed_string(nvbio::plain_view(d_string));

        cuda::suffix_sort(n, d_packed_string, d_sa.begin(), &params);
        thrust::copy(d_sa.begin(), d_sa.end(), out_sa);

        packed_stream_type d_packed_bwt(nvbio::plain_view(d_bwt));
        *out_primary = cuda::bwt(n, d_packed_string, d_packed_bwt, &params);
        thrust::copy(d_bwt.begin(), d_bwt.begin() + n_words, out_bwt_words);

        *out_found_primary = cuda::find_primary(n, const_packed_stream_type(nvbio::plain_view(d_string)));
        return 0;
    } catch (const std::exception& e) { fprintf(stderr, "compat_sufsort: %s\n", e.what()); return -1; }
}

// ---- the same through the generic path: a little-endian string that starts `skip` symbols into its words, a suffix array of 64-bit
// entries, and the BWT as one byte a symbol and into a packed stream that starts 3 symbols into its first word
API int compat_sufsort_generic(const uint32* h_le_words, uint32 skip, uint32 n, unsigned long long* out_sa, uint8* out_bwt, uint32* out_bwt_words3,
                               uint32* out_primary)
{
    try {
        const uint32 n_words = (skip + n + 15u) / 16u;
        thrust::device_vector<uint32> d_string(h_le_words, h_le_words + n_words);
        thrust::device_vector<unsigned long long> d_sa(n + 1u);
        thrust::device_vector<uint8>  d_bwt(n);
        thrust::device_vector<uint32> d_bwt3((3u + n + 15u) / 16u, 0xFFFFFFFFu);

        const const_le_stream_type d_packed_string = const_le_stream_type(nvbio::plain_view(d_string)) + skip;

        cuda::suffix_sort(n, d_packed_string, thrust::raw_pointer_cast(d_sa.data()), (BWTParams*)NULL);
        thrust::copy(d_sa.begin(), d_sa.end(), out_sa);

        *out_primary = cuda::bwt(n, d_packed_string, thrust::raw_pointer_cast(d_bwt.data()), (BWTParams*)NULL);
        thrust::copy(d_bwt.begin(), d_bwt.end(), out_bwt);

        const uint32 again = cuda::bwt(n, d_packed_string, packed_stream_type(nvbio::plain_view(d_bwt3)) + 3, (BWTParams*)NULL);
        thrust::copy(d_bwt3.begin(), d_bwt3.end(), out_bwt_words3);
        return again == *out_primary ? 0 : -2;
    } catch (const std::exception& e) { fprintf(stderr, "compat_sufsort_generic: %s\n", e.what()); return -1; }
}
