// tests/cxx/sufsort_shim.cpp -- the C++ host layer's suffix_sort / bwt (include/nvbio_hip/sufsort.h) behind one C entry point that
// tests/test_sufsort_gpu.py calls.  g++, no HIP.
#include "nvbio_hip/sufsort.h"
#include <stdio.h>
#include <exception>
#include <vector>

using namespace nvbio;

/// the text's words in host memory -> its suffix array, BWT words, primary and sampled suffix array, through device vectors
template <bool BE>
static int run(const unsigned* h_words, unsigned long long n, unsigned sa_int, unsigned* out_sa, unsigned* out_bwt_words, unsigned* out_primary, unsigned* out_ssa)
{
    hip::device_vector<uint32> words(std::vector<uint32>(h_words, h_words + (n + 15u) / 16u));
    const hip::PackedTextView<BE> text(words.data(), n);
    hip::device_vector<uint32> sa;
    hip::device_vector<uint8>  temp;
    hip::suffix_sort(text, sa, temp);
    if (sa.size() != n + 1u) return -2;
    hip_check(nvbio_hip_memcpy(out_sa, sa.data(), (n + 1u) * 4u, 2, nullptr), "nvbio_hip_memcpy");
    hip::BWTResult r;
    hip::bwt(text, sa_int, r, temp);                  // the same scratch, grown
    if (r.sa.size() != 0u || r.ssa.size() != (n + sa_int) / sa_int) return -3;
    hip_check(nvbio_hip_memcpy(out_bwt_words, r.bwt_words.data(), r.bwt_words.size() * 4u, 2, nullptr), "nvbio_hip_memcpy");
    hip_check(nvbio_hip_memcpy(out_ssa, r.ssa.data(), r.ssa.size() * 4u, 2, nullptr), "nvbio_hip_memcpy");
    hip_check(nvbio_hip_stream_synchronize(nullptr), "nvbio_hip_stream_synchronize");
    *out_primary = r.primary;
    return 0;
}

extern "C" __attribute__((visibility("default")))
int sufsort_host_layer(const unsigned* h_words, int big_endian, unsigned long long n, unsigned sa_int, unsigned* out_sa, unsigned* out_bwt_words,
                       unsigned* out_primary, unsigned* out_ssa)
{
    try {
        return big_endian ? run<true>(h_words, n, sa_int, out_sa, out_bwt_words, out_primary, out_ssa)
                          : run<false>(h_words, n, sa_int, out_sa, out_bwt_words, out_primary, out_ssa);
    } catch (const std::exception& e) { fprintf(stderr, "sufsort_host_layer: %s\n", e.what()); return -1; }
}
