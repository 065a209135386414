// tests/cxx/hamming_shim.cpp -- the C++ host layer's ungapped aligner (include/nvbio_hip/alignment.h: HammingDistanceAligner,
// batch_alignment_score / BatchedAlignmentScore) behind one C entry point that tests/test_hamming_gpu.py calls.  g++, no HIP.
#include "nvbio_hip/alignment.h"
#include <stdio.h>
#include <exception>
#include <type_traits>

using namespace nvbio;

namespace {
struct Set
{
    nvbio_hip_string_set s; uint32 n;
    nvbio_hip_string_set abi() const { return s; }
    uint32 size() const { return n; }
};
template <aln::AlignmentType TYPE>
int run(const int match, const int mismatch, const int use_quals, const int mmp_min, const int mmp_max, const Set& p, const uint8* quals, const uint64 n_quals, const Set& t,
        const uint32 maxP, const uint32 maxT, const int32* min_score, int32* score, uint32* sink, uint8* ok)
{
    const aln::BestSinkArrays sinks = { score, sink };
    if (!use_quals)
    {
        const auto aligner = aln::make_hamming_distance_aligner<TYPE>(aln::SimpleSmithWatermanScheme(match, mismatch, -1000, -1000));
        if (!min_score && !ok) { aln::batch_alignment_score(aligner, p, t, sinks, aln::DeviceThreadScheduler(), maxP, maxT); return 0; }
        typedef aln::PackedAlignmentStream<std::decay_t<decltype(aligner)>, Set, Set> stream_type;
        aln::BatchedAlignmentScore<stream_type> batch;
        batch.enact(stream_type(aligner, p, t, sinks, maxP, maxT), 0u, nullptr, min_score, ok);
        return 0;
    }
    aln::SmithWatermanScoringScheme scheme; scheme.m_match = match; scheme.m_mmp_min = mmp_min; scheme.m_mmp_max = mmp_max;
    const auto aligner = aln::make_hamming_distance_aligner<TYPE>(scheme);
    typedef aln::PackedAlignmentStream<std::decay_t<decltype(aligner)>, Set, Set> stream_type;
    aln::BatchedAlignmentScore<stream_type> batch;
    batch.enact(stream_type(aligner, p, t, sinks, maxP, maxT), 0u, nullptr, min_score, ok, nullptr, quals, n_quals);
    return 0;
}
}

extern "C" __attribute__((visibility("default")))
int hamming_host_class(int type, int match, int mismatch, int use_quals, int mmp_min, int mmp_max, const nvbio_hip_string_set* patterns, const unsigned char* quals,
                       unsigned long long n_quals, const nvbio_hip_string_set* texts, unsigned n, unsigned max_pattern_len, unsigned max_text_len,
                       const int* min_score, int* score, unsigned* sink, unsigned char* ok)
{
    try {
        const Set p = { *patterns, n }, t = { *texts, n };
        if (type == 0) return run<aln::GLOBAL>(match, mismatch, use_quals, mmp_min, mmp_max, p, quals, n_quals, t, max_pattern_len, max_text_len, min_score, score, sink, ok);
        if (type == 1) return run<aln::LOCAL>(match, mismatch, use_quals, mmp_min, mmp_max, p, quals, n_quals, t, max_pattern_len, max_text_len, min_score, score, sink, ok);
        return run<aln::SEMI_GLOBAL>(match, mismatch, use_quals, mmp_min, mmp_max, p, quals, n_quals, t, max_pattern_len, max_text_len, min_score, score, sink, ok);
    } catch (const std::exception& e) { fprintf(stderr, "hamming_host_class: %s\n", e.what()); return -1; }
}
