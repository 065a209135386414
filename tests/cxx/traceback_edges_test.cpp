// The C++ host layer's traceback batch classes (include/nvbio_hip/alignment.h) for the linear-gap aligners: SmithWatermanAligner over a
// SimpleSmithWatermanScheme whose deletion and insertion differ, and EditDistanceAligner.  One C entry point, called by
// tests/test_traceback_edges_gpu.py, runs a batch through BatchedBandedAlignmentTraceback<15> and BatchedAlignmentTraceback and returns
// a checksum of each class's outputs; the caller computes the same checksum from the oracle's tracebacks.
#include <cstdio>
#include <exception>
#include <vector>
#include "nvbio_hip/alignment.h"

using namespace nvbio;

namespace {

const uint32 BAND = 15;

// FNV-1a over 32-bit words: score, sink, source, cigar_len and the stored CIGAR words of every job, in job order
struct Checksum
{
    uint64 h;
    Checksum() : h(14695981039346656037ull) {}
    void add(const uint32 w) { h = (h ^ uint64(w)) * 1099511628211ull; }
};

struct Outputs
{
    hip::device_vector<int32>     score;
    hip::device_vector<uint32>    sink, source, len;
    hip::device_vector<io::Cigar> cigar;
    uint32 n, stride;
    Outputs(const uint32 _n, const uint32 _stride) : score(_n), sink(2 * size_t(_n)), source(2 * size_t(_n)), len(_n), cigar(size_t(_n) * _stride), n(_n), stride(_stride)
    {
        const std::vector<io::Cigar> zero(size_t(n) * stride, io::Cigar(0, 0));
        cigar.assign(zero.data(), zero.size());
    }
    aln::AlignmentArrays alignments() { const aln::AlignmentArrays a = { score.data(), source.data(), sink.data() }; return a; }
    aln::CigarArrays     cigars()     { const aln::CigarArrays c = { cigar.data(), stride, len.data() }; return c; }
    uint64 checksum() const
    {
        hip::synchronize();
        const std::vector<int32> s = score.to_host();
        const std::vector<uint32> k = sink.to_host(), o = source.to_host(), l = len.to_host();
        const std::vector<io::Cigar> c = cigar.to_host();
        Checksum sum;
        for (uint32 i = 0; i < n; ++i)
        {
            sum.add(uint32(s[i])); sum.add(k[2 * i]); sum.add(k[2 * i + 1]); sum.add(o[2 * i]); sum.add(o[2 * i + 1]); sum.add(l[i]);
            for (uint32 w = 0; w < std::min(l[i], stride); ++w)
                sum.add(uint32(c[size_t(i) * stride + w].m_type) | (uint32(c[size_t(i) * stride + w].m_len) << 2));
        }
        return sum.h;
    }
};

template <typename aligner_type>
void run(const aligner_type aligner, const std::vector<std::vector<uint8> >& patterns, const std::vector<std::vector<uint8> >& texts,
         const uint32 stride, uint64* sums)
{
    typedef aln::PackedTracebackStream<aligner_type, PackedStringSetView<4, true>, PackedStringSetView<2, true> > stream_type;
    const uint32 n = uint32(patterns.size());
    uint32 maxP = 0, maxT = 0;
    for (uint32 i = 0; i < n; ++i) { maxP = std::max(maxP, uint32(patterns[i].size())); maxT = std::max(maxT, uint32(texts[i].size())); }
    PackedStringSetDevice<4, true> d_patterns(patterns);
    PackedStringSetDevice<2, true> d_texts(texts);
    {
        typedef aln::BatchedBandedAlignmentTraceback<BAND, 32u, stream_type> batch_type;
        Outputs out(n, stride);
        const uint64 temp_size = batch_type::max_temp_storage(maxP, maxT, n);
        hip::device_vector<uint8> temp(temp_size ? temp_size : 1);
        batch_type batch;
        batch.enact(stream_type(aligner, d_patterns.view(), d_texts.view(), out.alignments(), out.cigars(), maxP, maxT), temp_size, temp.data());
        sums[0] = out.checksum();
    }
    {
        typedef aln::BatchedAlignmentTraceback<32u, stream_type> batch_type;
        Outputs out(n, stride);
        const uint64 temp_size = batch_type::max_temp_storage(maxP, maxT, n);
        hip::device_vector<uint8> temp(temp_size ? temp_size : 1);
        batch_type batch;
        batch.enact(stream_type(aligner, d_patterns.view(), d_texts.view(), out.alignments(), out.cigars(), maxP, maxT), temp_size, temp.data());
        sums[1] = out.checksum();
    }
}

template <aln::AlignmentType TYPE>
void run_type(const int32 kind, const int32* scheme, const std::vector<std::vector<uint8> >& patterns, const std::vector<std::vector<uint8> >& texts,
              const uint32 stride, uint64* sums)
{
    if (kind == 0) run(aln::make_smith_waterman_aligner<TYPE>(aln::SimpleSmithWatermanScheme(scheme[0], scheme[1], scheme[2], scheme[3])), patterns, texts, stride, sums);
    else           run(aln::make_edit_distance_aligner<TYPE>(), patterns, texts, stride, sums);
}

} // namespace

// kind 0: SmithWatermanAligner with scheme = {match, mismatch, deletion, insertion}; kind 1: EditDistanceAligner.  String i of each set
// is sym[begin[i] .. begin[i] + len[i]).  sums[0] / sums[1]: the checksums of the banded and the full-matrix class's outputs.
// Returns 0 when both equal `expect`, 1 when one differs, -1 on an exception (its text goes to stderr).
extern "C" __attribute__((visibility("default")))
int nvbio_traceback_edges_check(int32 kind, int32 type, const int32* scheme, uint32 n,
                                const uint8* pat_sym, const uint64* pat_begin, const uint32* pat_len,
                                const uint8* txt_sym, const uint64* txt_begin, const uint32* txt_len,
                                uint32 cigar_stride, const uint64* expect, uint64* sums)
{
    try
    {
        std::vector<std::vector<uint8> > patterns(n), texts(n);
        for (uint32 i = 0; i < n; ++i) {
            patterns[i].assign(pat_sym + pat_begin[i], pat_sym + pat_begin[i] + pat_len[i]);
            texts[i].assign(txt_sym + txt_begin[i], txt_sym + txt_begin[i] + txt_len[i]);
        }
        switch (type) {
        case aln::GLOBAL:      run_type<aln::GLOBAL>(kind, scheme, patterns, texts, cigar_stride, sums); break;
        case aln::LOCAL:       run_type<aln::LOCAL>(kind, scheme, patterns, texts, cigar_stride, sums); break;
        case aln::SEMI_GLOBAL: run_type<aln::SEMI_GLOBAL>(kind, scheme, patterns, texts, cigar_stride, sums); break;
        default: return -1;
        }
        return (sums[0] == expect[0] && sums[1] == expect[1]) ? 0 : 1;
    }
    catch (const std::exception& e)
    {
        fprintf(stderr, "nvbio_traceback_edges_check: %s\n", e.what());
        return -1;
    }
}
