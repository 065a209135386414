// tests/compat/hamming_callers.hip -- callers of aln::BatchedAlignmentScore over HammingDistanceAligner streams, written against the
// reference's documented stream concept (nvbio/alignment/batched.h:239-296) and compiled with `hipcc -I include/nvbio_hip/compat`:
//   * a stream of packed strings in place (reads 4 bits per base, big-endian; windows 2 bits per base, little-endian), trivial
//     qualities, SimpleSmithWatermanScheme -- PatternBlockingTag (the tuned kernel's order) and TextBlockingTag (generic lane);
//   * a stream shaped like nvBowtie's opposite-mate stream under --ungapped-mates: io::ReadStream views of stored reads (forward, or
//     reverse-complemented), their quality strings, a scheme of nvBowtie's concept, a genome window per job.
// The extern "C" entry points exist only so that tests/test_hamming_gpu.py can drive them.
#include <nvbio/basic/types.h>
#include <nvbio/basic/packedstream.h>
#include <nvbio/basic/packedstream_loader.h>
#include <nvbio/basic/vector_view.h>
#include <nvbio/basic/cuda/ldg.h>
#include <nvbio/io/utils.h>
#include <nvbio/io/sequence/sequence.h>
#include <nvbio/alignment/alignment.h>
#include <nvbio/alignment/batched.h>
#include <string.h>

using namespace nvbio;

// --------------------------------------------------------------------------------------------------------------------- packed strings
template <typename t_aligner_type>
struct PackedUngappedStream
{
    typedef t_aligner_type aligner_type;
    typedef cuda::ldg_pointer<uint32> word_iterator;
    typedef PackedStringLoader<word_iterator, io::SequenceDataTraits<DNA_N>::SEQUENCE_BITS, io::SequenceDataTraits<DNA_N>::SEQUENCE_BIG_ENDIAN, uncached_tag> read_loader_type;
    typedef PackedStringLoader<word_iterator, 2, false, uncached_tag>                                                                                            window_loader_type;
    typedef vector_view<typename read_loader_type::iterator>   read_string;
    typedef vector_view<typename window_loader_type::iterator> window_string;

    struct context_type { int32 min_score; aln::BestSink<int32> sink; };
    struct strings_type
    {
        read_loader_type            read_loader;
        window_loader_type          window_loader;
        read_string                 pattern;
        aln::trivial_quality_string quals;
        window_string               text;
    };

    PackedUngappedStream(aligner_type aligner, uint32 count, const uint32* read_offsets, const uint32* read_words, uint32 longest_read,
                         const uint32* window_offsets, const uint32* window_words, uint32 longest_window, const int32* thresholds, int32* scores, uint2* sinks)
        : m_aligner(aligner), m_count(count), m_read_offsets(read_offsets), m_reads(word_iterator(read_words)), m_longest_read(longest_read),
          m_window_offsets(window_offsets), m_windows(word_iterator(window_words)), m_longest_window(longest_window),
          m_thresholds(thresholds), m_scores(scores), m_sinks(sinks) {}

    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE const aligner_type& aligner() const { return m_aligner; }
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE uint32 max_pattern_length() const { return m_longest_read; }
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE uint32 max_text_length() const { return m_longest_window; }
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE uint32 size() const { return m_count; }
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE uint32 pattern_length(const uint32 i, context_type*) const { return m_read_offsets[i + 1] - m_read_offsets[i]; }
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE uint32 text_length(const uint32 i, context_type*) const { return m_window_offsets[i + 1] - m_window_offsets[i]; }
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE bool init_context(const uint32 i, context_type* context) const
    {
        context->min_score = m_thresholds ? m_thresholds[i] : Field_traits<int32>::min();
        return true;
    }
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE void load_strings(const uint32 i, const uint32 window_begin, const uint32 window_end, const context_type*, strings_type* strings) const
    {
        const uint32 r0 = m_read_offsets[i],   rn = m_read_offsets[i + 1] - r0;
        const uint32 w0 = m_window_offsets[i], wn = m_window_offsets[i + 1] - w0;
        strings->text    = window_string(wn, strings->window_loader.load(m_windows + w0, wn, make_uint2(window_begin, window_end), false));
        strings->pattern = read_string(rn, strings->read_loader.load(m_reads + r0, rn));
    }
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE void output(const uint32 i, const context_type* context) const { m_scores[i] = context->sink.score; m_sinks[i] = context->sink.sink; }

    aligner_type m_aligner; uint32 m_count;
    const uint32* m_read_offsets;   typename read_loader_type::input_iterator m_reads;     uint32 m_longest_read;
    const uint32* m_window_offsets; typename window_loader_type::input_iterator m_windows; uint32 m_longest_window;
    const int32* m_thresholds; int32* m_scores; uint2* m_sinks;
};

// --------------------------------------------------------------------------------------------------------------------- read views
struct PhredPenalty
{
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE PhredPenalty(const int at0 = 0, const int at40 = 0) : lo(at0), hi(at40) {}
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE int operator()(const int phred) const { return lo + int((float)(phred < 40 ? phred : 40) / 40.0f * (hi - lo)); }
    int lo, hi;
};
struct FixedBonus
{
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE FixedBonus(const int v = 0) : value(v) {}
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE int operator()(const int) const { return value; }
    int value;
};
/// what an ungapped aligner reads of a scheme of nvBowtie's concept (scoring.h:283-293), and the typedefs that mark the concept
struct MateScheme
{
    typedef FixedBonus   match_cost_function;
    typedef PhredPenalty mismatch_cost_function;
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE int32 match(const uint8 q = 0) const { return bonus(q); }
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE int32 mismatch(const uint8 q = 0) const { return -penalty(q); }
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE int32 mismatch(const uint8, const uint8, const uint8 q = 0) const { return -penalty(q); }
    FixedBonus bonus; PhredPenalty penalty;
};
/// 4-bit big-endian reads with a quality byte per stored symbol: what io::ReadLoader loads from
struct StoredReads
{
    static const uint32 SEQUENCE_BITS       = io::SequenceDataTraits<DNA_N>::SEQUENCE_BITS;
    static const bool   SEQUENCE_BIG_ENDIAN = io::SequenceDataTraits<DNA_N>::SEQUENCE_BIG_ENDIAN;
    typedef cuda::ldg_pointer<uint32>  sequence_storage_iterator;
    typedef cuda::ldg_pointer<uint8>   qual_storage_iterator;
    typedef PackedStream<sequence_storage_iterator, uint8, SEQUENCE_BITS, SEQUENCE_BIG_ENDIAN> sequence_stream_type;
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE sequence_stream_type  sequence_stream() const { return sequence_stream_type(sequence_storage_iterator(words)); }
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE qual_storage_iterator qual_stream()     const { return qual_storage_iterator(quals); }
    const uint32* words; const uint8* quals; const uint32* offsets;
};

template <typename Aligner>
struct MateStream
{
    typedef Aligner aligner_type;
    typedef lmem_cache_tag<64> cache_tag;
    typedef ReadLoader<StoredReads, cache_tag>                                     read_loader;
    typedef PackedStringLoader<cuda::ldg_pointer<uint32>, 2, true, cache_tag>      genome_loader;
    typedef PackedStream<cuda::ldg_pointer<uint32>, uint8, 2, true>                genome_type;

    struct context_type { aln::BestSink<int32> sink; int32 min_score; uint2 stored; bool reverse; uint32 lo, hi; };
    struct strings_type
    {
        typename read_loader::string_type                        pattern;
        typename read_loader::string_type::qual_string_type      quals;
        vector_view<typename genome_loader::iterator>            text;
        read_loader   loads_read;
        genome_loader loads_genome;
    };

    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE const Aligner& aligner() const { return al; }
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE uint32 size() const { return n; }
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE uint32 max_pattern_length() const { return longest; }
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE uint32 max_text_length() const { return widest; }
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE uint32 pattern_length(const uint32, const context_type* job) const { return job->stored.y - job->stored.x; }
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE uint32 text_length(const uint32, const context_type* job) const { return job->hi - job->lo; }
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE bool init_context(const uint32 i, context_type* job) const
    {
        job->stored = make_uint2(reads.offsets[i], reads.offsets[i + 1]);
        job->reverse = (i & flip) != 0u;                        // flip = 1: odd jobs look at the reverse complement of the stored read
        job->lo = windows[i].x; job->hi = windows[i].y;
        job->min_score = thresholds[i];
        job->sink = aln::BestSink<int32>();
        return job->hi > job->lo;                               // an empty window means "do not look": output as it is
    }
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE void load_strings(const uint32, const uint32, const uint32, const context_type* job, strings_type* s) const
    {
        s->pattern = s->loads_read.load(reads, job->stored, job->reverse ? REVERSE : FORWARD, job->reverse ? COMPLEMENT : STANDARD);
        s->quals   = s->pattern.qualities();
        const uint32 span = job->hi - job->lo;
        s->text    = vector_view<typename genome_loader::iterator>(span, s->loads_genome.load(genome + job->lo, span));
    }
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE void output(const uint32 i, const context_type* job) const { scores[i] = job->sink.score; sinks[i] = job->sink.sink; }

    Aligner al; uint32 n; uint32 flip; StoredReads reads; uint32 longest; genome_type genome; const uint2* windows; uint32 widest; const int32* thresholds; int32* scores; uint2* sinks;
};

// --------------------------------------------------------------------------------------------------------------------- entry points
#define API extern "C" __attribute__((visibility("default")))

template <typename F> static const char* with_type(const int type, F f)
{
    if (type == 0) return f(std::integral_constant<aln::AlignmentType, aln::GLOBAL>());
    if (type == 1) return f(std::integral_constant<aln::AlignmentType, aln::LOCAL>());
    return f(std::integral_constant<aln::AlignmentType, aln::SEMI_GLOBAL>());
}
template <typename stream_type>
static const char* enact(const stream_type& stream)
{
    aln::BatchedAlignmentScore<stream_type, aln::DeviceThreadScheduler> batch;
    batch.enact(stream, 0, NULL);
    if (hipDeviceSynchronize() != hipSuccess) return "error";
    return batch.last_path();
}

/// packed strings in place; text_blocking selects TextBlockingTag.  path: 16 bytes, which execution ran
API int hamming_packed(int type, int text_blocking, int match, int mismatch, unsigned n, const unsigned* read_offsets, const unsigned* reads, unsigned longest_read,
                       const unsigned* window_offsets, const unsigned* windows, unsigned longest_window, const int* thresholds, int* scores, unsigned* sinks, char* path)
{
    try {
        const aln::SimpleSmithWatermanScheme w(match, mismatch, -1000, -1000);
        const char* p = with_type(type, [&](auto T) -> const char* {
            const aln::AlignmentType TYPE = decltype(T)::value;
            typedef aln::HammingDistanceAligner<TYPE, aln::SimpleSmithWatermanScheme>                       pattern_blocking;
            typedef aln::HammingDistanceAligner<TYPE, aln::SimpleSmithWatermanScheme, aln::TextBlockingTag> text_blocking_aligner;
            static_assert(aln::priv::recognised< PackedUngappedStream<pattern_blocking> >::zero_copy, "packed ungapped streams run in place on the tuned kernel");
            static_assert(!aln::priv::recognised< PackedUngappedStream<text_blocking_aligner> >::value, "text blocking stays on the generic lane");
            if (text_blocking)
                return enact(PackedUngappedStream<text_blocking_aligner>(text_blocking_aligner(w), n, read_offsets, reads, longest_read, window_offsets, windows, longest_window, thresholds, scores, (uint2*)sinks));
            return enact(PackedUngappedStream<pattern_blocking>(aln::make_hamming_distance_aligner<TYPE>(w), n, read_offsets, reads, longest_read, window_offsets, windows, longest_window, thresholds, scores, (uint2*)sinks));
        });
        strncpy(path, p, 15); path[15] = 0;
        return 0;
    } catch (const std::exception& e) { fprintf(stderr, "hamming_packed: %s\n", e.what()); return -1; }
}

/// read views with qualities against genome windows: job i = stored read i (flip_odd and odd i: its reverse complement) on window windows[i] = (lo, hi)
API int hamming_views(int type, int flip_odd, int match, int mmp_min, int mmp_max, unsigned n, const unsigned* read_offsets, const unsigned* read_words, const unsigned char* quals,
                      unsigned longest, const unsigned* genome_words, const unsigned* windows, unsigned widest, const int* thresholds, int* scores, unsigned* sinks, char* path)
{
    try {
        MateScheme s; s.bonus = FixedBonus(match); s.penalty = PhredPenalty(mmp_min, mmp_max);
        const char* p = with_type(type, [&](auto T) -> const char* {
            const aln::AlignmentType TYPE = decltype(T)::value;
            typedef aln::HammingDistanceAligner<TYPE, MateScheme> aligner_type;
            typedef MateStream<aligner_type> stream_type;
            static_assert(aln::priv::recognised<stream_type>::staged && aln::priv::recognised<stream_type>::stage_quals, "a stream of read views under a quality scheme is recognised");
            stream_type st = { aligner_type(s), n, flip_odd ? 1u : 0u, { read_words, quals, read_offsets }, longest, typename stream_type::genome_type(cuda::ldg_pointer<uint32>(genome_words)),
                               (const uint2*)windows, widest, thresholds, scores, (uint2*)sinks };
            return enact(st);
        });
        strncpy(path, p, 15); path[15] = 0;
        return 0;
    } catch (const std::exception& e) { fprintf(stderr, "hamming_views: %s\n", e.what()); return -1; }
}
