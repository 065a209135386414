// host_twins.hip -- the `_host` twins of the C-ABI: the reference's HostThreadScheduler / host_tag paths
// (nvbio/alignment/batched_banded_inl.h:97-128, batched_inl.h:236-300, nvbio/fmindex/filter_inl.h:200-259) for callers
// that cannot instantiate templates.  Same argument lists as the device entry points with HOST pointers everywhere and a
// thread count instead of a stream; OpenMP over independent jobs.  They instantiate the very templates the drop-in layer
// hands to hipcc callers (include/nvbio_hip/compat: the generic per-job DP and fm_index functions), on runtime-typed packed
// strings.  These are explicit entry points -- nothing in the device path ever falls back to them.
#define NVBIO_HIP_COMPAT_NO_TUNED 1
#include "common.h"
#include "fm_mem_args.h"
#include "../../include/nvbio_hip/compat/nvbio/alignment/alignment.h"
#include "../../include/nvbio_hip/compat/nvbio/fmindex/fmindex.h"
#include "../../include/nvbio_hip/compat/nvbio/fmindex/mem.h"
#include "../../include/nvbio_hip/compat/nvbio/basic/deinterleaved_iterator.h"
#if defined(_OPENMP)
#include <omp.h>
#endif

namespace {

using namespace nvbio;

/// a packed string whose symbol width and endianness are runtime values (the C-ABI's nvbio_hip_string_set)
struct RtString
{
    typedef uint8 value_type;
    const uint32* words; uint64 begin; uint32 len; uint32 bits; uint32 be;
    uint32 length() const { return len; }
    uint8 operator[](const uint32 i) const
    {
        const uint64 s = begin + i;
        const uint32 per = 32u / bits, k = uint32(s % per);
        const uint32 sh = be ? (32u - bits * (k + 1u)) : (bits * k);
        return uint8((words[s / per] >> sh) & ((1u << bits) - 1u));
    }
};
inline RtString string_of(const nvbio_hip_string_set* s, const uint32 i)
{
    const RtString r = { s->words, s->begin[i], s->length ? s->length[i] : s->fixed_length, s->bits, s->big_endian };
    return r;
}
inline bool valid_set(const nvbio_hip_string_set* s) { return s && s->words && s->begin && (s->bits == 2 || s->bits == 4 || s->bits == 8); }

template <typename F> inline int with_band(const uint32 band, F f)
{
    switch (band) {
        case 3:  return f(std::integral_constant<uint32, 3>());
        case 5:  return f(std::integral_constant<uint32, 5>());
        case 7:  return f(std::integral_constant<uint32, 7>());
        case 15: return f(std::integral_constant<uint32, 15>());
        case 31: return f(std::integral_constant<uint32, 31>());
    }
    return hipErrorNotSupported;
}
template <typename F> inline int with_type(const int32 type, F f)
{
    if (type == 0) return f(std::integral_constant<aln::AlignmentType, aln::GLOBAL>());
    if (type == 1) return f(std::integral_constant<aln::AlignmentType, aln::LOCAL>());
    if (type == 2) return f(std::integral_constant<aln::AlignmentType, aln::SEMI_GLOBAL>());
    return hipErrorInvalidValue;
}

template <typename make_aligner>
int banded_host(make_aligner make, const int32 type, const uint32 band, const nvbio_hip_string_set* patterns, const nvbio_hip_string_set* texts,
                const uint32 n, int32* out_score, uint32* out_sink, const int n_threads)
{
    if (!valid_set(patterns) || !valid_set(texts)) return hipErrorInvalidValue;
    if (n && (!out_score || !out_sink)) return hipErrorInvalidValue;
#if defined(_OPENMP)
    const int threads = n_threads > 0 ? n_threads : omp_get_max_threads();
#endif
    return with_band(band, [&](auto B) { return with_type(type, [&](auto T) {
        const auto aligner = make(T);
        #pragma omp parallel for schedule(dynamic, 256) num_threads(threads)
        for (int64 i = 0; i < int64(n); ++i)
        {
            aln::BestSink<int32> sink;
            aln::banded_alignment_score<decltype(B)::value>(aligner, string_of(patterns, uint32(i)), aln::trivial_quality_string(), string_of(texts, uint32(i)),
                                                            Field_traits<int32>::min(), sink);
            out_score[i] = sink.score; out_sink[2 * i] = sink.sink.x; out_sink[2 * i + 1] = sink.sink.y;
        }
        return int(hipSuccess);
    }); });
}

// the production index layout seen through the reference's own types (nvbio/io/fmindex/fmindex.h:159-174)
typedef deinterleaved_iterator<2, 0, const uint4*>               bwt_words_t;
typedef deinterleaved_iterator<2, 1, const uint4*>               occ_t;
typedef PackedStream<bwt_words_t, uint8, 2, true>                bwt_t;
typedef rank_dictionary<2, 64, bwt_t, occ_t, null_type>          dict_t;

/// SSA sampled every sa_int rows, sa_int a runtime power of two
struct RtSSA
{
    const uint32* ssa; uint32 sa_int;
    bool fetch(const uint32 i, uint32& r) const { if (i & (sa_int - 1u)) return false; r = ssa[i / sa_int]; return true; }
    bool has(const uint32 i) const { return (i & (sa_int - 1u)) == 0u; }
};
typedef fm_index<dict_t, RtSSA> fmi_t;
inline fmi_t host_index(const nvbio_hip_fmindex* f)
{
    const uint4* base = reinterpret_cast<const uint4*>(f->bwt_occ);
    const RtSSA ssa = { f->ssa, f->sa_int };
    return fmi_t(f->length, f->primary, f->L2, dict_t(bwt_t(bwt_words_t(base)), occ_t(base), null_type()), ssa);
}

} // namespace

NVB_API int nvbio_hip_banded_gotoh_score_host(const nvbio_hip_gotoh_scheme* scheme, int32_t type, uint32_t band_len,
                                              const nvbio_hip_string_set* patterns, const nvbio_hip_string_set* texts,
                                              uint32_t n, int32_t* out_score, uint32_t* out_sink, int32_t n_threads)
{
    if (!scheme) return hipErrorInvalidValue;
    const aln::SimpleGotohScheme sc(scheme->match, scheme->mismatch, scheme->gap_open, scheme->gap_ext);
    return banded_host([&](auto T) { return aln::make_gotoh_aligner<decltype(T)::value>(sc); }, type, band_len, patterns, texts, n, out_score, out_sink, n_threads);
}

NVB_API int nvbio_hip_banded_sw_score_host(const nvbio_hip_sw_scheme* scheme, int32_t type, uint32_t band_len,
                                           const nvbio_hip_string_set* patterns, const nvbio_hip_string_set* texts,
                                           uint32_t n, int32_t* out_score, uint32_t* out_sink, int32_t n_threads)
{
    if (!scheme) return hipErrorInvalidValue;
    const aln::SimpleSmithWatermanScheme sc(scheme->match, scheme->mismatch, scheme->deletion, scheme->insertion);
    return banded_host([&](auto T) { return aln::make_smith_waterman_aligner<decltype(T)::value>(sc); }, type, band_len, patterns, texts, n, out_score, out_sink, n_threads);
}

NVB_API int nvbio_hip_alignment_score_host(int32_t aligner, int32_t algorithm, const int32_t* scheme4, int32_t type,
                                           const nvbio_hip_string_set* patterns, const nvbio_hip_string_set* texts, const int32_t* min_score,
                                           uint32_t n, int32_t* out_score, uint32_t* out_sink, uint8_t* out_ok, int32_t n_threads)
{
    if (!scheme4 || !valid_set(patterns) || !valid_set(texts)) return hipErrorInvalidValue;
    if (n && (!out_score || !out_sink)) return hipErrorInvalidValue;
    if (aligner != NVBIO_HIP_GOTOH_ALIGNER && aligner != NVBIO_HIP_SW_ALIGNER) return hipErrorInvalidValue;
#if defined(_OPENMP)
    const int threads = n_threads > 0 ? n_threads : omp_get_max_threads();
#endif
    auto run = [&](const auto al) {
        #pragma omp parallel num_threads(threads)
        {
            std::vector<int16> column;
            #pragma omp for schedule(dynamic, 64)
            for (int64 i = 0; i < int64(n); ++i)
            {
                const RtString p = string_of(patterns, uint32(i)), t = string_of(texts, uint32(i));
                column.resize(2u * size_t(p.len > t.len ? p.len : t.len) + 8u);
                aln::BestSink<int32> sink;
                const bool ok = aln::alignment_score(al, p, aln::trivial_quality_string(), t, min_score ? min_score[i] : Field_traits<int32>::min(), sink, column.data());
                out_score[i] = sink.score; out_sink[2 * i] = sink.sink.x; out_sink[2 * i + 1] = sink.sink.y;
                if (out_ok) out_ok[i] = ok ? 1 : 0;
            }
        }
        return int(hipSuccess);
    };
    return with_type(type, [&](auto T) {
        const aln::AlignmentType TYPE = decltype(T)::value;
        if (aligner == NVBIO_HIP_GOTOH_ALIGNER) {
            const aln::SimpleGotohScheme sc(scheme4[0], scheme4[1], scheme4[2], scheme4[3]);
            return algorithm == NVBIO_HIP_TEXT_BLOCKING ? run(aln::make_gotoh_aligner<TYPE, aln::TextBlockingTag>(sc)) : run(aln::make_gotoh_aligner<TYPE, aln::PatternBlockingTag>(sc));
        }
        const aln::SimpleSmithWatermanScheme sc(scheme4[0], scheme4[1], scheme4[2], scheme4[3]);
        return algorithm == NVBIO_HIP_TEXT_BLOCKING ? run(aln::make_smith_waterman_aligner<TYPE, aln::TextBlockingTag>(sc)) : run(aln::make_smith_waterman_aligner<TYPE, aln::PatternBlockingTag>(sc));
    });
}

namespace {

/// nvBowtie's quality scheme as the ungapped aligner reads it: match(q), mismatch(r, q, qq) = the table's entry for the quality byte
struct QualLutScheme
{
    int32 m_match; const int32* lut;
    int32 match(const uint8 = 0) const { return m_match; }
    int32 mismatch(const uint8, const uint8, const uint8 qq) const { return lut[qq]; }
};
/// quality bytes of one pattern: quals[begin + j], the last byte for anything past the array (as the device entries clamp)
struct RtQuals
{
    const uint8* q; uint64 begin, n;
    uint8 operator[](const uint32 j) const { const uint64 k = begin + j; return q[k < n ? k : n - 1u]; }
};

template <typename scheme_type>
int hamming_host(const scheme_type& sc, const int32 algorithm, const int32 type, const nvbio_hip_string_set* patterns, const uint8* quals, const uint64 n_quals,
                 const nvbio_hip_string_set* texts, const int32* min_score, const uint32 n, int32* out_score, uint32* out_sink, uint8_t* out_ok, const int n_threads)
{
    if (!valid_set(patterns) || !valid_set(texts)) return hipErrorInvalidValue;
    if (n && (!out_score || !out_sink)) return hipErrorInvalidValue;
    if (algorithm != NVBIO_HIP_PATTERN_BLOCKING && algorithm != NVBIO_HIP_TEXT_BLOCKING) return hipErrorInvalidValue;
#if defined(_OPENMP)
    const int threads = n_threads > 0 ? n_threads : omp_get_max_threads();
#endif
    auto run = [&](const auto al) {
        #pragma omp parallel num_threads(threads)
        {
            std::vector<int16> column;
            #pragma omp for schedule(dynamic, 64)
            for (int64 i = 0; i < int64(n); ++i)
            {
                const RtString p = string_of(patterns, uint32(i)), t = string_of(texts, uint32(i));
                column.resize(size_t(p.len > t.len ? p.len : t.len) + 8u);
                aln::BestSink<int32> sink;
                const int32 ms = min_score ? min_score[i] : Field_traits<int32>::min();
                bool ok;
                if (quals) { const RtQuals q = { quals, p.begin, n_quals }; ok = aln::alignment_score(al, p, q, t, ms, sink, column.data()); }
                else       ok = aln::alignment_score(al, p, aln::trivial_quality_string(), t, ms, sink, column.data());
                out_score[i] = sink.score; out_sink[2 * i] = sink.sink.x; out_sink[2 * i + 1] = sink.sink.y;
                if (out_ok) out_ok[i] = ok ? 1 : 0;
            }
        }
        return int(hipSuccess);
    };
    return with_type(type, [&](auto T) {
        const aln::AlignmentType TYPE = decltype(T)::value;
        return algorithm == NVBIO_HIP_TEXT_BLOCKING ? run(aln::HammingDistanceAligner<TYPE, scheme_type, aln::TextBlockingTag>(sc))
                                                    : run(aln::HammingDistanceAligner<TYPE, scheme_type, aln::PatternBlockingTag>(sc));
    });
}

} // namespace

NVB_API int nvbio_hip_hamming_score_host(const nvbio_hip_sw_scheme* scheme, int32_t algorithm, int32_t type,
                                         const nvbio_hip_string_set* patterns, const nvbio_hip_string_set* texts, const int32_t* min_score,
                                         uint32_t n, int32_t* out_score, uint32_t* out_sink, uint8_t* out_ok, int32_t n_threads)
{
    if (!scheme) return hipErrorInvalidValue;
    const aln::SimpleSmithWatermanScheme sc(scheme->match, scheme->mismatch, scheme->deletion, scheme->insertion);
    return hamming_host(sc, algorithm, type, patterns, nullptr, 0, texts, min_score, n, out_score, out_sink, out_ok, n_threads);
}

NVB_API int nvbio_hip_hamming_score_qual_host(const nvbio_hip_gotoh_qual_scheme* scheme, int32_t algorithm, int32_t type,
                                              const nvbio_hip_string_set* patterns, const uint8_t* quals, uint64_t n_quals, const nvbio_hip_string_set* texts,
                                              const int32_t* min_score, uint32_t n, int32_t* out_score, uint32_t* out_sink, uint8_t* out_ok, int32_t n_threads)
{
    if (!scheme || (n != 0 && (!quals || n_quals == 0))) return hipErrorInvalidValue;
    const QualLutScheme sc = { scheme->match, scheme->mismatch };
    return hamming_host(sc, algorithm, type, patterns, quals, n_quals, texts, min_score, n, out_score, out_sink, out_ok, n_threads);
}

NVB_API int nvbio_hip_fm_rank_host(const nvbio_hip_fmindex* fmi, const uint32_t* k, const uint8_t* c, uint32_t n, uint32_t* out, int32_t n_threads)
{
    if (!fmi || !fmi->bwt_occ || (n && (!k || !c || !out))) return hipErrorInvalidValue;
    const fmi_t f = host_index(fmi);
#if defined(_OPENMP)
    const int threads = n_threads > 0 ? n_threads : omp_get_max_threads();
#endif
    #pragma omp parallel for schedule(static) num_threads(threads)
    for (int64 i = 0; i < int64(n); ++i) out[i] = rank(f, k[i], uint8(c[i] & 3u));
    return hipSuccess;
}

NVB_API int nvbio_hip_fm_match_host(const nvbio_hip_fmindex* fmi, const nvbio_hip_string_set* seeds, uint32_t n, uint32_t* out_range, int32_t n_threads)
{
    if (!fmi || !fmi->bwt_occ || !valid_set(seeds) || (n && !out_range)) return hipErrorInvalidValue;
    const fmi_t f = host_index(fmi);
#if defined(_OPENMP)
    const int threads = n_threads > 0 ? n_threads : omp_get_max_threads();
#endif
    #pragma omp parallel for schedule(dynamic, 1024) num_threads(threads)
    for (int64 i = 0; i < int64(n); ++i)
    {
        const RtString s = string_of(seeds, uint32(i));
        const uint2 r = match(f, s, s.len);
        out_range[2 * i] = r.x; out_range[2 * i + 1] = r.y;
    }
    return hipSuccess;
}

NVB_API int nvbio_hip_fm_locate_host(const nvbio_hip_fmindex* fmi, const uint32_t* sa_rows, uint32_t n, uint32_t* out_pos, int32_t n_threads)
{
    if (!fmi || !fmi->bwt_occ || !fmi->ssa || fmi->sa_int == 0 || (fmi->sa_int & (fmi->sa_int - 1)) != 0 || (n && (!sa_rows || !out_pos))) return hipErrorInvalidValue;
    const fmi_t f = host_index(fmi);
#if defined(_OPENMP)
    const int threads = n_threads > 0 ? n_threads : omp_get_max_threads();
#endif
    #pragma omp parallel for schedule(dynamic, 1024) num_threads(threads)
    for (int64 i = 0; i < int64(n); ++i) out_pos[i] = locate(f, sa_rows[i]);
    return hipSuccess;
}

// ---------------------------------------------------------------------------------------- bidirectional search, MEMs
NVB_API int nvbio_hip_fm_extend_host(int32_t direction, const nvbio_hip_fmindex* f_fmi, const nvbio_hip_fmindex* r_fmi,
                                     const uint32_t* f_ranges, const uint32_t* r_ranges, const uint8_t* c, uint32_t n,
                                     uint32_t* out_f_ranges, uint32_t* out_r_ranges, int32_t n_threads)
{
    if (!f_fmi || !r_fmi || !f_fmi->bwt_occ || !r_fmi->bwt_occ || f_fmi->length != r_fmi->length) return hipErrorInvalidValue;
    if (direction != NVBIO_HIP_EXTEND_FORWARD && direction != NVBIO_HIP_EXTEND_BACKWARDS) return hipErrorInvalidValue;
    if (n && (!f_ranges || !r_ranges || !c || !out_f_ranges || !out_r_ranges)) return hipErrorInvalidValue;
    const fmi_t f = host_index(f_fmi), r = host_index(r_fmi);
#if defined(_OPENMP)
    const int threads = n_threads > 0 ? n_threads : omp_get_max_threads();
#endif
    #pragma omp parallel for schedule(static) num_threads(threads)
    for (int64 i = 0; i < int64(n); ++i)
    {
        uint2 fr = make_uint2(f_ranges[2 * i], f_ranges[2 * i + 1]), rr = make_uint2(r_ranges[2 * i], r_ranges[2 * i + 1]);
        if (c[i] > 3u) { fr = make_uint2(1u, 0u); rr = fr; }
        else if (direction == NVBIO_HIP_EXTEND_FORWARD) extend_forward(f, r, fr, rr, c[i]);
        else                                            extend_backwards(f, r, fr, rr, c[i]);
        out_f_ranges[2 * i] = fr.x; out_f_ranges[2 * i + 1] = fr.y; out_r_ranges[2 * i] = rr.x; out_r_ranges[2 * i + 1] = rr.y;
    }
    return hipSuccess;
}

namespace {

// The body of both rank twins.  walk(string, length, id, f, r, out, store, store2, &records) appends a string's records to `out` and
// returns how many spans it found.  What happens when `capacity` is too small follows the device entries: the plain one stores the
// first `capacity` records and reports the total; the re-seeding one (store_nothing) stages every span found, duplicates
// included, so past that many it stores nothing and reports that count.
template <typename Walk>
int mem_rank_twin(const nvbio_hip_fmindex* f_fmi, const nvbio_hip_fmindex* r_fmi, const nvbio_hip_string_set* strings,
                  const uint32 n, const uint32 max_pattern_len, const uint32 min_intv,
                  uint32* out_ranges, const uint64 capacity, uint64* out_index, uint64* out_slots, uint64* out_n_ranges,
                  uint64* out_records, const int32 n_threads, const bool store_nothing, const Walk walk)
{
    const int admitted = nvb::mem_rank_admission(f_fmi, r_fmi, strings, n, max_pattern_len, min_intv, out_ranges, capacity, out_index, out_slots, out_n_ranges,
                                                 [=]() { if (out_records) *out_records = 0; out_index[0] = 0; });
    if (admitted != nvb::MEM_ARGS_GO && admitted != nvb::MEM_ARGS_EMPTY) return admitted;
    if (admitted == nvb::MEM_ARGS_EMPTY) { for (uint32 i = 0; i < n; ++i) out_index[i + 1u] = 0; return hipSuccess; }
    if (strings->length) for (uint32 i = 0; i < n; ++i) if (strings->length[i] > max_pattern_len) return hipErrorInvalidValue;
    const fmi_t f = host_index(f_fmi), r = host_index(r_fmi);
#if defined(_OPENMP)
    const int threads = n_threads > 0 ? n_threads : omp_get_max_threads();
#endif
    std::vector< std::vector< MEMRange<uint32> > > found(n);
    uint64 records = 0, raw = 0;
    #pragma omp parallel num_threads(threads) reduction(+ : records, raw)
    {
        std::vector<uint4> store, store2;
        #pragma omp for schedule(dynamic, 256)
        for (int64 i = 0; i < int64(n); ++i)
        {
            const RtString s = string_of(strings, uint32(i));
            const uint32 len = s.len < max_pattern_len ? s.len : max_pattern_len;
            raw += walk(s, len, uint32(i), f, r, found[i], store, store2, &records);
        }
    }
    if (out_records) *out_records = records;
    if (store_nothing && raw > capacity) { *out_n_ranges = raw; return NVBIO_HIP_ERROR_CAPACITY; }
    fmindex::flatten_mems(found, capacity, out_index, [out_ranges](const uint64 at, const MEMRange<uint32>& m)
                          { uint32* o = out_ranges + 4 * at; o[0] = m.coords.x; o[1] = m.coords.y; o[2] = m.coords.z; o[3] = m.coords.w; }, out_slots);
    *out_n_ranges = out_index[n];
    return out_index[n] > capacity ? NVBIO_HIP_ERROR_CAPACITY : int(hipSuccess);
}

} // namespace

NVB_API int nvbio_hip_fm_mem_rank_host(const nvbio_hip_fmindex* f_fmi, const nvbio_hip_fmindex* r_fmi, const nvbio_hip_string_set* strings,
                                       uint32_t n, uint32_t max_pattern_len, uint32_t min_intv, uint32_t max_intv, uint32_t min_span,
                                       uint32_t* out_ranges, uint64_t capacity, uint64_t* out_index, uint64_t* out_slots, uint64_t* out_n_ranges,
                                       uint64_t* out_records, int32_t n_threads)
{
    return mem_rank_twin(f_fmi, r_fmi, strings, n, max_pattern_len, min_intv, out_ranges, capacity, out_index, out_slots, out_n_ranges, out_records, n_threads,
                         false, [=](const RtString& s, const uint32 len, const uint32 id, const fmi_t& f, const fmi_t& r, std::vector< MEMRange<uint32> >& out,
                                    std::vector<uint4>& store, std::vector<uint4>&, uint64* records)
                         { fmindex::string_mems(s, len, id, f, r, min_intv, max_intv, min_span, out, store, records); return uint64(out.size()); });
}

NVB_API int nvbio_hip_fm_mem_rank_split_host(const nvbio_hip_fmindex* f_fmi, const nvbio_hip_fmindex* r_fmi, const nvbio_hip_string_set* strings,
                                             uint32_t n, uint32_t max_pattern_len, uint32_t min_intv, uint32_t max_intv, uint32_t min_span,
                                             uint32_t split_len, uint32_t split_width,
                                             uint32_t* out_ranges, uint64_t capacity, uint64_t* out_index, uint64_t* out_slots, uint64_t* out_n_ranges,
                                             uint64_t* out_records, int32_t n_threads)
{
    if (split_len == 0xFFFFFFFFu)                      // no re-seeding: the plain twin, word for word
        return nvbio_hip_fm_mem_rank_host(f_fmi, r_fmi, strings, n, max_pattern_len, min_intv, max_intv, min_span, out_ranges, capacity, out_index, out_slots,
                                          out_n_ranges, out_records, n_threads);
    return mem_rank_twin(f_fmi, r_fmi, strings, n, max_pattern_len, min_intv, out_ranges, capacity, out_index, out_slots, out_n_ranges, out_records, n_threads,
                         true, [=](const RtString& s, const uint32 len, const uint32 id, const fmi_t& f, const fmi_t& r, std::vector< MEMRange<uint32> >& out,
                                   std::vector<uint4>& store, std::vector<uint4>& store2, uint64* records)
                         { return fmindex::string_mems_split(s, len, id, f, r, min_intv, max_intv, min_span, split_len, split_width, out, store, store2, records); });
}

NVB_API int nvbio_hip_fm_mem_locate_host(const nvbio_hip_fmindex* f_fmi, const uint32_t* ranges, const uint64_t* slots, uint64_t n_ranges,
                                         uint64_t begin, uint64_t end, uint32_t* out_hits, int32_t n_threads)
{
    if (!f_fmi || !f_fmi->bwt_occ || !f_fmi->ssa || f_fmi->sa_int == 0 || (f_fmi->sa_int & (f_fmi->sa_int - 1)) != 0) return hipErrorInvalidValue;
    if (end < begin) return hipErrorInvalidValue;
    if (end == begin) return hipSuccess;
    if (!ranges || !slots || !out_hits || n_ranges == 0) return hipErrorInvalidValue;
    const fmi_t f = host_index(f_fmi);
#if defined(_OPENMP)
    const int threads = n_threads > 0 ? n_threads : omp_get_max_threads();
#endif
    #pragma omp parallel for schedule(dynamic, 1024) num_threads(threads)
    for (int64 h = 0; h < int64(end - begin); ++h)
    {
        const uint64 g = begin + uint64(h);
        const uint64 lo = nvbio::upper_bound_index(g, slots, n_ranges);
        uint32* o = out_hits + 4 * h;
        if (lo >= n_ranges) { o[0] = o[1] = 0xFFFFFFFFu; o[2] = o[3] = 0u; continue; }
        const uint32* rg = ranges + 4 * lo;
        o[0] = locate(f, uint32(rg[0] + uint32(g - (lo ? slots[lo - 1u] : 0u))));
        o[1] = rg[2] & 0x7FFFFFFFu; o[2] = rg[3] & 0xFFFFu; o[3] = rg[3] >> 16;
    }
    return hipSuccess;
}

// ---- suffix sorting and BWT of one 2-bit text (sufsort.hip): prefix doubling with std::sort, the same convention, the same bytes ----
namespace {

inline uint32 text_symbol(const uint32* words, const uint32 be, const uint64 i)
{
    const uint32 k = uint32(i & 15u);
    return (words[i >> 4] >> (be ? 30u - 2u * k : 2u * k)) & 3u;
}

/// sym(i): symbol i of the text
template <typename Sym>
int suffix_sort_host_of(const Sym sym, const uint64 n, uint32* sa, const int threads)
{
    // rank 0 = past the end, so a suffix that is a prefix of another sorts first; symbols are 1.. in the first round
    std::vector<uint32> rank(n), next(n);
    std::vector<uint64> key(n);
    uint32* rows = sa + 1;
    sa[0] = uint32(n);
    #pragma omp parallel for schedule(static) num_threads(threads)
    for (int64 i = 0; i < int64(n); ++i) { rows[i] = uint32(i); rank[i] = uint32(sym(uint64(i))) + 1u; }
    for (uint64 h = 1;; h *= 2u)
    {
        #pragma omp parallel for schedule(static) num_threads(threads)
        for (int64 i = 0; i < int64(n); ++i)
            key[i] = (uint64(rank[i]) << 32) | (uint64(i) + h < n ? rank[uint64(i) + h] : 0u);
        std::sort(rows, rows + n, [&](const uint32 a, const uint32 b) { return key[a] < key[b]; });
        uint32 groups = 0;
        for (uint64 k = 0; k < n; ++k)
        {
            if (k == 0 || key[rows[k]] != key[rows[k - 1u]]) ++groups;
            next[rows[k]] = groups;
        }
        rank.swap(next);
        if (groups == n) return hipSuccess;
    }
}

int suffix_sort_host(const uint32* words, const uint32 be, const uint64 n, uint32* sa, const int threads)
{
    return suffix_sort_host_of([=](const uint64 i) { return text_symbol(words, be, i); }, n, sa, threads);
}

inline int sufsort_args(const uint32* words, const uint32 bits, const uint64 n)
{
    return (!words || bits != 2u || n == 0u || n > 0xFFFFFFFEull) ? int(hipErrorInvalidValue) : int(hipSuccess);
}

} // anonymous namespace

NVB_API int nvbio_hip_suffix_sort_host(const uint32_t* words, uint32_t bits, uint32_t big_endian, uint64_t n, uint32_t* sa_out, int32_t n_threads)
{
    if (int e = sufsort_args(words, bits, n)) return e;
    if (!sa_out) return hipErrorInvalidValue;
#if defined(_OPENMP)
    const int threads = n_threads > 0 ? n_threads : omp_get_max_threads();
#else
    const int threads = 1;
#endif
    return suffix_sort_host(words, big_endian ? 1u : 0u, n, sa_out, threads);
}

NVB_API int nvbio_hip_bwt_host(const uint32_t* words, uint32_t bits, uint32_t big_endian, uint64_t n, uint32_t sa_int, uint32_t* bwt_words_out,
                               uint32_t* primary_out, uint32_t* ssa_out, uint32_t* sa_out, int32_t n_threads)
{
    if (int e = sufsort_args(words, bits, n)) return e;
    if (!bwt_words_out || !primary_out || (ssa_out && sa_int == 0u)) return hipErrorInvalidValue;
#if defined(_OPENMP)
    const int threads = n_threads > 0 ? n_threads : omp_get_max_threads();
#else
    const int threads = 1;
#endif
    std::vector<uint32> own;
    if (!sa_out) { own.resize(n + 1u); sa_out = own.data(); }
    const uint32 be = big_endian ? 1u : 0u;
    if (int e = suffix_sort_host(words, be, n, sa_out, threads)) return e;
    uint64 primary = 0;
    for (uint64 r = 0; r <= n; ++r) if (sa_out[r] == 0u) { primary = r; break; }
    *primary_out = uint32(primary);
    const uint64 n_words = 4u * ((n + 63u) / 64u);
    #pragma omp parallel for schedule(static) num_threads(threads)
    for (int64 w = 0; w < int64(n_words); ++w)
    {
        uint32 out = 0u;
        for (uint32 q = 0; q < 16u; ++q)
        {
            const uint64 j = uint64(w) * 16u + q;
            if (j < n) out |= text_symbol(words, be, uint64(sa_out[j + (j >= primary ? 1u : 0u)]) - 1u) << (30u - 2u * q);
        }
        bwt_words_out[w] = out;
    }
    if (ssa_out)
    {
        const uint64 n_ssa = (n + sa_int) / sa_int;
        for (uint64 k = 0; k < n_ssa; ++k) ssa_out[k] = k ? sa_out[k * sa_int] : 0xFFFFFFFFu;
    }
    return hipSuccess;
}

// ---- suffix sorting and BWT of a set of 2-bit strings (sufsort.hip, the set entries): prefix doubling with std::sort over the slots, each
// string's empty suffix a terminator of its own that sorts by string id below every symbol -- the definition, and so the same bytes ----
namespace {

struct SetSlots
{
    std::vector<uint64> cum;         // inclusive sums of length + 1
    std::vector<uint32> sid;         // the string of every slot
};

inline uint32 set_length(const nvbio_hip_string_set* set, const uint32 s) { return set->length ? set->length[s] : set->fixed_length; }

inline int set_sufsort_args(const nvbio_hip_string_set* set, const uint32 n_strings, const uint64 n)
{
    if (!set || !set->words || !set->begin || set->bits != 2u) return hipErrorInvalidValue;
    if (n_strings == 0u || n_strings > n || n > 0xFFFFFFFEull) return hipErrorInvalidValue;
    if (n_strings > 0xFFFFFFFBu) return hipErrorInvalidValue;          // the first ranks, up to n_strings + 4, are 32-bit words
    return hipSuccess;
}

/// rows[row] = the global index of the slot on that row; hipErrorInvalidValue when the lengths do not add up to n
int set_suffix_sort_host(const nvbio_hip_string_set* set, const uint32 N, const uint64 n, SetSlots& slots, uint32* rows, const int threads)
{
    slots.cum.resize(N);
    uint64 total = 0;
    for (uint32 s = 0; s < N; ++s) { total += uint64(set_length(set, s)) + 1u; slots.cum[s] = total; }
    if (total != n) return hipErrorInvalidValue;
    slots.sid.resize(n);
    std::vector<uint32> rank(n), next(n), term(n);       // term: the slot of the string's empty suffix
    std::vector<uint64> key(n);
    const uint32 be = set->big_endian ? 1u : 0u;
    #pragma omp parallel for schedule(dynamic, 256) num_threads(threads)
    for (int64 s = 0; s < int64(N); ++s)
    {
        const uint64 first = s ? slots.cum[s - 1] : 0u, last = slots.cum[s] - 1u;
        for (uint64 g = first; g <= last; ++g)
        {
            slots.sid[g] = uint32(s);
            term[g] = uint32(last);
            rows[g] = uint32(g);
            rank[g] = g == last ? uint32(s) + 1u : N + 1u + text_symbol(set->words, be, set->begin[s] + (g - first));
        }
    }
    // the first key holds an initial rank, which may need all 32 bits beside the next slot's; later ranks are group numbers <= n
    for (uint64 h = 1;; h *= 2u)
    {
        #pragma omp parallel for schedule(static) num_threads(threads)
        for (int64 g = 0; g < int64(n); ++g)
            key[g] = (uint64(rank[g]) << 32) | (uint64(g) + h <= term[g] ? rank[uint64(g) + h] : 0u);
        std::sort(rows, rows + n, [&](const uint32 a, const uint32 b) { return key[a] < key[b]; });
        uint32 groups = 0;
        for (uint64 k = 0; k < n; ++k)
        {
            if (k == 0 || key[rows[k]] != key[rows[k - 1u]]) ++groups;
            next[rows[k]] = groups;
        }
        rank.swap(next);
        if (groups == n) return hipSuccess;
    }
}

} // anonymous namespace

NVB_API int nvbio_hip_set_suffix_sort_host(const nvbio_hip_string_set* set, uint32_t n_strings, uint64_t n_suffixes, uint32_t* suffixes_out,
                                           uint32_t* string_ids_out, uint32_t* cum_lengths_out, int32_t n_threads)
{
    if (int e = set_sufsort_args(set, n_strings, n_suffixes)) return e;
    if (!suffixes_out) return hipErrorInvalidValue;
#if defined(_OPENMP)
    const int threads = n_threads > 0 ? n_threads : omp_get_max_threads();
#else
    const int threads = 1;
#endif
    SetSlots slots;
    std::vector<uint32> rows(n_suffixes);                // the outputs stay untouched when the lengths do not add up
    if (int e = set_suffix_sort_host(set, n_strings, n_suffixes, slots, rows.data(), threads)) return e;
    std::copy(rows.begin(), rows.end(), suffixes_out);
    if (string_ids_out) std::copy(slots.sid.begin(), slots.sid.end(), string_ids_out);
    if (cum_lengths_out) for (uint32 s = 0; s < n_strings; ++s) cum_lengths_out[s] = uint32(slots.cum[s]);
    return hipSuccess;
}

NVB_API int nvbio_hip_set_bwt_host(const nvbio_hip_string_set* set, uint32_t n_strings, uint64_t n_suffixes, uint8_t* bwt_out,
                                   uint32_t* dollar_rows_out, uint32_t* dollar_ids_out, uint32_t* suffixes_out, int32_t n_threads)
{
    if (int e = set_sufsort_args(set, n_strings, n_suffixes)) return e;
    if (!bwt_out || !dollar_rows_out || !dollar_ids_out) return hipErrorInvalidValue;
#if defined(_OPENMP)
    const int threads = n_threads > 0 ? n_threads : omp_get_max_threads();
#else
    const int threads = 1;
#endif
    SetSlots slots;
    std::vector<uint32> rows(n_suffixes);
    if (int e = set_suffix_sort_host(set, n_strings, n_suffixes, slots, rows.data(), threads)) return e;
    const uint32 be = set->big_endian ? 1u : 0u;
    uint64 n_dollars = 0;
    for (uint64 row = 0; row < n_suffixes; ++row)
    {
        const uint32 g = rows[row], s = slots.sid[g];
        const uint64 p = g - (s ? slots.cum[s - 1] : 0u);
        bwt_out[row] = p ? uint8(text_symbol(set->words, be, set->begin[s] + p - 1u)) : uint8(255u);
        if (p == 0u) { dollar_rows_out[n_dollars] = uint32(row); dollar_ids_out[n_dollars] = s; ++n_dollars; }
        if (suffixes_out) { suffixes_out[2u * row] = uint32(p); suffixes_out[2u * row + 1u] = s; }
    }
    return hipSuccess;
}

// ---- q-gram indices and the q-gram filter (qgram.hip): the definitions of include/nvbio_hip.h symbol by symbol, std::stable_sort for
// the build and std::sort for merge -- all orders are total, so the same bytes ----
namespace {

inline bool qgram_params_ok(const uint32 bits, const uint32 q, const uint32 ql) { return bits == 2u && q >= 1u && q <= 32u && ql <= (q < 16u ? q : 16u); }
inline bool qgram_set_ok(const nvbio_hip_string_set* set, const uint32 n_strings)
{
    return set && set->words && set->n_words && (set->begin || n_strings == 0u) && set->bits == 2u;
}
inline int qgram_threads(const int32 n_threads)
{
#if defined(_OPENMP)
    return n_threads > 0 ? n_threads : omp_get_max_threads();
#else
    return 1;
#endif
}

/// the q-gram at position pos of the string [begin, begin + len): only symbols of the string are read
inline uint64 qgram_at(const uint32* words, const uint32 be, const uint64 begin, const uint64 len, const uint64 pos, const uint32 q)
{
    uint64 g = 0;
    for (uint32 j = 0; j < q && pos + j < len; ++j)
        g |= uint64(text_symbol(words, be, begin + pos + j)) << (2u * j);
    return g;
}

inline uint64 qgram_seed_count(const uint32 len, const uint32 q, const uint32 interval) { return len >= q ? uint64(len - q) / interval + 1u : 0u; }

/// keys / coords in enumeration order -> the index arrays
template <typename V>
void qgram_build_host(const std::vector<uint64>& keys, const V* coords, const uint32 q, const uint32 ql, uint64* qgrams_out, uint32* slots_out,
                      V* index_out, uint32* lut_out, uint32* n_unique_out)
{
    const uint64 n = keys.size();
    std::vector<uint32> order(n);
    for (uint64 i = 0; i < n; ++i) order[i] = uint32(i);
    std::stable_sort(order.begin(), order.end(), [&](const uint32 a, const uint32 b) { return keys[a] < keys[b]; });
    uint32 n_unique = 0;
    for (uint64 k = 0; k < n; ++k)
    {
        if (k == 0 || keys[order[k]] != keys[order[k - 1u]]) { qgrams_out[n_unique] = keys[order[k]]; slots_out[n_unique] = uint32(k); ++n_unique; }
        index_out[k] = coords[order[k]];
    }
    slots_out[n_unique] = uint32(n);
    if (ql)
    {
        const uint64 n_keys = 1ull << (2u * ql);
        for (uint64 k = 0; k < n_keys; ++k)
            lut_out[k] = uint32(std::lower_bound(qgrams_out, qgrams_out + n_unique, k << (2u * (q - ql))) - qgrams_out);
        lut_out[n_keys] = n_unique;
    }
    *n_unique_out = n_unique;
}

inline bool qgram_index_ok(const nvbio_hip_qgram_index* ix)
{
    if (!ix || !ix->slots || !qgram_params_ok(2u, ix->q, ix->ql) || ix->n_unique > ix->n_qgrams) return false;
    if (ix->n_unique && !ix->qgrams) return false;
    if (ix->ql && !ix->lut) return false;
    return true;
}

inline void qgram_range_of(const nvbio_hip_qgram_index* ix, const uint64 g, uint32* out)
{
    out[0] = out[1] = 0u;
    if (ix->q < 32u && (g >> (2u * ix->q))) return;
    uint32 lo = 0u, hi = ix->n_unique;
    if (ix->ql) { const uint64 k = g >> (2u * (ix->q - ix->ql)); lo = ix->lut[k]; hi = ix->lut[k + 1u]; }
    const uint32 i = uint32(std::lower_bound(ix->qgrams + lo, ix->qgrams + hi, g) - ix->qgrams);
    if (i >= ix->n_unique || ix->qgrams[i] != g) return;
    out[0] = ix->slots[i]; out[1] = ix->slots[i + 1u];
}

template <bool SET>
int qgram_locate_host(const nvbio_hip_qgram_index* ix, const uint32 n_queries, const uint32* ranges, const uint64* slots, const uint32* indices,
                      const uint64 begin, const uint64 end, uint32* hits, const int32 n_threads)
{
    if (!qgram_index_ok(ix) || begin > end) return hipErrorInvalidValue;
    if (begin == end) return hipSuccess;
    if (n_queries == 0u || !ranges || !slots || !indices || !hits || !ix->index) return hipErrorInvalidValue;
    const int threads = qgram_threads(n_threads);
    #pragma omp parallel for schedule(static) num_threads(threads)
    for (int64 k = 0; k < int64(end - begin); ++k)
    {
        const uint64 o = begin + uint64(k);
        const uint32 slot = uint32(std::upper_bound(slots, slots + n_queries, o) - slots);
        uint32 h0 = 0u, h1 = 0u, h2 = 0u;
        if (slot < n_queries)
        {
            const uint64 at = uint64(ranges[2u * slot]) + (o - (slot ? slots[slot - 1u] : 0ull));
            if (at < ix->n_qgrams)
            {
                if (SET) { h0 = ix->index[2u * at]; h1 = ix->index[2u * at + 1u]; h2 = indices[slot]; }
                else     { h0 = ix->index[at]; h1 = indices[slot]; }
            }
        }
        if (SET) { hits[4 * k] = h0; hits[4 * k + 1] = h1; hits[4 * k + 2] = h2; hits[4 * k + 3] = 0u; }
        else     { hits[2 * k] = h0; hits[2 * k + 1] = h1; }
    }
    return hipSuccess;
}

inline uint32 qgram_snap(const uint32 diag, const uint32 interval)
{
    const uint32 r = (diag / interval) * interval;
    return uint32((diag - r) * 2u) > interval ? r + 1u : r;
}

template <typename K>
void qgram_merge_keys(std::vector<K>& keys, K* merged_out, uint32* counts_out, uint32* n_merged_out)
{
    std::sort(keys.begin(), keys.end());
    uint32 m = 0;
    for (size_t k = 0; k < keys.size(); ++k)
    {
        if (k == 0 || keys[k] != keys[k - 1u]) { merged_out[m] = keys[k]; counts_out[m] = 0u; ++m; }
        ++counts_out[m - 1u];
    }
    *n_merged_out = m;
}

} // anonymous namespace

NVB_API int nvbio_hip_qgram_generate_host(const uint32_t* words, uint64_t n_words, uint32_t bits, uint32_t big_endian, uint64_t len, uint32_t q,
                                          const uint32_t* positions, uint64_t n, uint64_t* qgrams_out, int32_t n_threads)
{
    if (!words || !n_words || !qgram_params_ok(bits, q, 0u) || len > 0xFFFFFFFFull || n > 0xFFFFFFFFull) return hipErrorInvalidValue;
    if (n == 0u) return hipSuccess;
    if (!qgrams_out) return hipErrorInvalidValue;
    const int threads = qgram_threads(n_threads);
    const uint32 be = big_endian ? 1u : 0u;
    #pragma omp parallel for schedule(static) num_threads(threads)
    for (int64 i = 0; i < int64(n); ++i)
        qgrams_out[i] = qgram_at(words, be, 0u, len, positions ? positions[i] : uint64(i), q);
    return hipSuccess;
}

NVB_API int nvbio_hip_qgram_set_generate_host(const nvbio_hip_string_set* set, uint32_t n_strings, uint32_t q, const uint32_t* coords, uint64_t n,
                                              uint64_t* qgrams_out, int32_t n_threads)
{
    if (!qgram_set_ok(set, n_strings) || !qgram_params_ok(2u, q, 0u) || n > 0xFFFFFFFFull) return hipErrorInvalidValue;
    if (n == 0u) return hipSuccess;
    if (!coords || !qgrams_out) return hipErrorInvalidValue;
    const int threads = qgram_threads(n_threads);
    const uint32 be = set->big_endian ? 1u : 0u;
    #pragma omp parallel for schedule(static) num_threads(threads)
    for (int64 i = 0; i < int64(n); ++i)
    {
        const uint32 id = coords[2 * i], pos = coords[2 * i + 1];
        qgrams_out[i] = id < n_strings ? qgram_at(set->words, be, set->begin[id], set_length(set, id), pos, q) : 0ull;
    }
    return hipSuccess;
}

NVB_API int nvbio_hip_qgram_index_build_host(const uint32_t* words, uint64_t n_words, uint32_t bits, uint32_t big_endian, uint64_t len, uint32_t q, uint32_t ql,
                                             uint64_t* qgrams_out, uint32_t* slots_out, uint32_t* index_out, uint32_t* lut_out, uint32_t* n_unique_out,
                                             int32_t n_threads)
{
    if (!words || !n_words || !qgram_params_ok(bits, q, ql) || len > 0xFFFFFFFFull) return hipErrorInvalidValue;
    if (!slots_out || !n_unique_out || (len && (!qgrams_out || !index_out)) || (ql && !lut_out)) return hipErrorInvalidValue;
    const int threads = qgram_threads(n_threads);
    const uint32 be = big_endian ? 1u : 0u;
    std::vector<uint64> keys(len);
    std::vector<uint32> coords(len);
    #pragma omp parallel for schedule(static) num_threads(threads)
    for (int64 i = 0; i < int64(len); ++i) { keys[i] = qgram_at(words, be, 0u, len, uint64(i), q); coords[i] = uint32(i); }
    qgram_build_host<uint32>(keys, coords.data(), q, ql, qgrams_out, slots_out, index_out, lut_out, n_unique_out);
    return hipSuccess;
}

NVB_API int nvbio_hip_qgram_set_count_seeds_host(const nvbio_hip_string_set* set, uint32_t n_strings, uint32_t q, uint32_t interval, uint64_t* n_qgrams_out,
                                                 int32_t n_threads)
{
    (void)n_threads;
    if (!qgram_set_ok(set, n_strings) || !qgram_params_ok(2u, q, 0u) || interval == 0u || !n_qgrams_out) return hipErrorInvalidValue;
    uint64 total = 0;
    for (uint32 s = 0; s < n_strings; ++s) total += qgram_seed_count(set_length(set, s), q, interval);
    *n_qgrams_out = total;
    return hipSuccess;
}

NVB_API int nvbio_hip_qgram_set_index_build_host(const nvbio_hip_string_set* set, uint32_t n_strings, uint32_t q, uint32_t interval, uint32_t ql,
                                                 uint64_t n_qgrams, uint64_t* qgrams_out, uint32_t* slots_out, uint32_t* index_out, uint32_t* lut_out,
                                                 uint32_t* n_unique_out, int32_t n_threads)
{
    (void)n_threads;
    if (!qgram_set_ok(set, n_strings) || !qgram_params_ok(2u, q, ql) || interval == 0u || n_qgrams > 0xFFFFFFFFull) return hipErrorInvalidValue;
    if (!slots_out || !n_unique_out || (n_qgrams && (!qgrams_out || !index_out)) || (ql && !lut_out)) return hipErrorInvalidValue;
    uint64 total = 0;
    for (uint32 s = 0; s < n_strings; ++s) total += qgram_seed_count(set_length(set, s), q, interval);
    if (total != n_qgrams) return hipErrorInvalidValue;
    const uint32 be = set->big_endian ? 1u : 0u;
    std::vector<uint64> keys, coords;
    keys.reserve(n_qgrams); coords.reserve(n_qgrams);
    for (uint32 s = 0; s < n_strings; ++s)
    {
        const uint32 len = set_length(set, s);
        for (uint64 pos = 0; pos + q <= len; pos += interval)
        {
            keys.push_back(qgram_at(set->words, be, set->begin[s], len, pos, q));
            coords.push_back((pos << 32) | s);
        }
    }
    qgram_build_host<uint64>(keys, coords.data(), q, ql, qgrams_out, slots_out, reinterpret_cast<uint64*>(index_out), lut_out, n_unique_out);
    return hipSuccess;
}

NVB_API int nvbio_hip_qgram_range_host(const nvbio_hip_qgram_index* index, const uint64_t* queries, uint64_t n_queries, uint32_t* ranges_out, int32_t n_threads)
{
    if (!qgram_index_ok(index) || n_queries > 0xFFFFFFFFull) return hipErrorInvalidValue;
    if (n_queries == 0u) return hipSuccess;
    if (!queries || !ranges_out) return hipErrorInvalidValue;
    const int threads = qgram_threads(n_threads);
    #pragma omp parallel for schedule(static) num_threads(threads)
    for (int64 i = 0; i < int64(n_queries); ++i) qgram_range_of(index, queries[i], ranges_out + 2 * i);
    return hipSuccess;
}

NVB_API int nvbio_hip_qgram_rank_host(const nvbio_hip_qgram_index* index, const uint64_t* queries, uint64_t n_queries, uint32_t* ranges_out,
                                      uint64_t* slots_out, uint64_t* total_out, int32_t n_threads)
{
    if (!qgram_index_ok(index) || n_queries > 0xFFFFFFFFull || !total_out) return hipErrorInvalidValue;
    if (n_queries == 0u) { *total_out = 0u; return hipSuccess; }
    if (!queries || !ranges_out || !slots_out) return hipErrorInvalidValue;
    if (int e = nvbio_hip_qgram_range_host(index, queries, n_queries, ranges_out, n_threads)) return e;
    uint64 sum = 0;
    for (uint64 i = 0; i < n_queries; ++i) { sum += uint64(ranges_out[2 * i + 1] - ranges_out[2 * i]); slots_out[i] = sum; }
    *total_out = sum;
    return hipSuccess;
}

NVB_API int nvbio_hip_qgram_locate_host(const nvbio_hip_qgram_index* index, uint32_t n_queries, const uint32_t* ranges, const uint64_t* slots,
                                        const uint32_t* indices, uint64_t begin, uint64_t end, uint32_t* hits_out, int32_t n_threads)
{
    return qgram_locate_host<false>(index, n_queries, ranges, slots, indices, begin, end, hits_out, n_threads);
}

NVB_API int nvbio_hip_qgram_set_locate_host(const nvbio_hip_qgram_index* index, uint32_t n_queries, const uint32_t* ranges, const uint64_t* slots,
                                            const uint32_t* indices, uint64_t begin, uint64_t end, uint32_t* hits_out, int32_t n_threads)
{
    return qgram_locate_host<true>(index, n_queries, ranges, slots, indices, begin, end, hits_out, n_threads);
}

NVB_API int nvbio_hip_qgram_merge_host(const uint32_t* hits, uint32_t n_hits, uint32_t interval, uint32_t* merged_out, uint32_t* counts_out,
                                       uint32_t* n_merged_out, int32_t n_threads)
{
    (void)n_threads;
    if (interval == 0u || !n_merged_out) return hipErrorInvalidValue;
    if (n_hits == 0u) { *n_merged_out = 0u; return hipSuccess; }
    if (!hits || !merged_out || !counts_out) return hipErrorInvalidValue;
    std::vector<uint32> keys(n_hits);
    for (uint32 i = 0; i < n_hits; ++i) keys[i] = qgram_snap(hits[2u * uint64(i) + 1u] - hits[2u * uint64(i)], interval);
    qgram_merge_keys<uint32>(keys, merged_out, counts_out, n_merged_out);
    return hipSuccess;
}

NVB_API int nvbio_hip_qgram_set_merge_host(const uint32_t* hits, uint32_t n_hits, uint32_t interval, uint32_t* merged_out, uint32_t* counts_out,
                                           uint32_t* n_merged_out, int32_t n_threads)
{
    (void)n_threads;
    if (interval == 0u || !n_merged_out) return hipErrorInvalidValue;
    if (n_hits == 0u) { *n_merged_out = 0u; return hipSuccess; }
    if (!hits || !merged_out || !counts_out) return hipErrorInvalidValue;
    std::vector<uint64> keys(n_hits);
    for (uint32 i = 0; i < n_hits; ++i)
    {
        const uint32* h = hits + 4u * uint64(i);
        keys[i] = (uint64(h[0]) << 32) | qgram_snap(h[2] - h[1], interval);
    }
    qgram_merge_keys<uint64>(keys, reinterpret_cast<uint64*>(merged_out), counts_out, n_merged_out);
    return hipSuccess;
}

// ---- byte alphabets (sufsort.hip's `_bytes` entries, wavelet.hip): the suffix sort above over masked bytes, the tree by its definition
// (a stable sort by the top l bits for every level, the node table by counting bits of the finished stream), and the walks in the
// reference's terms (wavelet_tree_inl.h:339-497: inclusive positions, the clamp to the level's end, 0 at an empty node) ----
namespace {

inline int host_threads(const int32 n_threads)
{
#if defined(_OPENMP)
    return n_threads > 0 ? n_threads : omp_get_max_threads();
#else
    (void)n_threads;
    return 1;
#endif
}

inline bool bytes_args_ok(const uint8* symbols, const uint32 S, const uint64 n) { return symbols && S >= 1u && S <= 8u && n >= 1u && n <= 0xFFFFFFFEull; }
inline bool wavelet_size_ok(const uint64 n, const uint32 S) { return S >= 1u && S <= 8u && n >= 1u && n * S <= 0xFFFFFFFFull; }
inline bool wavelet_ok(const nvbio_hip_wavelet_tree* t) { return t && t->bits && t->splits && t->occ && wavelet_size_ok(t->size, t->symbol_size); }
inline bool wavelet_fm_ok(const nvbio_hip_wavelet_fmindex* f)
{
    return f && f->L2 && wavelet_ok(&f->bwt) && f->length == f->bwt.size && f->primary >= 1u && f->primary <= f->length;
}

inline uint32 wt_bit(const uint32* bits, const uint64 g) { return (bits[g >> 5] >> (31u - uint32(g & 31u))) & 1u; }

/// bits equal to b among the first `count` (>= 1) bits of a node of level l that starts `begin` bits into its level; `before` = occ[node].
/// The last bit looked at is clamped to the level's end, as the reference's node rank does.
inline uint32 wt_count_in_node(const nvbio_hip_wavelet_tree& t, const uint32 l, const uint32 before, const uint32 begin, const uint32 count, const uint32 b)
{
    const uint32 K = 1u << t.symbol_size;
    const uint32 first = l * t.size + begin;                                    // the node's first bit in the stream
    const uint32 last = std::min(first + count - 1u, (l + 1u) * t.size - 1u);   // inclusive
    const uint32 w = last >> 5, keep = (last & 31u) + 1u;                       // `keep` leading bits of word w belong to the prefix
    const uint32 ones_to_last = t.occ[K + w] + uint32(__builtin_popcount(t.bits[w] >> (32u - keep)));
    const uint32 ones = ones_to_last - before;
    return b ? ones : (last + 1u - first) - ones;
}

/// occurrences of symbol c in [0, i]; i = 0xFFFFFFFF gives 0, i >= size counts the whole text
inline uint32 wt_rank_host(const nvbio_hip_wavelet_tree& t, const uint32 i, const uint32 c)
{
    const uint32 S = t.symbol_size;
    uint32 node = 0u, begin = 0u, end = t.size, count = i + 1u;                 // the node's symbols are [begin, end) of the sorted text
    for (uint32 l = 0; l < S; ++l)
    {
        if (begin == end) return 0u;                                            // an empty node
        const uint32 b = (c >> (S - 1u - l)) & 1u;
        if (count) count = wt_count_in_node(t, l, t.occ[node], begin, count, b);
        const uint32 middle = t.splits[node];
        if (b) begin = middle; else end = middle;
        node = 2u * node + 1u + b;
    }
    return count;
}

/// the symbol at i < size; r_out = its occurrences before i
inline uint32 wt_text_host(const nvbio_hip_wavelet_tree& t, const uint32 i, uint32* r_out = nullptr)
{
    const uint32 S = t.symbol_size;
    uint32 node = 0u, begin = 0u, at = i, c = 0u;                               // `at`: the symbol's place inside its node
    for (uint32 l = 0; l < S; ++l)
    {
        const uint32 b = wt_bit(t.bits, uint64(l) * t.size + begin + at);
        c = (c << 1) | b;
        if (at) at = wt_count_in_node(t, l, t.occ[node], begin, at, b);         // the equal bits before it
        if (b) begin = t.splits[node];
        node = 2u * node + 1u + b;
    }
    if (r_out) *r_out = at;
    return c;
}

/// rank(fmi, k, c) of fmindex_inl.h:36-57 over the tree
inline uint32 wt_fm_rank_host(const nvbio_hip_wavelet_fmindex& f, uint32 k, const uint32 c)
{
    if (k == 0xFFFFFFFFu) return 0u;
    if (k == f.length) return f.L2[c + 1u] - f.L2[c];
    if (k >= f.primary) --k;
    return wt_rank_host(f.bwt, k, c);
}

} // anonymous namespace

NVB_API int nvbio_hip_suffix_sort_bytes_host(const uint8_t* symbols, uint32_t symbol_size, uint64_t n, uint32_t* sa_out, int32_t n_threads)
{
    if (!bytes_args_ok(symbols, symbol_size, n) || !sa_out) return hipErrorInvalidValue;
    const uint32 mask = (1u << symbol_size) - 1u;
    return suffix_sort_host_of([=](const uint64 i) { return uint32(symbols[i]) & mask; }, n, sa_out, host_threads(n_threads));
}

NVB_API int nvbio_hip_bwt_bytes_host(const uint8_t* symbols, uint32_t symbol_size, uint64_t n, uint32_t sa_int, uint8_t* bwt_out, uint32_t* primary_out,
                                     uint32_t* ssa_out, uint32_t* sa_out, int32_t n_threads)
{
    if (!bytes_args_ok(symbols, symbol_size, n)) return hipErrorInvalidValue;
    if (!bwt_out || !primary_out || (ssa_out && sa_int == 0u)) return hipErrorInvalidValue;
    std::vector<uint32> own;
    if (!sa_out) { own.resize(n + 1u); sa_out = own.data(); }
    const uint32 mask = (1u << symbol_size) - 1u;
    if (int e = suffix_sort_host_of([=](const uint64 i) { return uint32(symbols[i]) & mask; }, n, sa_out, host_threads(n_threads))) return e;
    uint64 primary = 0;
    for (uint64 r = 0; r <= n; ++r) if (sa_out[r] == 0u) { primary = r; break; }
    *primary_out = uint32(primary);
    for (uint64 j = 0; j < n; ++j) bwt_out[j] = uint8(symbols[sa_out[j + (j >= primary ? 1u : 0u)] - 1u] & mask);
    if (ssa_out)
    {
        const uint64 n_ssa = (n + sa_int) / sa_int;
        for (uint64 k = 0; k < n_ssa; ++k) ssa_out[k] = k ? sa_out[k * sa_int] : 0xFFFFFFFFu;
    }
    return hipSuccess;
}

NVB_API int nvbio_hip_wavelet_setup_host(const uint8_t* symbols, uint32_t symbol_size, uint64_t n, uint32_t* bits_out, uint32_t* splits_out, uint32_t* occ_out,
                                         int32_t n_threads)
{
    (void)n_threads;
    if (!symbols || !bits_out || !splits_out || !occ_out || !wavelet_size_ok(n, symbol_size)) return hipErrorInvalidValue;
    const uint32 S = symbol_size, K = 1u << S;
    const uint64 W = (n * S + 31u) / 32u;
    std::vector<uint8> cur(n);
    for (uint64 i = 0; i < n; ++i) cur[i] = uint8(symbols[i] & (K - 1u));
    std::fill(bits_out, bits_out + W, 0u);
    for (uint32 l = 0; l < S; ++l)
    {
        for (uint64 i = 0; i < n; ++i)
            if ((cur[i] >> (S - 1u - l)) & 1u) { const uint64 g = uint64(l) * n + i; bits_out[g >> 5] |= 1u << (31u - uint32(g & 31u)); }
        const uint32 sh = S - 1u - l;                                   // the next level's order: by the top l + 1 bits
        std::stable_sort(cur.begin(), cur.end(), [sh](const uint8 a, const uint8 b) { return (a >> sh) < (b >> sh); });
    }
    uint32 sum = 0u;
    for (uint64 w = 0; w < W; ++w) { occ_out[K + w] = sum; sum += uint32(__builtin_popcount(bits_out[w])); }
    // cur is the sorted text by now: C(s) = the symbols smaller than s
    const auto C = [&](const uint32 s) { return uint32(std::lower_bound(cur.begin(), cur.end(), s, [](const uint8 a, const uint32 v) { return uint32(a) < v; }) - cur.begin()); };
    const auto ones_before = [&](const uint64 g) { uint32 c = (g >> 5) < W ? occ_out[K + (g >> 5)] : sum; for (uint64 k = g & ~31ull; k < g; ++k) c += wt_bit(bits_out, k); return c; };
    for (uint32 l = 0; l < S; ++l)
        for (uint32 j = 0; j < (1u << l); ++j)
        {
            const uint32 node = (1u << l) - 1u + j, first = j * (K >> l), mid = first + (K >> (l + 1u));
            splits_out[node] = C(mid);
            occ_out[node] = ones_before(uint64(l) * n + C(first));
        }
    splits_out[K - 1u] = 0u;
    occ_out[K - 1u] = 0u;
    return hipSuccess;
}

NVB_API int nvbio_hip_wavelet_text_host(const nvbio_hip_wavelet_tree* tree, const uint32_t* positions, uint64_t n_queries, uint8_t* out, int32_t n_threads)
{
    if (!wavelet_ok(tree) || n_queries > 0xFFFFFFFFull || (n_queries && !out)) return hipErrorInvalidValue;
    const int threads = host_threads(n_threads);
    #pragma omp parallel for schedule(static) num_threads(threads)
    for (int64 k = 0; k < int64(n_queries); ++k)
    {
        const uint64 p = positions ? uint64(positions[k]) : uint64(k);
        out[k] = p < tree->size ? uint8(wt_text_host(*tree, uint32(p))) : uint8(0);
    }
    return hipSuccess;
}

NVB_API int nvbio_hip_wavelet_rank_host(const nvbio_hip_wavelet_tree* tree, const uint32_t* positions, const uint8_t* symbols, uint64_t n_queries, uint32_t* out,
                                        int32_t n_threads)
{
    if (!wavelet_ok(tree) || n_queries > 0xFFFFFFFFull || (n_queries && (!positions || !symbols || !out))) return hipErrorInvalidValue;
    const int threads = host_threads(n_threads);
    #pragma omp parallel for schedule(static) num_threads(threads)
    for (int64 k = 0; k < int64(n_queries); ++k) out[k] = wt_rank_host(*tree, positions[k], symbols[k]);
    return hipSuccess;
}

NVB_API int nvbio_hip_wavelet_rank_range_host(const nvbio_hip_wavelet_tree* tree, const uint32_t* ranges, const uint8_t* symbols, uint64_t n_queries, uint32_t* out,
                                              int32_t n_threads)
{
    if (!wavelet_ok(tree) || n_queries > 0xFFFFFFFFull || (n_queries && (!ranges || !symbols || !out))) return hipErrorInvalidValue;
    const int threads = host_threads(n_threads);
    #pragma omp parallel for schedule(static) num_threads(threads)
    for (int64 k = 0; k < int64(n_queries); ++k)
    {
        out[2 * k]     = wt_rank_host(*tree, ranges[2 * k], symbols[k]);
        out[2 * k + 1] = wt_rank_host(*tree, ranges[2 * k + 1], symbols[k]);
    }
    return hipSuccess;
}

NVB_API int nvbio_hip_wavelet_fm_L2_host(const nvbio_hip_wavelet_tree* tree, uint32_t* L2_out, int32_t n_threads)
{
    (void)n_threads;
    if (!wavelet_ok(tree) || !L2_out) return hipErrorInvalidValue;
    const uint32 K = 1u << tree->symbol_size;
    L2_out[0] = 0u;
    for (uint32 c = 0; c < K; ++c) L2_out[c + 1u] = L2_out[c] + wt_rank_host(*tree, tree->size - 1u, c);
    return hipSuccess;
}

NVB_API int nvbio_hip_wavelet_fm_match_host(const nvbio_hip_wavelet_fmindex* fmi, const nvbio_hip_byte_string_set* patterns, uint64_t n, uint32_t* ranges_out,
                                            int32_t n_threads)
{
    if (!wavelet_fm_ok(fmi) || !patterns || n > 0xFFFFFFFFull || (n && (!patterns->begin || !ranges_out))) return hipErrorInvalidValue;
    if (n && !patterns->symbols && patterns->n_symbols) return hipErrorInvalidValue;
    const int threads = host_threads(n_threads);
    const uint32 K = 1u << fmi->bwt.symbol_size;
    const uint64 n_symbols = patterns->symbols ? patterns->n_symbols : 0u;
    #pragma omp parallel for schedule(dynamic, 256) num_threads(threads)
    for (int64 id = 0; id < int64(n); ++id)
    {
        const uint64 beg = patterns->begin[id];
        uint64 len = patterns->length ? patterns->length[id] : patterns->fixed_length;
        if (beg >= n_symbols) len = 0u; else if (len > n_symbols - beg) len = n_symbols - beg;
        uint32 x = 0u, y = fmi->length;
        for (uint64 i = len; i-- > 0u && x <= y;)
        {
            const uint32 c = patterns->symbols[beg + i];
            if (c >= K) { x = 1u; y = 0u; break; }
            const uint32 rx = wt_fm_rank_host(*fmi, x - 1u, c), ry = wt_fm_rank_host(*fmi, y, c);
            x = fmi->L2[c] + rx + 1u;
            y = fmi->L2[c] + ry;
        }
        ranges_out[2 * id] = x; ranges_out[2 * id + 1] = y;
    }
    return hipSuccess;
}

NVB_API int nvbio_hip_wavelet_fm_locate_host(const nvbio_hip_wavelet_fmindex* fmi, const uint32_t* rows, uint64_t n_rows, uint32_t* positions_out, int32_t n_threads)
{
    if (!wavelet_fm_ok(fmi) || !fmi->ssa || fmi->sa_int == 0u) return hipErrorInvalidValue;
    if (n_rows > 0xFFFFFFFFull || (n_rows && (!rows || !positions_out))) return hipErrorInvalidValue;
    const int threads = host_threads(n_threads);
    #pragma omp parallel for schedule(dynamic, 256) num_threads(threads)
    for (int64 id = 0; id < int64(n_rows); ++id)
    {
        uint32 j = rows[id], t = 0u;
        while (j <= fmi->length && j % fmi->sa_int != 0u && t <= fmi->length)
        {
            if (j != fmi->primary)
            {
                const uint32 c = wt_text_host(fmi->bwt, j < fmi->primary ? j : j - 1u);
                j = fmi->L2[c] + wt_fm_rank_host(*fmi, j, c);                  // fmindex_inl.h:491-492
            }
            else j = 0u;
            ++t;
        }
        positions_out[id] = (j <= fmi->length && j % fmi->sa_int == 0u) ? fmi->ssa[j / fmi->sa_int] + t : 0xFFFFFFFFu;
    }
    return hipSuccess;
}
