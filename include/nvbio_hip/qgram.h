// include/nvbio_hip/qgram.h -- the C++ host layer of the q-gram module (nvbio/qgram/qgram.h, filter.h): thin callers of the
// nvbio_hip_qgram_* entries (include/nvbio_hip.h) over the project's device vectors.  No HIP headers are needed to
// include it.
//
//   generate_qgrams(text, q, positions, n, out)      the q-grams of a packed text at n positions (positions == nullptr: 0 .. n - 1)
//   generate_qgrams(set, q, coords, n, out)          the q-grams of a string set at n (string id, position) pairs
//   QGramIndexDevice::build(q, text, qlut)           qgrams / slots / index / lut of one text, every position indexed
//   QGramSetIndexDevice::build(q, set, interval, qlut)   the same over the seeds 0, interval, .. of every string; index holds uint2
//   index.range(queries, n, ranges)                  the slots of n query q-grams, (0, 0) where absent
//   QGramFilterDevice                                rank(index, n, queries, indices) -> hits; locate(begin, end, hits);
//                                                    merge(interval, n_hits, hits, merged, counts) -> n_merged
#pragma once
#include "types.h"
#include "strings.h"
#include "sufsort.h"
#include <type_traits>

namespace nvbio {
namespace hip {

template <bool BE>
inline void generate_qgrams(const PackedTextView<BE>& text, const uint32 q, const uint32* positions, const uint64 n, device_vector<uint64>& out, void* stream = nullptr)
{
    out.resize(n);
    const uint64 n_words = text.length ? (text.length + 15u) / 16u : 1u;
    hip_check(nvbio_hip_qgram_generate(text.words, n_words, 2u, BE ? 1u : 0u, text.length, q, positions, n, out.data(), stream), "nvbio_hip_qgram_generate");
}

template <bool BE>
inline void generate_qgrams(const PackedStringSetView<2, BE>& set, const uint32 q, const uint2* coords, const uint64 n, device_vector<uint64>& out, void* stream = nullptr)
{
    out.resize(n);
    const nvbio_hip_string_set s = set.abi();
    hip_check(nvbio_hip_qgram_set_generate(&s, set.size(), q, reinterpret_cast<const uint32*>(coords), n, out.data(), stream), "nvbio_hip_qgram_set_generate");
}

/// the arrays of an index and the calls both kinds share; COORD is uint32 (a text position) or uint2 (string id, position)
template <typename COORD>
struct QGramIndexDeviceCore
{
    typedef COORD coord_type;
    QGramIndexDeviceCore() : Q(0), QL(0), n_qgrams(0), n_unique_qgrams(0) {}

    uint32 Q, QL;
    uint32 n_qgrams, n_unique_qgrams;
    device_vector<uint64> qgrams;          ///< the distinct q-grams, ascending (sized for n_qgrams; the first n_unique_qgrams are set)
    device_vector<uint32> slots;           ///< n_unique_qgrams + 1 exclusive sums of their counts
    device_vector<COORD>  index;           ///< the coordinates grouped by q-gram, in enumeration order inside one
    device_vector<uint32> lut;             ///< 4^QL + 1 words, empty when QL == 0

    nvbio_hip_qgram_index abi() const
    {
        nvbio_hip_qgram_index ix;
        ix.qgrams = qgrams.data(); ix.slots = slots.data(); ix.index = reinterpret_cast<const uint32*>(index.data()); ix.lut = QL ? lut.data() : nullptr;
        ix.q = Q; ix.ql = QL; ix.n_unique = n_unique_qgrams; ix.n_qgrams = n_qgrams;
        return ix;
    }

    /// ranges[i] = the slots (begin, end) of queries[i] in `index`, (0, 0) where the q-gram is not indexed
    void range(const uint64* queries, const uint64 n, device_vector<uint2>& ranges, void* stream = nullptr) const
    {
        ranges.resize(n);
        const nvbio_hip_qgram_index ix = abi();
        hip_check(nvbio_hip_qgram_range(&ix, queries, n, reinterpret_cast<uint32*>(ranges.data()), stream), "nvbio_hip_qgram_range");
    }

protected:
    void size_for(const uint32 q, const uint32 qlut, const uint64 n)
    {
        if (n > 0xFFFFFFFFull) throw hip_error("the q-gram index build (more than 2^32 - 1 q-grams)", 1);      // before anything is allocated
        Q = q; QL = qlut; n_qgrams = uint32(n);
        qgrams.resize(n); slots.resize(n + 1u); index.resize(n);
        if (qlut && qlut <= 16u) lut.resize((size_t(1) << (2u * qlut)) + 1u);
    }
};

struct QGramIndexDevice : public QGramIndexDeviceCore<uint32>
{
    /// index every position of `text`; `temp` is the call's scratch, kept by the caller between calls
    template <bool BE>
    void build(const uint32 q, const PackedTextView<BE>& text, const uint32 qlut, device_vector<uint8>& temp, void* stream = nullptr)
    {
        const uint64 tb = nvbio_hip_qgram_index_build_temp_bytes(text.length);
        if (temp.size() < tb) temp.resize(tb);
        size_for(q, qlut, text.length);
        const uint64 n_words = text.length ? (text.length + 15u) / 16u : 1u;
        hip_check(nvbio_hip_qgram_index_build(text.words, n_words, 2u, BE ? 1u : 0u, text.length, q, qlut, qgrams.data(), slots.data(), index.data(),
                                              qlut ? lut.data() : nullptr, &n_unique_qgrams, temp.data(), temp.size(), stream), "nvbio_hip_qgram_index_build");
    }
    template <bool BE>
    void build(const uint32 q, const PackedTextView<BE>& text, const uint32 qlut = 0u, void* stream = nullptr)
    {
        device_vector<uint8> temp;
        build(q, text, qlut, temp, stream);
    }
};

struct QGramSetIndexDevice : public QGramIndexDeviceCore<uint2>
{
    /// index the seeds 0, interval, 2 interval, .. (while a whole q-gram fits) of every string of `set`
    template <bool BE>
    void build(const uint32 q, const PackedStringSetView<2, BE>& set, const uint32 interval, const uint32 qlut, device_vector<uint8>& temp, void* stream = nullptr)
    {
        const nvbio_hip_string_set s = set.abi();
        const uint64 cb = nvbio_hip_qgram_set_count_seeds_temp_bytes(set.size());
        if (temp.size() < cb) temp.resize(cb);
        uint64 n = 0;
        hip_check(nvbio_hip_qgram_set_count_seeds(&s, set.size(), q, interval, &n, temp.data(), temp.size(), stream), "nvbio_hip_qgram_set_count_seeds");
        const uint64 tb = nvbio_hip_qgram_set_index_build_temp_bytes(n, set.size());
        if (temp.size() < tb) temp.resize(tb);
        size_for(q, qlut, n);
        hip_check(nvbio_hip_qgram_set_index_build(&s, set.size(), q, interval, qlut, n, qgrams.data(), slots.data(), reinterpret_cast<uint32*>(index.data()),
                                                  qlut ? lut.data() : nullptr, &n_unique_qgrams, temp.data(), temp.size(), stream),
                  "nvbio_hip_qgram_set_index_build");
    }
    template <bool BE>
    void build(const uint32 q, const PackedStringSetView<2, BE>& set, const uint32 interval = 1u, const uint32 qlut = 0u, void* stream = nullptr)
    {
        device_vector<uint8> temp;
        build(q, set, interval, qlut, temp, stream);
    }
};

/// the q-gram filter over an index of either kind: hit_type is uint2 (index position, query index) for a QGramIndexDevice and
/// uint4 (string id, position, query index, 0) for a QGramSetIndexDevice; diagonal_type is uint32, or uint2 (diagonal, string id)
template <typename qgram_index_type>
struct QGramFilterDevice
{
    typedef typename qgram_index_type::coord_type coord_type;
    static const bool is_set = sizeof(coord_type) == 8u;
    struct string_types { typedef uint2 hit_type; typedef uint32 diagonal_type; };
    struct set_types    { typedef uint4 hit_type; typedef uint2  diagonal_type; };
    typedef typename std::conditional<is_set, set_types, string_types>::type types;
    typedef typename types::hit_type      hit_type;
    typedef typename types::diagonal_type diagonal_type;

    QGramFilterDevice() : m_index(nullptr), m_n_queries(0), m_indices(nullptr), m_n_occurrences(0) {}

    /// look the n query q-grams up; indices[i] is what query i is called in a hit.  -> the number of hits
    uint64 rank(const qgram_index_type& index, const uint32 n_queries, const uint64* queries, const uint32* indices, void* stream = nullptr)
    {
        m_index = &index; m_n_queries = n_queries; m_indices = indices;
        m_ranges.resize(n_queries); m_slots.resize(n_queries);
        const uint64 tb = nvbio_hip_qgram_rank_temp_bytes(n_queries);
        if (m_temp.size() < tb) m_temp.resize(tb);
        const nvbio_hip_qgram_index ix = index.abi();
        hip_check(nvbio_hip_qgram_rank(&ix, queries, n_queries, reinterpret_cast<uint32*>(m_ranges.data()), m_slots.data(), &m_n_occurrences, m_temp.data(),
                                       m_temp.size(), stream), "nvbio_hip_qgram_rank");
        return m_n_occurrences;
    }

    uint64 n_hits() const { return m_n_occurrences; }

    /// hits [begin, end) of the last rank() into `hits` (device memory for end - begin of them)
    void locate(const uint64 begin, const uint64 end, hit_type* hits, void* stream = nullptr) const
    {
        const nvbio_hip_qgram_index ix = m_index->abi();
        const uint32* ranges = reinterpret_cast<const uint32*>(m_ranges.data());
        if (is_set) hip_check(nvbio_hip_qgram_set_locate(&ix, m_n_queries, ranges, m_slots.data(), m_indices, begin, end, reinterpret_cast<uint32*>(hits), stream),
                              "nvbio_hip_qgram_set_locate");
        else        hip_check(nvbio_hip_qgram_locate(&ix, m_n_queries, ranges, m_slots.data(), m_indices, begin, end, reinterpret_cast<uint32*>(hits), stream),
                              "nvbio_hip_qgram_locate");
    }

    /// the distinct snapped diagonals of n_hits hits, ascending, and their counts (device memory for n_hits of each).  -> their number
    uint32 merge(const uint32 interval, const uint32 n_hits, const hit_type* hits, diagonal_type* merged_hits, uint32* merged_counts, void* stream = nullptr)
    {
        const uint64 tb = is_set ? nvbio_hip_qgram_set_merge_temp_bytes(n_hits) : nvbio_hip_qgram_merge_temp_bytes(n_hits);
        if (m_temp.size() < tb) m_temp.resize(tb);
        uint32 n_merged = 0;
        if (is_set) hip_check(nvbio_hip_qgram_set_merge(reinterpret_cast<const uint32*>(hits), n_hits, interval, reinterpret_cast<uint32*>(merged_hits), merged_counts,
                                                        &n_merged, m_temp.data(), m_temp.size(), stream), "nvbio_hip_qgram_set_merge");
        else        hip_check(nvbio_hip_qgram_merge(reinterpret_cast<const uint32*>(hits), n_hits, interval, reinterpret_cast<uint32*>(merged_hits), merged_counts,
                                                    &n_merged, m_temp.data(), m_temp.size(), stream), "nvbio_hip_qgram_merge");
        return n_merged;
    }

    const qgram_index_type* m_index;
    uint32                  m_n_queries;
    const uint32*           m_indices;
    uint64                  m_n_occurrences;
    device_vector<uint2>    m_ranges;
    device_vector<uint64>   m_slots;
    device_vector<uint8>    m_temp;
};

} // namespace hip
} // namespace nvbio
