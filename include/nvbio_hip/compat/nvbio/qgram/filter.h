// compat/nvbio/qgram/filter.h -- QGramFilter<system_tag, qgram_index_type, query_iterator, index_iterator> (nvbio/qgram/filter.h)
// behind the reference's own template: rank(index, n_queries, queries, indices) looks the query q-grams up and ranks their slot ranges
// (inclusive 64-bit scan of the sizes), locate(begin, end, hits) enumerates the hits [begin, end) -- uint2 (index position, query index)
// for a string index, uint4 (string id, position, query index, 0) for a set index --, merge(interval, n_hits, hits, merged, counts)
// counts the hits per snapped diagonal.  QGramFilterHost / QGramFilterDevice are the two names callers use.  Definitions and the two
// deliberate points (64-bit offsets for set hits too; the reference's rounding of diagonals, r + 1) are in DESIGN.md 3.14.
//
// The device filter picks one of two executions per call, with identical results (last_path() says which):
//   * tuned   -- queries, query indices, hits and outputs are plain device memory (pointers, thrust::device_ptr, device_vector
//                iterators): the index view is described to the C-ABI and nvbio_hip_qgram_rank / _locate / _merge run;
//   * generic -- any other iterator (a transform_iterator of queries, say), or set_generic(true): thrust::transform with the index
//                view as the functor, a thrust scan, one upper bound per hit, a thrust sort and reduce_by_key.
// The host filter runs the same functors in loops.
#pragma once
#include "qgram.h"
#include <thrust/device_vector.h>
#include <thrust/execution_policy.h>
#include <algorithm>
#include <vector>

namespace nvbio {

namespace qgram {

/// the reference's util::round(diag, interval) as it is written: the multiple of interval at or below diag, plus ONE where the
/// remainder is more than half the interval
NVBIO_FORCEINLINE NVBIO_HOST_DEVICE uint32 snap_diagonal(const uint32 diag, const uint32 interval)
{
    const uint32 r = (diag / interval) * interval;
    return uint32((diag - r) * 2u) > interval ? r + 1u : r;
}

struct range_size
{
    typedef uint2  argument_type;
    typedef uint64 result_type;
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE uint64 operator()(const uint2 range) const { return uint64(range.y - range.x); }
};

template <typename hit_type> struct closest_diagonal {};
template <> struct closest_diagonal<uint2>
{
    typedef uint2  argument_type;
    typedef uint32 result_type;
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE closest_diagonal(const uint32 i) : interval(i) {}
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE uint32 operator()(const uint2 hit) const { return snap_diagonal(hit.y - hit.x, interval); }
    const uint32 interval;
};
/// a set hit gives the 64-bit sort word of the uint2 (diagonal, string id): the string id in the high half
template <> struct closest_diagonal<uint4>
{
    typedef uint4  argument_type;
    typedef uint64 result_type;
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE closest_diagonal(const uint32 i) : interval(i) {}
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE uint64 operator()(const uint4 hit) const { return (uint64(hit.x) << 32) | snap_diagonal(hit.z - hit.y, interval); }
    const uint32 interval;
};

template <typename hit_type, typename coord_type> struct make_hit {};
template <> struct make_hit<uint2, uint32> { NVBIO_FORCEINLINE NVBIO_HOST_DEVICE static uint2 make(const uint32 c, const uint32 q) { return make_uint2(c, q); } };
template <> struct make_hit<uint4, uint2>  { NVBIO_FORCEINLINE NVBIO_HOST_DEVICE static uint4 make(const uint2 c, const uint32 q)  { return make_uint4(c.x, c.y, q, 0u); } };

template <typename P> struct diagonal_of {};
template <> struct diagonal_of<uint32> { typedef uint32 type; NVBIO_FORCEINLINE NVBIO_HOST_DEVICE static uint32 make(const uint32 w) { return w; } };
template <> struct diagonal_of<uint64> { typedef uint2  type; NVBIO_FORCEINLINE NVBIO_HOST_DEVICE static uint2 make(const uint64 w) { return make_uint2(uint32(w), uint32(w >> 32)); } };

/// output index -> hit: the upper bound of the index in the ranked slots, the offset inside that query's range in 64 bits
template <typename index_view, typename index_iterator, typename hit_type>
struct filter_results
{
    typedef uint64   argument_type;
    typedef hit_type result_type;
    filter_results(const index_view v, const uint32 n, const uint64* s, const uint2* r, const index_iterator i) : view(v), n_queries(n), slots(s), ranges(r), indices(i) {}
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE hit_type operator()(const uint64 output_index) const
    {
        uint32 lo = 0u, hi = n_queries;
        while (lo < hi) { const uint32 mid = lo + (hi - lo) / 2u; if (slots[mid] <= output_index) lo = mid + 1u; else hi = mid; }
        const uint64 base = lo ? slots[lo - 1u] : 0u;
        return make_hit<hit_type, typename index_view::coord_type>::make(view.locate(uint32(uint64(ranges[lo].x) + (output_index - base))), uint32(indices[lo]));
    }
    const index_view view; const uint32 n_queries; const uint64* slots; const uint2* ranges; const index_iterator indices;
};

template <typename P> struct word_to_diagonal
{
    typedef P argument_type;
    typedef typename diagonal_of<P>::type result_type;
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE result_type operator()(const P w) const { return diagonal_of<P>::make(w); }
};

/// plain device memory holding values of `bytes` bytes
template <typename It, uint32 bytes, bool OK = nvbio::priv::plain_iterator<It>::ok> struct plain_memory { static const bool ok = false; static void* get(It) { return nullptr; } };
template <typename It, uint32 bytes> struct plain_memory<It, bytes, true>
{
    typedef nvbio::priv::plain_iterator<It> plain;
    static const bool ok = sizeof(typename plain::value_type) == bytes;
    static void* get(It it) { return (void*)plain::get(it); }
};

} // namespace qgram

template <typename system_tag, typename qgram_index_type, typename query_iterator, typename index_iterator> struct QGramFilter {};

// ---------------------------------------------------------------------------------------- host
template <typename qgram_index_type, typename query_iterator, typename index_iterator>
struct QGramFilter<host_tag, qgram_index_type, query_iterator, index_iterator>
{
    typedef host_tag                                                   system_tag;
    typedef typename plain_view_subtype<const qgram_index_type>::type  qgram_index_view;
    typedef typename qgram_index_type::coord_type                      coord_type;
    static const bool is_set = !same_type<coord_type, uint32>::pred;
    typedef typename std::conditional<is_set, uint4, uint2>::type      hit_type;
    typedef typename std::conditional<is_set, uint2, uint32>::type     diagonal_type;
    typedef typename std::conditional<is_set, uint64, uint32>::type    primitive_type;

    QGramFilter() : m_n_queries(0), m_n_occurrences(0) {}

    uint64 rank(const qgram_index_type& index, const uint32 n_queries, const query_iterator queries, const index_iterator indices)
    {
        m_n_queries = n_queries; m_queries = queries; m_indices = indices; m_qgram_index = plain_view(index);
        m_ranges.resize(n_queries); m_slots.resize(n_queries);
        uint64 sum = 0u;
        for (uint32 i = 0; i < n_queries; ++i)
        {
            m_ranges[i] = m_qgram_index(queries[i]);
            sum += qgram::range_size()(m_ranges[i]);
            m_slots[i] = sum;
        }
        m_n_occurrences = sum;                      // 0 for no queries
        return m_n_occurrences;
    }

    template <typename hits_iterator>
    void locate(const uint64 begin, const uint64 end, hits_iterator hits)
    {
        const qgram::filter_results<qgram_index_view, index_iterator, hit_type> f(m_qgram_index, m_n_queries, m_slots.data(), m_ranges.data(), m_indices);
        for (uint64 o = begin; o < end; ++o) hits[o - begin] = f(o);
    }

    template <typename hits_iterator, typename output_iterator>
    void diagonals(const uint32 n_hits, const hits_iterator hits, output_iterator diags, const uint32 interval)
    {
        const qgram::closest_diagonal<hit_type> f(interval);
        for (uint32 i = 0; i < n_hits; ++i) diags[i] = qgram::diagonal_of<primitive_type>::make(f(hits[i]));
    }

    template <typename hits_iterator, typename output_iterator, typename count_iterator>
    uint32 merge(const uint32 interval, const uint32 n_hits, const hits_iterator hits, output_iterator merged_hits, count_iterator merged_counts)
    {
        const qgram::closest_diagonal<hit_type> f(interval);
        m_diags.resize(n_hits);
        for (uint32 i = 0; i < n_hits; ++i) m_diags[i] = f(hits[i]);
        std::sort(m_diags.begin(), m_diags.end());
        uint32 n_merged = 0u;
        for (uint32 i = 0; i < n_hits; ++i)
        {
            if (i == 0u || m_diags[i] != m_diags[i - 1u]) { merged_hits[n_merged] = qgram::diagonal_of<primitive_type>::make(m_diags[i]); merged_counts[n_merged] = 0u; ++n_merged; }
            merged_counts[n_merged - 1u] = merged_counts[n_merged - 1u] + 1u;
        }
        return n_merged;
    }

    uint64        n_hits() const { return m_n_occurrences; }
    const uint64* ranks()  const { return m_slots.data(); }
    const uint2*  ranges() const { return m_ranges.data(); }
    const char*   last_path() const { return "host"; }

    uint32                      m_n_queries;
    query_iterator              m_queries;
    index_iterator              m_indices;
    qgram_index_view            m_qgram_index;
    uint64                      m_n_occurrences;
    std::vector<uint2>          m_ranges;
    std::vector<uint64>         m_slots;
    std::vector<primitive_type> m_diags;
};

// ---------------------------------------------------------------------------------------- device
template <typename qgram_index_type, typename query_iterator, typename index_iterator>
struct QGramFilter<device_tag, qgram_index_type, query_iterator, index_iterator>
{
    typedef device_tag                                                 system_tag;
    typedef typename plain_view_subtype<const qgram_index_type>::type  qgram_index_view;
    typedef typename qgram_index_type::coord_type                      coord_type;
    static const bool is_set = !same_type<coord_type, uint32>::pred;
    typedef typename std::conditional<is_set, uint4, uint2>::type      hit_type;
    typedef typename std::conditional<is_set, uint2, uint32>::type     diagonal_type;
    typedef typename std::conditional<is_set, uint64, uint32>::type    primitive_type;

    QGramFilter() : m_n_queries(0), m_n_occurrences(0), m_generic(false), m_path("none") {}

    /// true: never call the C-ABI, whatever the iterators are
    void set_generic(const bool on) { m_generic = on; }
    const char* last_path() const { return m_path; }

    uint64 rank(const qgram_index_type& index, const uint32 n_queries, const query_iterator queries, const index_iterator indices)
    {
        m_n_queries = n_queries; m_queries = queries; m_indices = indices; m_qgram_index = plain_view(index);
        m_n_occurrences = 0u;
        if (n_queries == 0u) return 0u;             // the reference reads slots[-1] here
        if (m_ranges.size() < n_queries) { m_ranges.clear(); m_ranges.resize(n_queries); }
        if (m_slots.size() < n_queries)  { m_slots.clear();  m_slots.resize(n_queries); }
        if (!rank_tuned(std::integral_constant<bool, qgram::plain_memory<query_iterator, 8u>::ok>()))
        {
            thrust::transform(thrust::device, queries, queries + n_queries, m_ranges.begin(), m_qgram_index);
            thrust::inclusive_scan(thrust::device, thrust::make_transform_iterator(m_ranges.begin(), qgram::range_size()),
                                   thrust::make_transform_iterator(m_ranges.begin(), qgram::range_size()) + n_queries, m_slots.begin());
            m_n_occurrences = m_slots[n_queries - 1u];
            m_path = "generic";
        }
        return m_n_occurrences;
    }

    template <typename hits_iterator>
    void locate(const uint64 begin, const uint64 end, hits_iterator hits)
    {
        if (end <= begin || m_n_queries == 0u) return;
        if (locate_tuned(begin, end, hits, std::integral_constant<bool, qgram::plain_memory<index_iterator, 4u>::ok && qgram::plain_memory<hits_iterator, sizeof(hit_type)>::ok>())) return;
        thrust::transform(thrust::device, thrust::make_counting_iterator<uint64>(begin), thrust::make_counting_iterator<uint64>(end), hits,
                          qgram::filter_results<qgram_index_view, index_iterator, hit_type>(m_qgram_index, m_n_queries, raw_pointer(m_slots), raw_pointer(m_ranges), m_indices));
        m_path = "generic";
    }

    template <typename hits_iterator, typename output_iterator>
    void diagonals(const uint32 n_hits, const hits_iterator hits, output_iterator diags, const uint32 interval)
    {
        thrust::transform(thrust::device, thrust::make_transform_iterator(hits, qgram::closest_diagonal<hit_type>(interval)),
                          thrust::make_transform_iterator(hits, qgram::closest_diagonal<hit_type>(interval)) + n_hits, diags, qgram::word_to_diagonal<primitive_type>());
    }

    template <typename hits_iterator, typename output_iterator, typename count_iterator>
    uint32 merge(const uint32 interval, const uint32 n_hits, const hits_iterator hits, output_iterator merged_hits, count_iterator merged_counts)
    {
        if (n_hits == 0u) return 0u;
        if (interval == 0u) throw std::runtime_error("nvbio qgram: the merging interval must be at least 1");
        uint32 n_merged = 0u;
        if (merge_tuned(interval, n_hits, hits, merged_hits, merged_counts, n_merged,
                        std::integral_constant<bool, qgram::plain_memory<hits_iterator, sizeof(hit_type)>::ok && qgram::plain_memory<output_iterator, sizeof(diagonal_type)>::ok &&
                                                     qgram::plain_memory<count_iterator, 4u>::ok>())) return n_merged;
        m_diags.resize(n_hits);
        thrust::transform(thrust::device, hits, hits + n_hits, m_diags.begin(), qgram::closest_diagonal<hit_type>(interval));
        thrust::sort(thrust::device, m_diags.begin(), m_diags.end());
        m_keys.resize(n_hits);
        n_merged = uint32(thrust::reduce_by_key(thrust::device, m_diags.begin(), m_diags.end(), thrust::make_constant_iterator<uint32>(1u),
                                                m_keys.begin(), merged_counts).first - m_keys.begin());
        thrust::transform(thrust::device, m_keys.begin(), m_keys.begin() + n_merged, merged_hits, qgram::word_to_diagonal<primitive_type>());
        m_path = "generic";
        return n_merged;
    }

    uint64        n_hits() const { return m_n_occurrences; }
    const uint64* ranks()  const { return raw_pointer(m_slots); }       ///< device memory
    const uint2*  ranges() const { return raw_pointer(m_ranges); }      ///< device memory

private:
    nvbio_hip_qgram_index abi() const
    {
        nvbio_hip_qgram_index ix;
        ix.qgrams = m_qgram_index.qgrams; ix.slots = m_qgram_index.slots; ix.index = reinterpret_cast<const uint32*>(m_qgram_index.index);
        ix.lut = m_qgram_index.QL ? m_qgram_index.lut : nullptr;
        ix.q = m_qgram_index.Q; ix.ql = m_qgram_index.QL; ix.n_unique = m_qgram_index.n_unique_qgrams; ix.n_qgrams = m_qgram_index.n_qgrams;
        return ix;
    }
    /// the C-ABI serves 2-bit symbols, uint64 q-grams and a LUT of at most 16 symbols
    bool abi_index() const { return !m_generic && m_qgram_index.symbol_size == 2u && m_qgram_index.QL <= 16u && sizeof(typename qgram_index_view::qgram_type) == 8u; }

    bool rank_tuned(std::false_type) { return false; }
    bool rank_tuned(std::true_type)
    {
        if (!abi_index()) return false;
        const nvbio_hip_qgram_index ix = abi();
        const uint64 tb = nvbio_hip_qgram_rank_temp_bytes(m_n_queries);
        if (m_temp.size() < tb) m_temp.resize(tb);
        qgram::check(nvbio_hip_qgram_rank(&ix, reinterpret_cast<const uint64*>(qgram::plain_memory<query_iterator, 8u>::get(m_queries)), m_n_queries,
                                          reinterpret_cast<uint32*>(raw_pointer(m_ranges)), raw_pointer(m_slots), &m_n_occurrences, raw_pointer(m_temp), tb, nullptr),
                     "nvbio_hip_qgram_rank");
        m_path = "tuned";
        return true;
    }
    template <typename hits_iterator> bool locate_tuned(const uint64, const uint64, hits_iterator, std::false_type) { return false; }
    template <typename hits_iterator> bool locate_tuned(const uint64 begin, const uint64 end, hits_iterator hits, std::true_type)
    {
        if (!abi_index()) return false;
        const nvbio_hip_qgram_index ix = abi();
        const uint32* indices = reinterpret_cast<const uint32*>(qgram::plain_memory<index_iterator, 4u>::get(m_indices));
        uint32* out = reinterpret_cast<uint32*>(qgram::plain_memory<hits_iterator, sizeof(hit_type)>::get(hits));
        const uint32* ranges = reinterpret_cast<const uint32*>(raw_pointer(m_ranges));
        if (is_set) qgram::check(nvbio_hip_qgram_set_locate(&ix, m_n_queries, ranges, raw_pointer(m_slots), indices, begin, end, out, nullptr), "nvbio_hip_qgram_set_locate");
        else        qgram::check(nvbio_hip_qgram_locate(&ix, m_n_queries, ranges, raw_pointer(m_slots), indices, begin, end, out, nullptr), "nvbio_hip_qgram_locate");
        m_path = "tuned";
        return true;
    }
    template <typename H, typename O, typename C> bool merge_tuned(const uint32, const uint32, H, O, C, uint32&, std::false_type) { return false; }
    template <typename H, typename O, typename C> bool merge_tuned(const uint32 interval, const uint32 n_hits, H hits, O merged, C counts, uint32& n_merged, std::true_type)
    {
        if (m_generic) return false;
        const uint64 tb = is_set ? nvbio_hip_qgram_set_merge_temp_bytes(n_hits) : nvbio_hip_qgram_merge_temp_bytes(n_hits);
        if (m_temp.size() < tb) m_temp.resize(tb);
        const uint32* h = reinterpret_cast<const uint32*>(qgram::plain_memory<H, sizeof(hit_type)>::get(hits));
        uint32* m = reinterpret_cast<uint32*>(qgram::plain_memory<O, sizeof(diagonal_type)>::get(merged));
        uint32* c = reinterpret_cast<uint32*>(qgram::plain_memory<C, 4u>::get(counts));
        if (is_set) qgram::check(nvbio_hip_qgram_set_merge(h, n_hits, interval, m, c, &n_merged, raw_pointer(m_temp), tb, nullptr), "nvbio_hip_qgram_set_merge");
        else        qgram::check(nvbio_hip_qgram_merge(h, n_hits, interval, m, c, &n_merged, raw_pointer(m_temp), tb, nullptr), "nvbio_hip_qgram_merge");
        m_path = "tuned";
        return true;
    }

public:
    uint32                                m_n_queries;
    query_iterator                        m_queries;
    index_iterator                        m_indices;
    qgram_index_view                      m_qgram_index;
    uint64                                m_n_occurrences;
private:
    thrust::device_vector<uint2>          m_ranges;
    thrust::device_vector<uint64>         m_slots;
    thrust::device_vector<primitive_type> m_diags, m_keys;
    thrust::device_vector<uint8>          m_temp;
    bool                                  m_generic;
    const char*                           m_path;
};

template <typename qgram_index_type, typename query_iterator, typename index_iterator>
struct QGramFilterHost : public QGramFilter<host_tag, qgram_index_type, query_iterator, index_iterator> {};

template <typename qgram_index_type, typename query_iterator, typename index_iterator>
struct QGramFilterDevice : public QGramFilter<device_tag, qgram_index_type, query_iterator, index_iterator> {};

} // namespace nvbio
