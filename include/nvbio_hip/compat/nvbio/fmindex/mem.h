// compat/nvbio/fmindex/mem.h -- maximal exact matches on a bidirectional FM-index (nvbio/fmindex/mem.h, mem_inl.h): find_kmems,
// MEMRange / MEMHit and MEMFilter<host_tag | device_tag, fm_index> (MEMFilterHost / MEMFilterDevice): rank(f_index, r_index, string_set, min_intv, max_intv, min_span, split_len, split_width) finds the
// k-SMEMs of every string and ranks their SA ranges, locate(begin, end, mems) enumerates the global hits [begin, end) as
// (text position, string id, span begin, span end).
//
// What is computed is DEFINED, not copied from the reference's output, because the reference's ranges start one
// row low (bidir.h here) and its walk drops some matches:
//   symbols > 3 match nothing; ell_k(p) = the longest l such that P[p, p+l) holds no such symbol and occurs at least k = min_intv
//   times; the k-SMEMs are the spans [p, p + ell_k(p)), ell_k(p) >= 1, that end past the span of p - 1; one is REPORTED iff it is
//   at least min_span long and its SA range holds at most max_intv rows; a string's MEMs are ordered by begin.
// Deviations from the reference: the start row (above); a right extension whose range never changes size after its first symbol is
// reported (the reference pushes its last range only after an earlier one, mem_inl.h:92); spans keep 16 bits of `begin`
// (the reference's span() masks it to 8, mem.h:220) and nothing is dropped past 1 024 ranges (mem_inl.h:381-382).
// rank's split_len / split_width re-seed in BWA-MEM's sense, by definition as well: a reported MEM at least split_len long whose range
// holds occ <= split_width rows is kept, and the (occ + 1)-SMEMs covering its midpoint that pass min_span and max_intv are added, every
// span once, ordered by begin, then end (the reference replaces the MEM and takes the begins at another threshold than the ends, mem_inl.h:1364-1424).
// find_threshold_kmems is not provided.
// Every execution -- the host filter, the lanes of the generic device filter, the C-ABI's `_host` twins -- walks a string with
// fmindex::walk_kmems and reports through mem_reseed_handler (plain) or mem_split_handler (re-seeding) into a sink; the host ones
// build their rank table with fmindex::flatten_mems.
#pragma once
#include "bidir.h"
#include "filter.h"
#include "../basic/algorithms.h"
#include <algorithm>
#include <vector>

namespace nvbio {

/// (SA begin, SA end, string id, begin | end << 16)   (mem.h:166-223)
template <typename coord_type>
struct MEMRange
{
    typedef typename vector_type<coord_type, 4u>::type base_type;
    typedef typename vector_type<coord_type, 2u>::type range_type;
    static const uint32 GROUP_FLAG = 1u << 31;

    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE MEMRange() {}
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE MEMRange(const base_type vec) : coords(vec) {}
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE MEMRange(const range_type range, const uint32 string_id, const uint2 span, const bool flag = false)
    { coords.x = range.x; coords.y = range.y; coords.z = string_id; coords.w = span.x | (span.y << 16); if (flag) set_group_flag(); }
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE MEMRange(const range_type range, const uint32 string_id, const uint32 span_begin, const uint32 span_end, const bool flag = false)
    { coords.x = range.x; coords.y = range.y; coords.z = string_id; coords.w = span_begin | (span_end << 16); if (flag) set_group_flag(); }

    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE void       set_group_flag()   { coords.z |= GROUP_FLAG; }
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE bool       group_flag() const { return (coords.z & GROUP_FLAG) ? true : false; }
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE range_type range() const      { return make_vector(coord_type(coords.x), coord_type(coords.y)); }
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE coord_type range_size() const { return coord_type(1) + coords.y - coords.x; }
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE uint32     string_id() const  { return uint32(coords.z) & (~GROUP_FLAG); }
    /// all 16 bits of the begin (the reference keeps 8, mem.h:220)
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE uint2      span() const       { return make_uint2(uint32(coords.w) & 0xFFFFu, uint32(coords.w) >> 16u); }

    base_type coords;
};

/// (text position, string id, span begin, span end)   (mem.h:233-272)
template <typename coord_type>
struct MEMHit
{
    typedef typename vector_type<coord_type, 4u>::type base_type;

    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE MEMHit() {}
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE MEMHit(const base_type vec) : coords(vec) {}
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE MEMHit(const coord_type index_pos, const uint32 string_id, const uint2 span)
    { coords.x = index_pos; coords.y = string_id; coords.z = span.x; coords.w = span.y; }
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE MEMHit(const coord_type index_pos, const uint32 string_id, const uint32 span_begin, const uint32 span_end)
    { coords.x = index_pos; coords.y = string_id; coords.z = span_begin; coords.w = span_end; }

    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE coord_type index_pos() const { return coords.x; }
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE uint32     string_id() const { return uint32(coords.y); }
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE uint2      span() const      { return make_uint2(uint32(coords.z), uint32(coords.w)); }

    base_type coords;
};

/// The k-SMEMs that cover symbol x of the pattern, begin ascending, handed to handler.output(range, span) (the delegate of
/// mem.h:56-68); returns the right-most end of those matches, or x if nothing matches there.  A caller walks the pattern with
/// x = max(returned, x + 1).  `store` keeps (SA begin, SA end, end) of the right extensions whose range size differs from the
/// next one's: anything with operator[] over uint4-like elements and room for pattern_len - x of them.  The last argument, if
/// given, receives the number of index records the walk read (priv::range_records of every step).
///
/// Right extension on the reverse index, then for each kept range, shortest first, a backward search on the forward index:
/// the begins can only grow with the length, and a span is a k-SMEM exactly when it begins before the next longer one does.
template <typename pattern_type, typename fm_index_type, typename delegate_type, typename store_type>
NVBIO_FORCEINLINE NVBIO_HOST_DEVICE
uint32 find_kmems(const uint32 pattern_len, const pattern_type pattern, const uint32 x, const fm_index_type f_index, const fm_index_type r_index,
                  delegate_type& handler, const uint32 min_intv, const uint32 min_span, store_type& store, uint64* n_records = NULL)
{
    typedef typename fm_index_type::index_type coord_type;
    typedef typename fm_index_type::range_type range_type;

    uint32 m = 0, i;
    uint64 records = 0;
    {
        range_type f_range = make_vector(coord_type(0u), f_index.length());
        range_type r_range = make_vector(coord_type(0u), r_index.length());
        for (i = x; i < pattern_len; ++i)
        {
            const uint8 c = pattern[i];
            if (c > 3) break;
            range_type nf = f_range, nr = r_range;
            records += priv::range_records(r_index, r_range);
            extend_forward(f_index, r_index, nf, nr, c);
            const coord_type size = coord_type(1u) + nf.y - nf.x;
            if (size < min_intv) break;
            if (i > x && size != coord_type(coord_type(1u) + f_range.y - f_range.x))
            { store[m].x = f_range.x; store[m].y = f_range.y; store[m].z = i; ++m; }
            f_range = nf; r_range = nr;
        }
        if (i > x) { store[m].x = f_range.x; store[m].y = f_range.y; store[m].z = i; ++m; }
    }
    if (m == 0u) { if (n_records) *n_records += records; return x; }

    bool       held = false;
    range_type held_range = make_vector(coord_type(0u), coord_type(0u));
    uint32     held_begin = 0, held_end = 0;
    for (uint32 j = 0; j < m; ++j)
    {
        range_type range = make_vector(coord_type(store[j].x), coord_type(store[j].y));
        int32 l;
        for (l = int32(x) - 1; l >= 0; --l)
        {
            const uint8 c = pattern[l];
            if (c > 3) break;
            const range_type c_rank = rank(f_index, make_vector(coord_type(range.x - 1), range.y), c);
            records += priv::range_records(f_index, range);
            const range_type next = make_vector(coord_type(f_index.L2(c) + c_rank.x + 1), coord_type(f_index.L2(c) + c_rank.y));
            if (coord_type(coord_type(1u) + next.y - next.x) < min_intv) break;
            range = next;
        }
        const uint32 begin = uint32(l + 1);
        if (held && held_begin < begin && held_end - held_begin >= min_span) handler.output(held_range, make_uint2(held_begin, held_end));
        held = true; held_range = range; held_begin = begin; held_end = uint32(store[j].z);
    }
    if (held_end - held_begin >= min_span) handler.output(held_range, make_uint2(held_begin, held_end));
    if (n_records) *n_records += records;
    return i;
}

/// the reference's argument list (mem.h:81-91); host only, the kept ranges live in a vector
template <typename pattern_type, typename fm_index_type, typename delegate_type>
uint32 find_kmems(const uint32 pattern_len, const pattern_type pattern, const uint32 x, const fm_index_type f_index, const fm_index_type r_index,
                  delegate_type& handler, const uint32 min_intv = 1u, const uint32 min_span = 1u)
{
    std::vector<uint4> store(pattern_len - x + 1u);
    return find_kmems(pattern_len, pattern, x, f_index, r_index, handler, min_intv, min_span, store);
}

namespace fmindex {

/// the walk over one string, on the host and in a lane: find_kmems from symbol 0, each group starting where the last one's matches end
template <typename pattern_type, typename fm_index_type, typename delegate_type, typename store_type>
NVBIO_FORCEINLINE NVBIO_HOST_DEVICE
void walk_kmems(const uint32 len, const pattern_type& s, const fm_index_type& f_index, const fm_index_type& r_index,
                delegate_type& handler, const uint32 min_intv, const uint32 min_span, store_type& store, uint64* n_records = NULL)
{
    for (uint32 x = 0; x < len;)
    {
        const uint32 e = find_kmems(len, s, x, f_index, r_index, handler, min_intv, min_span, store, n_records);
        x = e > x + 1u ? e : x + 1u;
    }
}

// ---- re-seeding (split_len / split_width): a reported MEM [b, e) at least split_len long with occ <= split_width rows is a
// candidate; its re-seeds are the (occ + 1)-SMEMs covering (b + e) >> 1 -- one find_kmems at that symbol and threshold -- kept iff
// they pass min_span and max_intv.  The spans go to a `sink` (output(range, span)) that makes the union.

/// the delegate of a walk that does not re-seed, and of a re-seed: applies max_intv and hands the span to the sink
template <typename coord_type, typename sink_type>
struct mem_reseed_handler
{
    typedef typename vector_type<coord_type, 2u>::type range_type;
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE mem_reseed_handler(sink_type& s, const uint32 max_intv_) : sink(s), max_intv(max_intv_) {}
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE void output(const range_type range, const uint2 span)
    {
        if (uint64(coord_type(coord_type(1u) + range.y - range.x)) <= uint64(max_intv)) sink.output(range, span);
    }
    sink_type& sink; uint32 max_intv;
};

/// the delegate of the base walk: applies max_intv, hands the MEM to the sink and, if it is a candidate, re-seeds it at once.
/// `store2` keeps the re-seed's right ranges (the base group's are still being read): room for pattern_len of them.
template <typename pattern_type, typename fm_index_type, typename sink_type, typename store_type>
struct mem_split_handler
{
    typedef typename fm_index_type::index_type coord_type;
    typedef typename fm_index_type::range_type range_type;
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE
    mem_split_handler(const uint32 len_, const pattern_type& pattern_, const fm_index_type& f, const fm_index_type& r, sink_type& sink_, store_type& store2_,
                      const uint32 max_intv_, const uint32 min_span_, const uint32 split_len_, const uint32 split_width_, uint64* n_records_) :
        len(len_), pattern(pattern_), f_index(f), r_index(r), sink(sink_), store2(store2_),
        max_intv(max_intv_), min_span(min_span_), split_len(split_len_), split_width(split_width_), n_records(n_records_) {}

    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE void output(const range_type range, const uint2 span)
    {
        const coord_type occ = coord_type(coord_type(1u) + range.y - range.x);
        if (uint64(occ) > uint64(max_intv)) return;
        sink.output(range, span);
        if (span.y - span.x < split_len || uint64(occ) > uint64(split_width)) return;
        const uint32 k = uint64(occ) >= 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32(occ) + 1u;      // cannot wrap
        mem_reseed_handler<coord_type, sink_type> reseed(sink, max_intv);
        find_kmems(len, pattern, (span.x + span.y) >> 1, f_index, r_index, reseed, k, min_span, store2, n_records);
    }
    const uint32 len; const pattern_type& pattern; const fm_index_type& f_index; const fm_index_type& r_index; sink_type& sink; store_type& store2;
    const uint32 max_intv, min_span, split_len, split_width; uint64* n_records;
};

/// begin, then end, of a span as one ordered key
NVBIO_FORCEINLINE NVBIO_HOST_DEVICE uint32 span_key(const uint32 w) { return (w << 16) | (w >> 16); }

/// a host sink: every span as it comes
template <typename coord_type>
struct mem_vector_sink
{
    typedef typename vector_type<coord_type, 2u>::type range_type;
    mem_vector_sink(std::vector< MEMRange<coord_type> >& out, const uint32 id) : ranges(out), string_id(id) {}
    void output(const range_type range, const uint2 span) { ranges.push_back(MEMRange<coord_type>(range, string_id, span)); }
    std::vector< MEMRange<coord_type> >& ranges; uint32 string_id;
};
template <typename coord_type>
struct mem_span_less
{
    bool operator() (const MEMRange<coord_type>& a, const MEMRange<coord_type>& b) const { return span_key(uint32(a.coords.w)) < span_key(uint32(b.coords.w)); }
};

/// every reported MEM of a string appended to `out`, begin ascending
template <typename string_type, typename fm_index_type>
void string_mems(const string_type& s, const uint32 len, const uint32 string_id, const fm_index_type& f_index, const fm_index_type& r_index,
                 const uint32 min_intv, const uint32 max_intv, const uint32 min_span,
                 std::vector< MEMRange<typename fm_index_type::index_type> >& out, std::vector<uint4>& store, uint64* n_records = NULL)
{
    typedef typename fm_index_type::index_type coord_type;
    typedef mem_vector_sink<coord_type>        sink_type;
    sink_type sink(out, string_id);
    mem_reseed_handler<coord_type, sink_type> handler(sink, max_intv);
    if (store.size() < size_t(len) + 1u) store.resize(size_t(len) + 1u);
    walk_kmems(len, s, f_index, r_index, handler, min_intv, min_span, store, n_records);
}

/// every reported MEM of a string and the re-seeds of its candidates appended to `out`, each span once, ordered by begin, then
/// end; returns the number of spans found before the duplicates were removed
template <typename string_type, typename fm_index_type>
uint64 string_mems_split(const string_type& s, const uint32 len, const uint32 string_id, const fm_index_type& f_index, const fm_index_type& r_index,
                         const uint32 min_intv, const uint32 max_intv, const uint32 min_span, const uint32 split_len, const uint32 split_width,
                         std::vector< MEMRange<typename fm_index_type::index_type> >& out, std::vector<uint4>& store, std::vector<uint4>& store2, uint64* n_records = NULL)
{
    typedef typename fm_index_type::index_type coord_type;
    typedef mem_vector_sink<coord_type>        sink_type;
    const size_t first = out.size();
    sink_type sink(out, string_id);
    if (store.size()  < size_t(len) + 1u) store.resize(size_t(len) + 1u);
    if (store2.size() < size_t(len) + 1u) store2.resize(size_t(len) + 1u);
    mem_split_handler<string_type, fm_index_type, sink_type, std::vector<uint4> > handler(len, s, f_index, r_index, sink, store2, max_intv, min_span, split_len, split_width, n_records);
    walk_kmems(len, s, f_index, r_index, handler, min_intv, min_span, store, n_records);
    const uint64 found = out.size() - first;
    std::sort(out.begin() + first, out.end(), mem_span_less<coord_type>());
    size_t kept = first;
    for (size_t k = first; k < out.size(); ++k)
        if (k == first || out[k].coords.w != out[k - 1u].coords.w) out[kept++] = out[k];
    out.resize(kept);
    return found;
}

/// the rank table of a batch from the MEMs of each string: index[q] = the first record of string q (n + 1 entries), then record
/// `at` goes to put(at, record) and slots[at] = the rows of the records up to it, for the first `capacity` records; returns the rows
/// of the records stored
template <typename coord_type, typename put_type>
uint64 flatten_mems(const std::vector< std::vector< MEMRange<coord_type> > >& per_string, const uint64 capacity, uint64* index, put_type put, uint64* slots)
{
    index[0] = 0;
    for (size_t q = 0; q < per_string.size(); ++q) index[q + 1u] = index[q] + per_string[q].size();
    uint64 sum = 0;
    for (size_t q = 0; q < per_string.size(); ++q)
        for (size_t k = 0; k < per_string[q].size(); ++k)
        {
            const uint64 at = index[q] + k;
            if (at >= capacity) return sum;
            put(at, per_string[q][k]);
            sum += uint64(per_string[q][k].range_size()); slots[at] = sum;
        }
    return sum;
}

} // namespace fmindex

template <typename system_tag, typename fm_index_type> struct MEMFilter {};

// ---------------------------------------------------------------------------------------- host   (mem.h:290-360)
template <typename fm_index_type>
struct MEMFilter<host_tag, fm_index_type>
{
    typedef host_tag                        system_tag;
    typedef fm_index_type                   index_type;
    typedef typename index_type::index_type coord_type;
    static const uint32                     coord_dim = vector_traits<coord_type>::DIM;
    typedef MEMRange<coord_type>            rank_type;
    typedef MEMHit<coord_type>              mem_type;
    typedef mem_type                        hit_type;

    MEMFilter() : m_n_queries(0), m_n_occurrences(0) {}

    /// returns the total number of MEM occurrences
    template <typename string_set_type>
    uint64 rank(const fm_index_type& f_index, const fm_index_type& r_index, const string_set_type& string_set,
                const uint32 min_intv = 1u, const uint32 max_intv = uint32(-1), const uint32 min_span = 1u,
                const uint32 split_len = uint32(-1), const uint32 split_width = uint32(-1))
    {
        m_n_queries = string_set.size();
        m_f_index = f_index; m_r_index = r_index;
        const int64 n = int64(m_n_queries);
        std::vector< std::vector<rank_type> > per_string(m_n_queries);
        #pragma omp parallel
        {
            std::vector<uint4> store, store2;
            #pragma omp for schedule(dynamic, 256)
            for (int64 q = 0; q < n; ++q)
            {
                const typename string_set_type::string_type s = string_set[uint32(q)];
                if (length(s) > 65535u) continue;       // refused below
                if (split_len == uint32(-1))
                    fmindex::string_mems(s, uint32(length(s)), uint32(q), m_f_index, m_r_index, min_intv ? min_intv : 1u, max_intv, min_span, per_string[q], store);
                else
                    fmindex::string_mems_split(s, uint32(length(s)), uint32(q), m_f_index, m_r_index, min_intv ? min_intv : 1u, max_intv, min_span, split_len, split_width,
                                               per_string[q], store, store2);
            }
        }
        uint64 total = 0;
        for (int64 q = 0; q < n; ++q)
        {
            if (length(string_set[uint32(q)]) > 65535u) throw std::runtime_error("MEMFilter::rank: a pattern is longer than 65 535 symbols");
            total += per_string[q].size();
        }
        m_index.resize(m_n_queries + 1u);
        m_mem_ranges.resize(total);
        m_slots.resize(total);
        m_n_occurrences = fmindex::flatten_mems(per_string, total, m_index.data(), [this](const uint64 at, const rank_type& r) { m_mem_ranges[at] = r; }, m_slots.data());
        return m_n_occurrences;
    }

    /// global index of the first hit of a string's MEMs
    uint64 first_hit(const uint32 string_id) const { const uint64 r = m_index[string_id]; return r ? m_slots[r - 1u] : 0u; }

    /// mems[h - begin] = (text position, string id, span) of global hit h, begin <= h < end
    template <typename mems_iterator>
    void locate(const uint64 begin, const uint64 end, mems_iterator mems)
    {
        const int64 n = int64(end - begin);
        const uint64 n_ranges = m_slots.size();
        #pragma omp parallel for schedule(dynamic, 1024)
        for (int64 h = 0; h < n; ++h)
        {
            const uint64 g = begin + uint64(h);
            const uint64 lo = nvbio::upper_bound_index(g, m_slots.data(), n_ranges);
            const rank_type& r = m_mem_ranges[lo];
            const coord_type row = coord_type(r.coords.x + coord_type(g - (lo ? m_slots[lo - 1u] : 0u)));
            mems[h] = mem_type(nvbio::locate(m_f_index, row), r.string_id(), r.span());
        }
    }

    uint64           n_hits()   const { return m_n_occurrences; }
    uint64           n_mems()   const { return m_n_occurrences; }
    uint64           n_ranges() const { return m_mem_ranges.size(); }
    const rank_type* ranges()   const { return m_mem_ranges.data(); }
    const uint64*    ranks()    const { return m_slots.data(); }
    const uint64*    index()    const { return m_index.data(); }      ///< first range of every string, n + 1 entries

    uint32                  m_n_queries;
    index_type              m_f_index, m_r_index;
    uint64                  m_n_occurrences;
    std::vector<rank_type>  m_mem_ranges;
    std::vector<uint64>     m_slots;
    std::vector<uint64>     m_index;
};

// ---------------------------------------------------------------------------------------- device   (mem.h:378-449)
#if defined(__HIPCC__)
namespace fmindex {

/// the delegate of the device filter's lanes: counts the reported MEMs of one string and, when `out` is set, writes them at `at`
template <typename coord_type>
struct mem_lane_handler
{
    typedef typename vector_type<coord_type, 2u>::type range_type;
    MEMRange<coord_type>* out; uint64* sizes; uint64 at; uint32 n, string_id, max_intv;
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE void output(const range_type range, const uint2 span)
    {
        const coord_type size = coord_type(coord_type(1u) + range.y - range.x);
        if (uint64(size) > uint64(max_intv)) return;
        if (out) { out[at + n] = MEMRange<coord_type>(range, string_id, span); sizes[at + n] = uint64(size); }
        ++n;
    }
};

template <typename string_set_type>
__global__ void __launch_bounds__(128) mem_max_length_kernel(const uint32 n, const string_set_type string_set, uint32* max_len)
{
    const uint32 q = blockIdx.x * 128u + threadIdx.x;
    if (q < n) atomicMax(max_len, uint32(length(string_set[q])));
}
/// one lane per string: the walk of find_kmems; index == NULL counts (counts[q] = the string's MEMs), else writes at index[q]
template <typename index_type, typename string_set_type>
__global__ void __launch_bounds__(128) mem_rank_kernel(const uint32 n, const index_type f_index, const index_type r_index, const string_set_type string_set,
                                                       const uint32 min_intv, const uint32 max_intv, const uint32 min_span, uint4* store, const uint32 max_len,
                                                       uint64* counts, const uint64* index, MEMRange<typename index_type::index_type>* out, uint64* sizes)
{
    const uint32 q = blockIdx.x * 128u + threadIdx.x;
    if (q >= n) return;
    const typename string_set_type::string_type s = string_set[q];
    const uint32 len = uint32(length(s)) < max_len ? uint32(length(s)) : max_len;
    uint4* my_store = store + size_t(q) * max_len;
    mem_lane_handler<typename index_type::index_type> handler = { index ? out : NULL, sizes, index ? index[q] : 0u, 0u, q, max_intv };
    walk_kmems(len, s, f_index, r_index, handler, min_intv, min_span, my_store);
    if (!index) counts[q] = handler.n;
}
/// the sink of a re-seeding lane: counts every span and, given the string's segment of the staging table, puts it at its place
/// by (begin, end) unless it is there already -- from the back: the base MEMs come in order, a re-seed lands near its candidate
template <typename coord_type>
struct mem_lane_sink
{
    typedef typename vector_type<coord_type, 2u>::type range_type;
    MEMRange<coord_type>* seg; uint32 raw, kept, string_id;
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE void output(const range_type range, const uint2 span)
    {
        ++raw;
        if (!seg) return;
        const uint32 key = span_key(span.x | (span.y << 16));
        uint32 p = kept;
        for (; p > 0u; --p)
        {
            const uint32 other = span_key(uint32(seg[p - 1u].coords.w));
            if (other == key) return;
            if (other < key) break;
        }
        for (uint32 k = kept; k > p; --k) seg[k] = seg[k - 1u];
        seg[p] = MEMRange<coord_type>(range, string_id, span);
        ++kept;
    }
};
/// one lane per string: the walk of find_kmems, every candidate re-seeded as it is reported.  raw_index == NULL counts
/// (counts[q] = the spans found, duplicates included); else the spans go to staging + raw_index[q], each once and in order, the
/// rest of the segment is filled with records that name the string, and counts[q] = the spans kept.  store: 2 * max_len a lane.
template <typename index_type, typename string_set_type>
__global__ void __launch_bounds__(128) mem_rank_split_kernel(const uint32 n, const index_type f_index, const index_type r_index, const string_set_type string_set,
                                                             const uint32 min_intv, const uint32 max_intv, const uint32 min_span, const uint32 split_len, const uint32 split_width,
                                                             uint4* store, const uint32 max_len, uint64* counts, const uint64* raw_index,
                                                             MEMRange<typename index_type::index_type>* staging)
{
    typedef typename index_type::index_type      coord_type;
    typedef typename string_set_type::string_type string_type;
    typedef mem_lane_sink<coord_type>            sink_type;
    const uint32 q = blockIdx.x * 128u + threadIdx.x;
    if (q >= n) return;
    const string_type s = string_set[q];
    const uint32 len = uint32(length(s)) < max_len ? uint32(length(s)) : max_len;
    uint4* my_store  = store + size_t(q) * 2u * max_len;
    uint4* my_store2 = my_store + max_len;
    sink_type sink = { raw_index ? staging + raw_index[q] : NULL, 0u, 0u, q };
    mem_split_handler<string_type, index_type, sink_type, uint4*> handler(len, s, f_index, r_index, sink, my_store2, max_intv, min_span, split_len, split_width, NULL);
    walk_kmems(len, s, f_index, r_index, handler, min_intv, min_span, my_store);
    if (raw_index)
        for (uint32 k = sink.kept; k < sink.raw; ++k) sink.seg[k] = MEMRange<coord_type>(make_vector(coord_type(0u), coord_type(0u)), q, make_uint2(0u, 0u));
    counts[q] = raw_index ? sink.kept : sink.raw;
}
/// one lane per staged slot: the first index[q + 1] - index[q] slots of string q's segment are its records
template <typename coord_type>
__global__ void __launch_bounds__(128) mem_compact_kernel(const uint32 n_raw, const MEMRange<coord_type>* staging, const uint64* raw_index, const uint64* index,
                                                          MEMRange<coord_type>* out, uint64* sizes)
{
    const uint32 t = blockIdx.x * 128u + threadIdx.x;
    if (t >= n_raw) return;
    const MEMRange<coord_type> r = staging[t];
    const uint32 q = r.string_id();
    const uint64 first = index[q], pos = t - raw_index[q];
    if (pos >= index[q + 1u] - first) return;
    out[first + pos] = r; sizes[first + pos] = uint64(r.range_size());
}
template <typename index_type, typename mems_iterator>
__global__ void __launch_bounds__(128) mem_locate_kernel(const uint64 begin, const uint32 n_hits, const index_type index, const uint64 n_ranges, const uint64* slots,
                                                         const MEMRange<typename index_type::index_type>* ranges, mems_iterator mems)
{
    typedef typename index_type::index_type coord_type;
    const uint32 h = blockIdx.x * 128u + threadIdx.x;
    if (h >= n_hits) return;
    const uint64 g = begin + h;
    const uint64 lo = nvbio::upper_bound_index(g, slots, n_ranges);
    if (lo >= n_ranges) return;
    const MEMRange<coord_type> r = ranges[lo];
    const coord_type row = coord_type(r.coords.x + coord_type(g - (lo ? slots[lo - 1u] : 0u)));
    mems[h] = MEMHit<coord_type>(locate(index, row), r.string_id(), r.span());
}

} // namespace fmindex

/// The device filter picks one of two executions with identical results (last_path() says which), as FMIndexFilter does:
///   * tuned   -- both indices are the production layout and the strings are windows of 2- or 4-bit packed words: the C-ABI's
///                nvbio_hip_fm_mem_rank / nvbio_hip_fm_mem_locate run the gfx950 kernels;
///   * generic -- any other fm_index<> / string set: one lane per string runs find_kmems, twice (count, hipCUB scan, write),
///                one lane per hit runs upper_bound + locate().
/// Both honour split_len / split_width: the tuned one through nvbio_hip_fm_mem_rank_split, the generic one with lanes that re-seed
/// their candidates as they report them and keep each string's spans in order and once in a staging table.
template <typename fm_index_type>
struct MEMFilter<device_tag, fm_index_type>
{
    typedef device_tag                      system_tag;
    typedef fm_index_type                   index_type;
    typedef typename index_type::index_type coord_type;
    static const uint32                     coord_dim = vector_traits<coord_type>::DIM;
    typedef MEMRange<coord_type>            rank_type;
    typedef MEMHit<coord_type>              mem_type;
    typedef mem_type                        hit_type;

    MEMFilter() : m_n_queries(0), m_n_occurrences(0), m_n_ranges(0), m_path("none"), m_stream(0), m_tuned(false), m_allow_tuned(true) {}

    void set_stream(hipStream_t s) { m_stream = s; }
    /// whether rank() and locate() may take the tuned execution (default: yes); off, every index and string set runs the templates
    void set_tuned(const bool on) { m_allow_tuned = on; }
    const char* last_path() const { return m_path; }

    /// returns the total number of MEM occurrences
    template <typename string_set_type>
    uint64 rank(const fm_index_type& f_index, const fm_index_type& r_index, const string_set_type& string_set,
                const uint32 min_intv = 1u, const uint32 max_intv = uint32(-1), const uint32 min_span = 1u,
                const uint32 split_len = uint32(-1), const uint32 split_width = uint32(-1))
    {
        m_n_queries = string_set.size();
        m_f_index = f_index; m_r_index = r_index;
        m_n_occurrences = 0; m_n_ranges = 0; m_tuned = false;
        const uint32 n = m_n_queries, k = min_intv ? min_intv : 1u;
        uint64* index = m_index.reserve(uint64(n) + 1u);
        fmindex::check(hipMemsetAsync(index, 0, (uint64(n) + 1u) * sizeof(uint64), m_stream), "hipMemsetAsync");
        if (n == 0) { m_path = "none"; return 0; }
        // the longest string
        uint32 max_len = 0;
        uint32* d_max = reinterpret_cast<uint32*>(m_temp.reserve(256u));
        fmindex::check(hipMemsetAsync(d_max, 0, sizeof(uint32), m_stream), "hipMemsetAsync");
        hipLaunchKernelGGL((fmindex::mem_max_length_kernel<string_set_type>), dim3((n + 127u) / 128u), dim3(128), 0, m_stream, n, string_set, d_max);
        fmindex::check(hipMemcpyAsync(&max_len, d_max, sizeof(uint32), hipMemcpyDeviceToHost, m_stream), "hipMemcpyAsync");
        fmindex::check(hipStreamSynchronize(m_stream), "hipStreamSynchronize");
        if (max_len > 65535u) throw std::runtime_error("MEMFilter::rank: a pattern is longer than 65 535 symbols");
        if (max_len == 0u) { m_path = "none"; return 0; }
        typedef typename string_set_type::string_type string_type;
        const bool tuned = rank_tuned(string_set, max_len, k, max_intv, min_span, split_len, split_width,
                                      std::integral_constant<bool, fmindex::production_layout<fm_index_type>::ok && nvbio::priv::packed_view<string_type>::ok>());
        if (!tuned && split_len != uint32(-1))
        {
            // count every span, scan, stage each string's spans in order and once, count again, scan, move them to their places
            uint4*  store     = reinterpret_cast<uint4*>(m_store.reserve(uint64(n) * 2u * max_len * sizeof(uint4)));
            uint64* raw_index = m_raw_index.reserve(uint64(n) + 1u);
            fmindex::check(hipMemsetAsync(raw_index, 0, sizeof(uint64), m_stream), "hipMemsetAsync");
            const uint64 raw = count_pass(raw_index + 1, n, "mem_rank_split_kernel", [&]() {
                hipLaunchKernelGGL((fmindex::mem_rank_split_kernel<fm_index_type, string_set_type>), dim3((n + 127u) / 128u), dim3(128), 0, m_stream, n, m_f_index, m_r_index,
                                   string_set, k, max_intv, min_span, split_len, split_width, store, max_len, raw_index + 1, (const uint64*)NULL, (rank_type*)NULL); });
            uint64 total = 0;
            if (raw)
            {
                rank_type* staging = m_staging.reserve(raw);
                total = count_pass(index + 1, n, "mem_rank_split_kernel", [&]() {
                    hipLaunchKernelGGL((fmindex::mem_rank_split_kernel<fm_index_type, string_set_type>), dim3((n + 127u) / 128u), dim3(128), 0, m_stream, n, m_f_index, m_r_index,
                                       string_set, k, max_intv, min_span, split_len, split_width, store, max_len, index + 1, (const uint64*)raw_index, staging); });
                rank_type* ranges = m_mem_ranges.reserve(total);
                uint64*    slots  = m_slots.reserve(total);
                hipLaunchKernelGGL((fmindex::mem_compact_kernel<coord_type>), dim3((uint32(raw) + 127u) / 128u), dim3(128), 0, m_stream, uint32(raw),
                                   (const rank_type*)staging, (const uint64*)raw_index, (const uint64*)index, ranges, slots);
                fmindex::check(hipGetLastError(), "mem_compact_kernel");
                scan(slots, uint32(total));
            }
            m_n_ranges = total;
            m_path = "generic";
        }
        else if (!tuned)
        {
            uint4* store = reinterpret_cast<uint4*>(m_store.reserve(uint64(n) * max_len * sizeof(uint4)));
            const uint64 total = count_pass(index + 1, n, "mem_rank_kernel", [&]() {
                hipLaunchKernelGGL((fmindex::mem_rank_kernel<fm_index_type, string_set_type>), dim3((n + 127u) / 128u), dim3(128), 0, m_stream, n, m_f_index, m_r_index,
                                   string_set, k, max_intv, min_span, store, max_len, index + 1, (const uint64*)NULL, (rank_type*)NULL, (uint64*)NULL); });
            rank_type* ranges = m_mem_ranges.reserve(total);
            uint64*    slots  = m_slots.reserve(total);
            if (total)
            {
                hipLaunchKernelGGL((fmindex::mem_rank_kernel<fm_index_type, string_set_type>), dim3((n + 127u) / 128u), dim3(128), 0, m_stream, n, m_f_index, m_r_index,
                                   string_set, k, max_intv, min_span, store, max_len, (uint64*)NULL, (const uint64*)index, ranges, slots);
                fmindex::check(hipGetLastError(), "mem_rank_kernel");
                scan(slots, uint32(total));
            }
            m_n_ranges = total;
            m_path = "generic";
        }
        if (m_n_ranges)
        {
            fmindex::check(hipMemcpyAsync(&m_n_occurrences, m_slots.ptr + (m_n_ranges - 1u), sizeof(uint64), hipMemcpyDeviceToHost, m_stream), "hipMemcpyAsync");
            fmindex::check(hipStreamSynchronize(m_stream), "hipStreamSynchronize");
        }
        return m_n_occurrences;
    }

    /// global index of the first hit of a string's MEMs
    uint64 first_hit(const uint32 string_id) const
    {
        uint64 r = 0, h = 0;
        fmindex::check(hipMemcpy(&r, m_index.ptr + string_id, sizeof(uint64), hipMemcpyDeviceToHost), "hipMemcpy");
        if (r) fmindex::check(hipMemcpy(&h, m_slots.ptr + (r - 1u), sizeof(uint64), hipMemcpyDeviceToHost), "hipMemcpy");
        return h;
    }

    /// mems: any device iterator of mem_type.  The call returns after queueing the work.
    template <typename mems_iterator>
    void locate(const uint64 begin, const uint64 end, mems_iterator mems)
    {
        if (end <= begin || m_n_ranges == 0) return;
        if (end - begin > 0xFFFFFFFFull) throw std::runtime_error("MEMFilter::locate: more than 2^32 - 1 hits in one call");
        const uint32 n_hits = uint32(end - begin);
        if (locate_tuned(begin, end, mems, std::integral_constant<bool, fmindex::production_layout<fm_index_type>::ok && nvbio::priv::plain_iterator<mems_iterator>::ok && sizeof(mem_type) == 16u>())) return;
        hipLaunchKernelGGL((fmindex::mem_locate_kernel<fm_index_type, mems_iterator>), dim3((n_hits + 127u) / 128u), dim3(128), 0, m_stream,
                           begin, n_hits, m_f_index, m_n_ranges, m_slots.ptr, m_mem_ranges.ptr, mems);
        fmindex::check(hipGetLastError(), "mem_locate_kernel");
        m_path = "generic";
    }

    uint64           n_hits()   const { return m_n_occurrences; }
    uint64           n_mems()   const { return m_n_occurrences; }
    uint64           n_ranges() const { return m_n_ranges; }
    const rank_type* ranges()   const { return m_mem_ranges.ptr; }     ///< device memory
    const uint64*    ranks()    const { return m_slots.ptr; }          ///< device memory
    const uint64*    index()    const { return m_index.ptr; }          ///< device memory: first range of every string, n + 1 entries

private:
    void scan(uint64* values, const uint32 n)
    {
        size_t tb = 0;
        fmindex::check(hipcub::DeviceScan::InclusiveSum(nullptr, tb, values, values, int(n), m_stream), "hipcub::DeviceScan::InclusiveSum");
        uint8* temp = m_temp.reserve(tb + 16u);
        fmindex::check(hipcub::DeviceScan::InclusiveSum(temp, tb, values, values, int(n), m_stream), "hipcub::DeviceScan::InclusiveSum");
    }
    /// one counting pass of a generic rank: `launch` runs a kernel that leaves a count per string in counts[0, n); they are scanned
    /// in place, and their total comes back
    template <typename launch_type>
    uint64 count_pass(uint64* counts, const uint32 n, const char* kernel, launch_type launch)
    {
        launch();
        fmindex::check(hipGetLastError(), kernel);
        scan(counts, n);
        uint64 total = 0;
        fmindex::check(hipMemcpyAsync(&total, counts + (n - 1u), sizeof(uint64), hipMemcpyDeviceToHost, m_stream), "hipMemcpyAsync");
        fmindex::check(hipStreamSynchronize(m_stream), "hipStreamSynchronize");
        if (total > 0x7FFFFFFFull) throw std::runtime_error("MEMFilter::rank: more than 2^31 - 1 MEMs in one call");
        return total;
    }
    template <typename string_set_type>
    bool rank_tuned(const string_set_type&, const uint32, const uint32, const uint32, const uint32, const uint32, const uint32, std::false_type) { return false; }
    template <typename mems_iterator>
    bool locate_tuned(const uint64, const uint64, mems_iterator, std::false_type) { return false; }

    template <typename string_set_type>
    bool rank_tuned(const string_set_type& string_set, const uint32 max_len, const uint32 min_intv, const uint32 max_intv, const uint32 min_span,
                    const uint32 split_len, const uint32 split_width, std::true_type)
    {
#if defined(NVBIO_HIP_COMPAT_FILTER_TUNED)
        typedef typename string_set_type::string_type string_type;
        typedef nvbio::priv::packed_view<string_type> view;
        if (!m_allow_tuned || (view::BITS != 2u && view::BITS != 4u)) return false;
        if (!fmindex::production_layout<fm_index_type>::describe(m_f_index, m_f_fmi) || !fmindex::production_layout<fm_index_type>::describe(m_r_index, m_r_fmi)) return false;
        const uint32 n = m_n_queries;
        // the strings in place: a job table of (offset, length) into the caller's own words
        uint8* base = m_jobs.reserve(64u + uint64(n) * 12u + 16u);
        unsigned long long* bounds = reinterpret_cast<unsigned long long*>(base);
        uint64* begin = reinterpret_cast<uint64*>(base + 64u);
        uint32* len   = reinterpret_cast<uint32*>(begin + n);
        hipLaunchKernelGGL(fmindex::filter_init_bounds_kernel, dim3(1), dim3(64), 0, m_stream, bounds);
        hipLaunchKernelGGL((fmindex::filter_describe_kernel<string_set_type>), dim3((n + 127u) / 128u), dim3(128), 0, m_stream, n, string_set, begin, len, bounds);
        unsigned long long b[2];
        fmindex::check(hipMemcpyAsync(b, bounds, sizeof(b), hipMemcpyDeviceToHost, m_stream), "hipMemcpyAsync");
        fmindex::check(hipStreamSynchronize(m_stream), "hipStreamSynchronize");
        if (b[1] == 0ull) { b[0] = 0ull; b[1] = 1ull; }
        hipLaunchKernelGGL(fmindex::filter_rebase_kernel, dim3((n + 255u) / 256u), dim3(256), 0, m_stream, n, begin, uint64(b[0]) * (32u / view::BITS));
        nvbio_hip_string_set strings;
        strings.words = reinterpret_cast<const uint32*>(uintptr_t(b[0]) * 4u); strings.n_words = b[1] - b[0];
        strings.bits = view::BITS; strings.big_endian = view::BE ? 1u : 0u;
        strings.begin = begin; strings.length = len; strings.fixed_length = 0; strings._pad = 0;
        const bool split = split_len != uint32(-1);          // re-seeding: its own entry, whose scratch grows with the capacity
        uint64 capacity = split ? 16ull * n + 1024u : (uint64(n) * max_len < 8ull * n + 1024u ? uint64(n) * max_len : 8ull * n + 1024u), found = 0;
        for (int attempt = 0; attempt < 2; ++attempt)      // at most one retry, with the number the library found
        {
            const uint64 tb = split ? nvbio_hip_fm_mem_split_temp_bytes(n, max_len, capacity) : nvbio_hip_fm_mem_temp_bytes(n, max_len);
            uint8* temp = m_store.reserve(tb + 16u);
            rank_type* ranges = m_mem_ranges.reserve(capacity);
            uint64*    slots  = m_slots.reserve(capacity);
            const int err = split ?
                nvbio_hip_fm_mem_rank_split(&m_f_fmi, &m_r_fmi, &strings, n, max_len, min_intv, max_intv, min_span, split_len, split_width, reinterpret_cast<uint32*>(ranges), capacity,
                                            m_index.ptr, slots, &found, temp, tb, m_stream) :
                nvbio_hip_fm_mem_rank(&m_f_fmi, &m_r_fmi, &strings, n, max_len, min_intv, max_intv, min_span, reinterpret_cast<uint32*>(ranges), capacity,
                                      m_index.ptr, slots, &found, temp, tb, m_stream);
            if (err == 801) return false;
            if (err != NVBIO_HIP_ERROR_CAPACITY || attempt == 1) { fmindex::check(err, split ? "nvbio_hip_fm_mem_rank_split" : "nvbio_hip_fm_mem_rank"); break; }
            capacity = found;
        }
        m_n_ranges = found;
        m_tuned = true; m_path = "tuned";
        return true;
#else
        (void)string_set; (void)max_len; (void)min_intv; (void)max_intv; (void)min_span; (void)split_len; (void)split_width; return false;
#endif
    }
    template <typename mems_iterator>
    bool locate_tuned(const uint64 begin, const uint64 end, mems_iterator mems, std::true_type)
    {
#if defined(NVBIO_HIP_COMPAT_FILTER_TUNED)
        if (!m_allow_tuned) return false;
        if (!m_tuned && !fmindex::production_layout<fm_index_type>::describe(m_f_index, m_f_fmi)) return false;
        const int err = nvbio_hip_fm_mem_locate(&m_f_fmi, reinterpret_cast<const uint32*>(m_mem_ranges.ptr), m_slots.ptr, m_n_ranges, begin, end,
                                                reinterpret_cast<uint32*>(nvbio::priv::plain_iterator<mems_iterator>::get(mems)), m_stream);
        if (err == 801) return false;
        fmindex::check(err, "nvbio_hip_fm_mem_locate");
        m_path = "tuned";
        return true;
#else
        (void)begin; (void)end; (void)mems; return false;
#endif
    }
#if defined(NVBIO_HIP_COMPAT_FILTER_TUNED)
    nvbio_hip_fmindex                 m_f_fmi, m_r_fmi;
#endif
public:
    uint32                            m_n_queries;
    index_type                        m_f_index, m_r_index;
    uint64                            m_n_occurrences, m_n_ranges;
private:
    fmindex::device_array<rank_type>  m_mem_ranges;
    fmindex::device_array<rank_type>  m_staging;
    fmindex::device_array<uint64>     m_slots, m_index, m_raw_index;
    fmindex::device_array<uint8>      m_temp, m_jobs, m_store;
    const char*                       m_path;
    hipStream_t                       m_stream;
    bool                              m_tuned, m_allow_tuned;
};

template <typename fm_index_type> struct MEMFilterDevice : public MEMFilter<device_tag, fm_index_type>
{
    typedef MEMFilter<device_tag, fm_index_type> core_type;
    typedef typename core_type::system_tag       system_tag;
    typedef typename core_type::index_type       index_type;
    typedef typename core_type::coord_type       coord_type;
    typedef typename core_type::rank_type        rank_type;
    typedef typename core_type::mem_type         mem_type;
    typedef typename core_type::hit_type         hit_type;
};
#endif // __HIPCC__

template <typename fm_index_type> struct MEMFilterHost : public MEMFilter<host_tag, fm_index_type>
{
    typedef MEMFilter<host_tag, fm_index_type> core_type;
    typedef typename core_type::system_tag     system_tag;
    typedef typename core_type::index_type     index_type;
    typedef typename core_type::coord_type     coord_type;
    typedef typename core_type::rank_type      rank_type;
    typedef typename core_type::mem_type       mem_type;
    typedef typename core_type::hit_type       hit_type;
};

/// the furthest string i such that the strings before it have at most mem_count hits together   (mem.h:451-454)
template <typename system_tag, typename fm_index_type>
uint32 string_batch_bound(const MEMFilter<system_tag, fm_index_type>& filter, const uint32 mem_count)
{
    uint32 lo = 0, hi = filter.m_n_queries;
    while (lo < hi) { const uint32 mid = lo + (hi - lo + 1u) / 2u; if (filter.first_hit(mid) <= uint64(mem_count)) lo = mid; else hi = mid - 1u; }
    return lo;
}

} // namespace nvbio
