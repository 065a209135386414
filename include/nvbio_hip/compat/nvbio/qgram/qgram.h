// compat/nvbio/qgram/qgram.h -- the q-gram index of a string and of a string set behind the reference's own names
// (nvbio/qgram/qgram.h): QGramIndexViewCore / QGramIndexCore, QGramIndexHost / QGramIndexDevice, QGramSetIndexHost /
// QGramSetIndexDevice with the cross-system operator=, plain_view() of an index as a unary functor (q-gram -> slot range),
// string_qgram_functor, string_set_qgram_functor and generate_qgrams.  Definitions: include/nvbio_hip.h, DESIGN.md 3.14.
//
// A device build picks one of two executions, with identical results (last_path() says which):
//   * tuned   -- 2-bit symbols in a PackedStream over a word pointer that starts on a word boundary, or a ConcatenatedStringSet over
//                such a stream (at any symbol) seeded by uniform_seeds_functor(q, interval): the strings are described to the C-ABI
//                in place and nvbio_hip_qgram_index_build / nvbio_hip_qgram_set_index_build run the gfx950 kernels;
//   * generic -- any other string iterator, symbol size or seeding functor: q-grams by string_qgram_functor /
//                string_set_qgram_functor, a stable thrust sort by key, reduce_by_key, a scan and a vectorised lower bound for the LUT.
// Needs a translation unit compiled by hipcc and linked with libnvbio_hip.
#pragma once
#include "../basic/types.h"
#include "../basic/packedstream.h"
#include "../basic/packed_view.h"
#include "../basic/vector.h"
#include "../strings/string_set.h"
#include "../strings/seeds.h"
#include "../sufsort/sufsort.h"
#include <thrust/sort.h>
#include <thrust/reduce.h>
#include <thrust/scan.h>
#include <thrust/transform.h>
#include <thrust/sequence.h>
#include <thrust/binary_search.h>
#include <thrust/iterator/constant_iterator.h>
#include <thrust/iterator/counting_iterator.h>
#include <thrust/iterator/transform_iterator.h>
#include <iterator>
#include <stdexcept>

namespace nvbio {

/// position i -> the q-gram of `string` there: symbol j at bits [j * symbol_size, (j + 1) * symbol_size), symbols past the end 0
template <typename string_type>
struct string_qgram_functor
{
    typedef uint32 argument_type;
    typedef uint64 result_type;

    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE
    string_qgram_functor(const uint32 _Q, const uint32 _symbol_size, const uint32 _string_len, const string_type _string) :
        Q(_Q), symbol_size(_symbol_size), symbol_mask((1u << _symbol_size) - 1u), string_len(_string_len), string(_string) {}

    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE
    uint64 operator()(const uint32 i) const
    {
        uint64 qgram = 0u;
        for (uint32 j = 0; j < Q && i + j < string_len; ++j)
            qgram |= uint64(uint32(string[i + j]) & symbol_mask) << (j * symbol_size);
        return qgram;
    }

    const uint32      Q;
    const uint32      symbol_size;
    const uint32      symbol_mask;
    const uint32      string_len;
    const string_type string;
};

/// (string id, position) -> the q-gram of that string of the set there
template <typename string_set_type>
struct string_set_qgram_functor
{
    typedef uint2  argument_type;
    typedef uint64 result_type;
    typedef typename string_set_type::string_type string_type;

    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE
    string_set_qgram_functor(const uint32 _Q, const uint32 _symbol_size, const string_set_type _string_set) :
        Q(_Q), symbol_size(_symbol_size), symbol_mask((1u << _symbol_size) - 1u), string_set(_string_set) {}

    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE
    uint64 operator()(const uint2 id) const
    {
        const string_type s = string_set[id.x];
        const uint32 len = uint32(length(s));
        uint64 qgram = 0u;
        for (uint32 j = 0; j < Q && id.y + j < len; ++j)
            qgram |= uint64(uint32(s[id.y + j]) & symbol_mask) << (j * symbol_size);
        return qgram;
    }

    const uint32          Q;
    const uint32          symbol_size;
    const uint32          symbol_mask;
    const string_set_type string_set;
};

/// qgrams[k] = the q-gram of `string` at indices[k]
template <typename string_type, typename index_iterator, typename qgram_iterator>
void generate_qgrams(const uint32 q, const uint32 symbol_size, const uint32 string_len, const string_type string, const uint32 n_qgrams,
                     const index_iterator indices, qgram_iterator qgrams)
{
    thrust::transform(indices, indices + n_qgrams, qgrams, string_qgram_functor<string_type>(q, symbol_size, string_len, string));
}

/// qgrams[k] = the q-gram of the set at the (string id, position) pair indices[k]
template <typename string_set_type, typename index_iterator, typename qgram_iterator>
void generate_qgrams(const uint32 q, const uint32 symbol_size, const string_set_type string_set, const uint32 n_qgrams,
                     const index_iterator indices, qgram_iterator qgrams)
{
    thrust::transform(indices, indices + n_qgrams, qgrams, string_set_qgram_functor<string_set_type>(q, symbol_size, string_set));
}

/// the arrays of an index as iterators: what kernels and functors take.  As a functor it maps a q-gram to its slot range.
template <typename QGramVectorType, typename IndexVectorType, typename CoordVectorType>
struct QGramIndexViewCore
{
    typedef QGramVectorType                                              qgram_vector_type;
    typedef IndexVectorType                                              index_vector_type;
    typedef CoordVectorType                                              coord_vector_type;
    typedef typename std::iterator_traits<qgram_vector_type>::value_type qgram_type;
    typedef typename std::iterator_traits<coord_vector_type>::value_type coord_type;

    typedef QGramIndexViewCore<QGramVectorType, IndexVectorType, CoordVectorType> plain_view_type;
    typedef QGramIndexViewCore<QGramVectorType, IndexVectorType, CoordVectorType> const_plain_view_type;

    typedef qgram_type argument_type;
    typedef uint2      result_type;

    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE
    QGramIndexViewCore() : Q(0), symbol_size(0), n_qgrams(0), n_unique_qgrams(0), QL(0), QLS(0) {}

    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE
    QGramIndexViewCore(const uint32 _Q, const uint32 _symbol_size, const uint32 _n_qgrams, const uint32 _n_unique_qgrams,
                       const qgram_vector_type _qgrams, const index_vector_type _slots, const coord_vector_type _index,
                       const uint32 _QL, const uint32 _QLS, const index_vector_type _lut) :
        Q(_Q), symbol_size(_symbol_size), n_qgrams(_n_qgrams), n_unique_qgrams(_n_unique_qgrams), QL(_QL), QLS(_QLS),
        qgrams(_qgrams), slots(_slots), index(_index), lut(_lut) {}

    /// the slots of q-gram g in `index`, (0, 0) if it is not indexed
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE
    uint2 range(const qgram_type g) const
    {
        uint32 lo = 0u, hi = n_unique_qgrams;
        if (QL)                                 // with no LUT the shift, which may be as wide as the word, is never evaluated
        {
            const uint64 k = uint64(g) >> QLS;
            if ((k >> (QL * symbol_size)) != 0u) return make_uint2(0u, 0u);      // more than Q symbols: not a q-gram, and past the LUT
            lo = lut[k]; hi = lut[k + 1u];
        }
        while (lo < hi) { const uint32 mid = lo + (hi - lo) / 2u; if (qgrams[mid] < g) lo = mid + 1u; else hi = mid; }
        if (lo >= n_unique_qgrams || !(qgrams[lo] == g)) return make_uint2(0u, 0u);
        return make_uint2(slots[lo], slots[lo + 1u]);
    }

    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE
    uint2 operator()(const qgram_type g) const { return range(g); }

    /// the coordinate in slot i
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE
    coord_type locate(const uint32 i) const { return index[i]; }

    uint32            Q;
    uint32            symbol_size;
    uint32            n_qgrams;
    uint32            n_unique_qgrams;
    uint32            QL;
    uint32            QLS;
    qgram_vector_type qgrams;
    index_vector_type slots;
    coord_vector_type index;
    index_vector_type lut;
};

/// the storage of an index in the memory of a system
template <typename SystemTag, typename QGramType, typename IndexType, typename CoordType>
struct QGramIndexCore
{
    typedef SystemTag                            system_tag;
    typedef QGramType                            qgram_type;
    typedef IndexType                            index_type;
    typedef CoordType                            coord_type;
    typedef nvbio::vector<system_tag, qgram_type> qgram_vector_type;
    typedef nvbio::vector<system_tag, index_type> index_vector_type;
    typedef nvbio::vector<system_tag, coord_type> coord_vector_type;

    typedef QGramIndexViewCore<QGramType*, IndexType*, CoordType*>                   plain_view_type;
    typedef QGramIndexViewCore<const QGramType*, const IndexType*, const CoordType*> const_plain_view_type;

    QGramIndexCore() : Q(0), symbol_size(0), n_qgrams(0), n_unique_qgrams(0), QL(0), QLS(0), m_path("none") {}

    uint64 bytes() const
    {
        return qgrams.size() * sizeof(qgram_type) + slots.size() * sizeof(index_type) + index.size() * sizeof(coord_type) + lut.size() * sizeof(index_type);
    }
    uint64 used_host_memory()   const { return same_type<system_tag, host_tag>::pred ? bytes() : 0u; }
    uint64 used_device_memory() const { return same_type<system_tag, device_tag>::pred ? bytes() : 0u; }

    /// "tuned" or "generic": the execution the last build() took
    const char* last_path() const { return m_path; }

    template <typename OtherTag>
    void copy_from(const QGramIndexCore<OtherTag, QGramType, IndexType, CoordType>& src)
    {
        Q = src.Q; symbol_size = src.symbol_size; n_qgrams = src.n_qgrams; n_unique_qgrams = src.n_unique_qgrams; QL = src.QL; QLS = src.QLS;
        qgrams = src.qgrams; slots = src.slots; index = src.index; lut = src.lut;
    }

    uint32            Q;
    uint32            symbol_size;
    uint32            n_qgrams;
    uint32            n_unique_qgrams;
    qgram_vector_type qgrams;
    index_vector_type slots;
    coord_vector_type index;
    uint32            QL;
    uint32            QLS;
    index_vector_type lut;
    const char*       m_path;
};

typedef QGramIndexViewCore<uint64*, uint32*, uint32*>                   QGramIndexView;
typedef QGramIndexViewCore<uint64*, uint32*, uint2*>                    QGramSetIndexView;
typedef QGramIndexViewCore<const uint64*, const uint32*, const uint32*> ConstQGramIndexView;
typedef QGramIndexViewCore<const uint64*, const uint32*, const uint2*>  ConstQGramSetIndexView;

template <typename SystemTag, typename QT, typename IT, typename CT>
QGramIndexViewCore<QT*, IT*, CT*> plain_view(QGramIndexCore<SystemTag, QT, IT, CT>& ix)
{
    return QGramIndexViewCore<QT*, IT*, CT*>(ix.Q, ix.symbol_size, ix.n_qgrams, ix.n_unique_qgrams, raw_pointer(ix.qgrams), raw_pointer(ix.slots),
                                            raw_pointer(ix.index), ix.QL, ix.QLS, raw_pointer(ix.lut));
}
template <typename SystemTag, typename QT, typename IT, typename CT>
QGramIndexViewCore<const QT*, const IT*, const CT*> plain_view(const QGramIndexCore<SystemTag, QT, IT, CT>& ix)
{
    return QGramIndexViewCore<const QT*, const IT*, const CT*>(ix.Q, ix.symbol_size, ix.n_qgrams, ix.n_unique_qgrams, raw_pointer(ix.qgrams),
                                                              raw_pointer(ix.slots), raw_pointer(ix.index), ix.QL, ix.QLS, raw_pointer(ix.lut));
}

namespace qgram {

inline void check(const int err, const char* what)
{
    if (err != 0) throw std::runtime_error(std::string("nvbio qgram: ") + what + " failed with hipError " + std::to_string(err));
}

struct lut_key
{
    typedef uint64 argument_type;
    typedef uint64 result_type;
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE lut_key(const uint32 s) : shift(s) {}
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE uint64 operator()(const uint64 k) const { return k << shift; }
    const uint32 shift;
};

inline void set_parameters(const uint32 q, const uint32 symbol_sz, const uint32 qlut, uint32& Q, uint32& symbol_size, uint32& QL, uint32& QLS)
{
    if (q == 0u || symbol_sz == 0u || q * symbol_sz > 64u) throw std::runtime_error("nvbio qgram: a q-gram must hold between 1 symbol and 64 bits");
    if (qlut > q || qlut * symbol_sz > 32u) throw std::runtime_error("nvbio qgram: the LUT may index at most q symbols and 32 bits");
    Q = q; symbol_size = symbol_sz; QL = qlut; QLS = (q - qlut) * symbol_sz;
}

/// keys / coords in enumeration order -> the arrays of the index, in the memory of the index's system
template <typename core_type>
void build_generic(core_type& ix, typename core_type::qgram_vector_type& keys, typename core_type::coord_vector_type& coords)
{
    typedef typename core_type::system_tag system_tag;
    typedef typename core_type::index_type index_type;
    const uint32 n = uint32(keys.size());
    ix.n_qgrams = n;
    thrust::stable_sort_by_key(nvbio::priv::exec_policy(system_tag()), keys.begin(), keys.end(), coords.begin());
    ix.index.swap(coords);
    ix.qgrams.resize(n);
    typename core_type::index_vector_type counts(n);
    const uint32 n_unique = uint32(thrust::reduce_by_key(nvbio::priv::exec_policy(system_tag()), keys.begin(), keys.end(), thrust::make_constant_iterator<index_type>(1u),
                                                         ix.qgrams.begin(), counts.begin()).first - ix.qgrams.begin());
    ix.n_unique_qgrams = n_unique;
    ix.qgrams.resize(n_unique);
    ix.slots.resize(n_unique + 1u);
    thrust::exclusive_scan(nvbio::priv::exec_policy(system_tag()), counts.begin(), counts.begin() + n_unique, ix.slots.begin(), index_type(0));
    ix.slots[n_unique] = n;
    ix.lut.resize(0);
    if (ix.QL)
    {
        const uint64 n_keys = uint64(1) << (ix.QL * ix.symbol_size);
        ix.lut.resize(n_keys + 1u);
        thrust::lower_bound(nvbio::priv::exec_policy(system_tag()), ix.qgrams.begin(), ix.qgrams.end(),
                            thrust::make_transform_iterator(thrust::make_counting_iterator<uint64>(0u), lut_key(ix.QLS)),
                            thrust::make_transform_iterator(thrust::make_counting_iterator<uint64>(0u), lut_key(ix.QLS)) + n_keys, ix.lut.begin());
        ix.lut[n_keys] = n_unique;
    }
    ix.m_path = "generic";
}

/// size the arrays for n q-grams, run a C-ABI build through `call`, cut them to what it found
template <typename core_type, typename F>
void build_tuned(core_type& ix, const uint64 n, const uint64 temp_bytes, F call)
{
    if (n > 0xFFFFFFFFull) throw std::runtime_error("nvbio qgram: at most 2^32 - 1 q-grams can be indexed");
    ix.n_qgrams = uint32(n);
    ix.qgrams.resize(n); ix.slots.resize(n + 1u); ix.index.resize(n);
    ix.lut.resize(ix.QL ? (uint64(1) << (2u * ix.QL)) + 1u : 0u);
    sufsort::scratch temp(temp_bytes);
    uint32 n_unique = 0u;
    check(call(raw_pointer(ix.qgrams), raw_pointer(ix.slots), reinterpret_cast<uint32*>(raw_pointer(ix.index)), raw_pointer(ix.lut), &n_unique, temp.ptr),
          "the q-gram index build");
    ix.n_unique_qgrams = n_unique;
    ix.qgrams.resize(n_unique); ix.slots.resize(n_unique + 1u);
    ix.m_path = "tuned";
}

/// whether a seeding functor is uniform_seeds_functor, whose seeds the C-ABI enumerates itself
template <typename F> struct uniform_seeder { static const bool ok = false; static uint32 len(const F&) { return 0u; } static uint32 interval(const F&) { return 0u; } };
template <typename I> struct uniform_seeder< uniform_seeds_functor<I> >
{
    static const bool ok = true;
    static uint32 len(const uniform_seeds_functor<I>& f) { return f.len; }
    static uint32 interval(const uniform_seeds_functor<I>& f) { return f.interval; }
};

} // namespace qgram

struct QGramIndexHost : public QGramIndexCore<host_tag, uint64, uint32, uint32>
{
    typedef host_tag                                        system_tag;
    typedef QGramIndexCore<host_tag, uint64, uint32, uint32> core_type;
    typedef core_type::qgram_vector_type                    qgram_vector_type;
    typedef core_type::index_vector_type                    index_vector_type;
    typedef core_type::coord_vector_type                    coord_vector_type;
    typedef core_type::qgram_type                           qgram_type;
    typedef core_type::coord_type                           coord_type;
    typedef core_type::plain_view_type                      plain_view_type;
    typedef core_type::const_plain_view_type                const_plain_view_type;

    template <typename SystemTag>
    QGramIndexHost& operator=(const QGramIndexCore<SystemTag, uint64, uint32, uint32>& src) { this->copy_from(src); return *this; }
};

struct QGramIndexDevice : public QGramIndexCore<device_tag, uint64, uint32, uint32>
{
    typedef device_tag                                        system_tag;
    typedef QGramIndexCore<device_tag, uint64, uint32, uint32> core_type;
    typedef core_type::qgram_vector_type                      qgram_vector_type;
    typedef core_type::index_vector_type                      index_vector_type;
    typedef core_type::coord_vector_type                      coord_vector_type;
    typedef core_type::qgram_type                             qgram_type;
    typedef core_type::coord_type                             coord_type;
    typedef core_type::plain_view_type                        plain_view_type;
    typedef core_type::const_plain_view_type                  const_plain_view_type;

    /// index every position of string[0, string_len), the truncated q-grams of the tail included
    template <typename string_type>
    void build(const uint32 q, const uint32 symbol_sz, const uint32 string_len, const string_type string, const uint32 qlut = 0)
    {
        qgram::set_parameters(q, symbol_sz, qlut, Q, symbol_size, QL, QLS);
        typedef nvbio::priv::packed_stream_where<string_type> where_type;
        if (symbol_sz == 2u && qlut <= 16u && build_tuned(string_len, string, std::integral_constant<bool, where_type::ok && where_type::BITS == 2u>())) return;
        qgram_vector_type keys(string_len);
        coord_vector_type coords(string_len);
        thrust::sequence(coords.begin(), coords.end());
        thrust::transform(thrust::device, thrust::make_counting_iterator<uint32>(0u), thrust::make_counting_iterator<uint32>(0u) + string_len, keys.begin(),
                          string_qgram_functor<string_type>(q, symbol_sz, string_len, string));
        qgram::build_generic(*this, keys, coords);
    }

    template <typename SystemTag>
    QGramIndexDevice& operator=(const QGramIndexCore<SystemTag, uint64, uint32, uint32>& src) { this->copy_from(src); return *this; }

private:
    template <typename string_type> bool build_tuned(const uint32, const string_type&, std::false_type) { return false; }
    template <typename string_type> bool build_tuned(const uint32 string_len, const string_type& string, std::true_type)
    {
        typedef nvbio::priv::packed_stream_where<string_type> where_type;
        uint64 word0; uint32 first;
        where_type::where(string, word0, first);
        if (first != 0u || word0 == 0u) return false;
        const uint32* words = reinterpret_cast<const uint32*>(uintptr_t(word0) * 4u);
        const uint64 n_words = string_len ? (uint64(string_len) + 15u) / 16u : 1u;
        const uint32 q = Q, ql = QL;
        qgram::build_tuned(*this, string_len, nvbio_hip_qgram_index_build_temp_bytes(string_len),
            [=](uint64* qg, uint32* sl, uint32* ix, uint32* lu, uint32* nu, void* temp) {
                return nvbio_hip_qgram_index_build(words, n_words, 2u, where_type::BE ? 1u : 0u, string_len, q, ql, qg, sl, ix, ql ? lu : nullptr, nu, temp,
                                                   nvbio_hip_qgram_index_build_temp_bytes(string_len), nullptr); });
        return true;
    }
};

struct QGramSetIndexHost : public QGramIndexCore<host_tag, uint64, uint32, uint2>
{
    typedef host_tag                                       system_tag;
    typedef QGramIndexCore<host_tag, uint64, uint32, uint2> core_type;
    typedef core_type::qgram_vector_type                   qgram_vector_type;
    typedef core_type::index_vector_type                   index_vector_type;
    typedef core_type::coord_vector_type                   coord_vector_type;
    typedef core_type::qgram_type                          qgram_type;
    typedef core_type::coord_type                          coord_type;
    typedef core_type::plain_view_type                     plain_view_type;
    typedef core_type::const_plain_view_type               const_plain_view_type;

    template <typename SystemTag>
    QGramSetIndexHost& operator=(const QGramIndexCore<SystemTag, uint64, uint32, uint2>& src) { this->copy_from(src); return *this; }
};

struct QGramSetIndexDevice : public QGramIndexCore<device_tag, uint64, uint32, uint2>
{
    typedef device_tag                                       system_tag;
    typedef QGramIndexCore<device_tag, uint64, uint32, uint2> core_type;
    typedef core_type::qgram_vector_type                     qgram_vector_type;
    typedef core_type::index_vector_type                     index_vector_type;
    typedef core_type::coord_vector_type                     coord_vector_type;
    typedef core_type::qgram_type                            qgram_type;
    typedef core_type::coord_type                            coord_type;
    typedef core_type::plain_view_type                       plain_view_type;
    typedef core_type::const_plain_view_type                 const_plain_view_type;

    /// index every position of every string at which a whole q-gram starts
    template <typename string_set_type>
    void build(const uint32 q, const uint32 symbol_sz, const string_set_type string_set, const uint32 qlut = 0)
    {
        build(q, symbol_sz, string_set, uniform_seeds_functor<>(q, 1u), qlut);
    }

    /// index the seeds of every string that `seeder` enumerates, by string and then in the seeder's order
    template <typename string_set_type, typename seed_functor>
    void build(const uint32 q, const uint32 symbol_sz, const string_set_type string_set, const seed_functor seeder, const uint32 qlut = 0)
    {
        qgram::set_parameters(q, symbol_sz, qlut, Q, symbol_size, QL, QLS);
        typedef nvbio::priv::packed_stream_where<typename string_set_type::symbol_iterator> where_type;
        typedef qgram::uniform_seeder<seed_functor> uniform;
        if (symbol_sz == 2u && qlut <= 16u && string_set.size() && uniform::ok && uniform::len(seeder) == q && uniform::interval(seeder) &&
            build_tuned(string_set, uniform::interval(seeder), std::integral_constant<bool, where_type::ok && where_type::BITS == 2u>())) return;
        coord_vector_type coords;
        enumerate_string_set_seeds(string_set, seeder, coords);
        qgram_vector_type keys(coords.size());
        thrust::transform(thrust::device, coords.begin(), coords.end(), keys.begin(), string_set_qgram_functor<string_set_type>(q, symbol_sz, string_set));
        qgram::build_generic(*this, keys, coords);
    }

    template <typename SystemTag>
    QGramSetIndexDevice& operator=(const QGramIndexCore<SystemTag, uint64, uint32, uint2>& src) { this->copy_from(src); return *this; }

private:
    template <typename string_set_type> bool build_tuned(const string_set_type&, const uint32, std::false_type) { return false; }
    template <typename string_set_type> bool build_tuned(const string_set_type& string_set, const uint32 interval, std::true_type)
    {
        sufsort::packed_set<string_set_type> packed(string_set);
        const nvbio_hip_string_set* set = &packed.set;
        const uint32 n_strings = packed.n_strings, q = Q, ql = QL;
        uint64 n = 0u;
        {
            const uint64 cb = nvbio_hip_qgram_set_count_seeds_temp_bytes(n_strings);
            sufsort::scratch temp(cb);
            qgram::check(nvbio_hip_qgram_set_count_seeds(set, n_strings, q, interval, &n, temp.ptr, cb, nullptr), "nvbio_hip_qgram_set_count_seeds");
        }
        const uint64 tb = nvbio_hip_qgram_set_index_build_temp_bytes(n, n_strings);
        qgram::build_tuned(*this, n, tb,
            [=](uint64* qg, uint32* sl, uint32* ix, uint32* lu, uint32* nu, void* temp) {
                return nvbio_hip_qgram_set_index_build(set, n_strings, q, interval, ql, n, qg, sl, ix, ql ? lu : nullptr, nu, temp, tb, nullptr); });
        return true;
    }
};

} // namespace nvbio
