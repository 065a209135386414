// compat/nvbio/basic/packed_vector.h -- PackedVector<system_tag, SYMBOL_SIZE, BIG_ENDIAN, IndexType> (nvbio/basic/packed_vector.h): a
// vector of 32-bit words in the memory the tag names, seen through a PackedStream of SYMBOL_SIZE-bit symbols.  The device flavour's
// stream runs over a thrust::device_ptr, so host code can read and write single symbols of it (one small copy each, as with the
// reference's) and device code can take the same iterator; a vector copies across memory spaces by construction.  A word holds
// floor(32 / SYMBOL_SIZE) symbols, as PackedStream lays them out.  Needs a translation unit compiled by hipcc.
#pragma once
#include "types.h"
#include "packedstream.h"
#include "vector.h"

namespace nvbio {

template <typename SystemTag, uint32 SYMBOL_SIZE_T, bool BIG_ENDIAN_T = false, typename IndexType = uint32>
struct PackedVector
{
    static const uint32 SYMBOL_SIZE      = SYMBOL_SIZE_T;
    static const uint32 BIG_ENDIAN       = BIG_ENDIAN_T;
    static const uint32 SYMBOLS_PER_WORD = 32u / SYMBOL_SIZE_T;

    typedef SystemTag                                                         system_tag;
    typedef IndexType                                                         index_type;
    typedef nvbio::vector<system_tag, uint32>                                 vector_type;
    typedef typename vector_type::base_type::pointer                          pointer;
    typedef typename vector_type::base_type::const_pointer                    const_pointer;
    typedef PackedStream<pointer, uint8, SYMBOL_SIZE_T, BIG_ENDIAN_T, IndexType>        stream_type;
    typedef PackedStream<const_pointer, uint8, SYMBOL_SIZE_T, BIG_ENDIAN_T, IndexType>  const_stream_type;
    typedef stream_type                                                       iterator;
    typedef const_stream_type                                                 const_iterator;
    typedef uint8                                                             value_type;
    typedef stream_type                                                       plain_view_type;
    typedef const_stream_type                                                 const_plain_view_type;

    PackedVector(const index_type size = 0) : m_size(0) { resize(size); }
    template <typename other_tag>
    PackedVector(const PackedVector<other_tag, SYMBOL_SIZE_T, BIG_ENDIAN_T, IndexType>& other) : m_storage(other.m_storage), m_size(other.m_size) {}
    template <typename other_tag>
    PackedVector& operator=(const PackedVector<other_tag, SYMBOL_SIZE_T, BIG_ENDIAN_T, IndexType>& other) { m_storage = other.m_storage; m_size = other.m_size; return *this; }

    /// words that hold `size` symbols
    static uint64 words_for(const uint64 size) { return (size + SYMBOLS_PER_WORD - 1u) / SYMBOLS_PER_WORD; }

    void resize(const index_type size) { m_size = size; m_storage.resize(words_for(size), 0u); }
    void clear() { resize(0); }
    index_type size() const { return m_size; }

    iterator       begin()       { return iterator(m_storage.data(), 0); }
    const_iterator begin() const { return const_iterator(m_storage.data(), 0); }
    iterator       end()         { return begin() + m_size; }
    const_iterator end() const   { return begin() + m_size; }

    uint8 operator[](const index_type i) const { return begin()[i]; }
    typename stream_type::reference operator[](const index_type i) { return begin()[i]; }

    /// the words themselves
    uint32*       words()       { return m_storage.empty() ? (uint32*)0 : thrust::raw_pointer_cast(m_storage.data()); }
    const uint32* words() const { return m_storage.empty() ? (const uint32*)0 : thrust::raw_pointer_cast(m_storage.data()); }

    vector_type m_storage;
    index_type  m_size;
};

template <typename T, uint32 S, bool E, typename X> inline typename PackedVector<T, S, E, X>::plain_view_type       plain_view(PackedVector<T, S, E, X>& v)       { return v.begin(); }
template <typename T, uint32 S, bool E, typename X> inline typename PackedVector<T, S, E, X>::const_plain_view_type plain_view(const PackedVector<T, S, E, X>& v) { return v.begin(); }

} // namespace nvbio
