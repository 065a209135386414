// compat/nvbio/strings/wavelet_tree.h -- the reference's wavelet tree (nvbio/strings/wavelet_tree.h): WaveletTree, the shallow view
// (bit stream, node splits, occurrence counts -- the layout of include/nvbio_hip.h, "Byte alphabets", bit for bit), WaveletTreeStorage,
// which owns the three arrays in host or device memory, setup(), text(), both rank() overloads and plain_view().  A WaveletTree is a
// rank dictionary and its own text, so fm_index<WaveletTree<..>, ..> of fmindex/fmindex.h searches over it.
//
// The walks are generic NVBIO_HOST_DEVICE code over any iterators (positions carried as counts, the clamp of a position
// to its level's end, 0 at an empty node).  setup() unpacks the string to one symbol per byte -- in place when it already is plain
// bytes -- and calls nvbio_hip_wavelet_setup for a device tree, nvbio_hip_wavelet_setup_host for a host tree.  Symbols wider than 8
// bits throw.  Needs a translation unit compiled by hipcc and linked with libnvbio_hip.
#pragma once
#include "../basic/types.h"
#include "../basic/numbers.h"
#include "../basic/packedstream.h"
#include "../basic/packed_vector.h"
#include "../basic/vector.h"
#include "../basic/primitives.h"
#include "../../../../nvbio_hip.h"
#include <hip/hip_runtime.h>
#include <stdexcept>
#include <string>
#include <vector>

namespace nvbio {

template <typename BitStreamIterator, typename IndexIterator, typename SymbolType = uint8>
struct WaveletTree
{
    typedef typename stream_traits<BitStreamIterator>::index_type   index_type;
    typedef SymbolType                                              symbol_type;
    typedef SymbolType                                              value_type;
    typedef BitStreamIterator                                       bit_iterator;
    typedef IndexIterator                                           index_iterator;
    typedef WaveletTree<BitStreamIterator, IndexIterator>           text_type;      // the tree is its own text
    typedef typename nvbio::vector_type<index_type, 2>::type        range_type;
    typedef null_type                                               vector_type;

    NVBIO_HOST_DEVICE WaveletTree(const uint32 _symbol_size = 0, const index_type _size = 0, const BitStreamIterator _bits = BitStreamIterator(),
                                  const IndexIterator _nodes = IndexIterator(), const IndexIterator _occ = IndexIterator())
        : m_symbol_size(_symbol_size), m_size(_size), m_bits(_bits), m_nodes(_nodes), m_occ(_occ) {}

    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE void resize(const uint32 _size, const uint32 _symbol_size) { m_size = _size; m_symbol_size = _symbol_size; }
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE uint32 symbol_count() const { return 1u << m_symbol_size; }
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE uint32 symbol_size()  const { return m_symbol_size; }
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE index_type size()     const { return m_size; }
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE BitStreamIterator bits() const { return m_bits; }
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE IndexIterator splits()   const { return m_nodes; }
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE IndexIterator occ()      const { return m_occ; }

    /// the bits equal to b in [0, r] of the node `node` of level l, whose first bit lies node_begin bits into its level; the last bit
    /// looked at is clamped to the level's end
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE index_type rank(const uint32 l, const uint32 node, const index_type node_begin, const index_type r, const uint8 b) const
    {
        const index_type first = index_type(l) * m_size + node_begin;
        index_type last = first + r;
        const index_type level_last = index_type(l + 1u) * m_size - 1u;
        if (last > level_last) last = level_last;
        const index_type w = last >> 5;
        const uint32 keep = uint32(last & 31u) + 1u;                       // leading bits of word w that belong to the prefix
        const uint32 word = uint32(m_bits.stream()[w]);
        const index_type ones = index_type(m_occ[symbol_count() + w]) + index_type(__builtin_popcount(word >> (32u - keep))) - index_type(m_occ[node]);
        return b ? ones : (last + 1u - first) - ones;
    }

    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE SymbolType operator[](const index_type i) const;
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE SymbolType operator()(const index_type i) const { return this->operator[](i); }

    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE       text_type& text()       { return *this; }
    NVBIO_FORCEINLINE NVBIO_HOST_DEVICE const text_type& text() const { return *this; }

    uint32              m_symbol_size;
    index_type          m_size;
    BitStreamIterator   m_bits;
    IndexIterator       m_nodes;
    IndexIterator       m_occ;
};

/// the symbol at position i
template <typename BitStreamIterator, typename IndexIterator, typename IndexType, typename SymbolType>
NVBIO_FORCEINLINE NVBIO_HOST_DEVICE SymbolType text(const WaveletTree<BitStreamIterator, IndexIterator, SymbolType>& tree, const IndexType i)
{
    const uint32 S = tree.symbol_size();
    uint32 node = 0u, c = 0u;
    IndexType begin = 0u, at = i;                                          // `at`: the symbol's place inside its node
    for (uint32 l = 0; l < S; ++l)
    {
        const uint32 b = tree.bits()[at + begin + IndexType(tree.size()) * l];
        c = (c << 1) | b;
        if (at) at = tree.rank(l, node, begin, at - 1u, uint8(b));        // the equal bits before it
        if (b) begin = tree.splits()[node];
        node = 2u * node + 1u + b;
    }
    return SymbolType(c);
}

/// the occurrences of c in [0, i]
template <typename BitStreamIterator, typename IndexIterator, typename SymbolType>
NVBIO_FORCEINLINE NVBIO_HOST_DEVICE typename WaveletTree<BitStreamIterator, IndexIterator, SymbolType>::index_type
rank(const WaveletTree<BitStreamIterator, IndexIterator, SymbolType>& tree, const typename WaveletTree<BitStreamIterator, IndexIterator, SymbolType>::index_type i, const uint32 c)
{
    typedef typename WaveletTree<BitStreamIterator, IndexIterator, SymbolType>::index_type index_type;
    const uint32 S = tree.symbol_size();
    uint32 node = 0u;
    index_type begin = 0u, end = tree.size(), count = i + 1u;              // the node's symbols are [begin, end) of the sorted text
    for (uint32 l = 0; l < S; ++l)
    {
        if (begin == end) return 0u;                                       // an empty node
        const uint32 b = (c >> (S - 1u - l)) & 1u;
        if (count) count = tree.rank(l, node, begin, count - 1u, uint8(b));
        const index_type middle = tree.splits()[node];
        if (b) begin = middle; else end = middle;
        node = 2u * node + 1u + b;
    }
    return count;
}

/// ... at both ends of a range
template <typename BitStreamIterator, typename IndexIterator, typename SymbolType>
NVBIO_FORCEINLINE NVBIO_HOST_DEVICE typename WaveletTree<BitStreamIterator, IndexIterator, SymbolType>::range_type
rank(const WaveletTree<BitStreamIterator, IndexIterator, SymbolType>& tree, const typename WaveletTree<BitStreamIterator, IndexIterator, SymbolType>::range_type range, const uint32 c)
{
    return make_vector(rank(tree, range.x, c), rank(tree, range.y, c));
}

template <typename BitStreamIterator, typename IndexIterator, typename SymbolType>
NVBIO_FORCEINLINE NVBIO_HOST_DEVICE SymbolType WaveletTree<BitStreamIterator, IndexIterator, SymbolType>::operator[](const index_type i) const { return nvbio::text(*this, i); }

template <typename SystemTag, typename IndexType = uint32, typename SymbolType = uint8>
struct WaveletTreeStorage
{
    typedef SystemTag                                           system_tag;
    typedef IndexType                                           index_type;
    typedef SymbolType                                          symbol_type;
    typedef PackedVector<system_tag, 1u, true, index_type>      bit_vector_type;
    typedef nvbio::vector<system_tag, index_type>               index_vector_type;
    typedef typename bit_vector_type::iterator                  bit_iterator;
    typedef typename bit_vector_type::const_iterator            const_bit_iterator;
    typedef typename index_vector_type::iterator                index_iterator;
    typedef typename index_vector_type::const_iterator          const_index_iterator;
    typedef WaveletTree<bit_iterator, index_iterator>                   plain_view_type;
    typedef WaveletTree<const_bit_iterator, const_index_iterator>       const_plain_view_type;

    WaveletTreeStorage() : m_symbol_size(0u), m_size(0u) {}

    void resize(const uint32 _size, const uint32 _symbol_size)
    {
        m_size = _size; m_symbol_size = _symbol_size;
        const uint32 n_symbols = 1u << _symbol_size;
        m_bits.resize(m_size * m_symbol_size);
        m_nodes.resize(n_symbols);
        m_occ.resize(n_symbols + util::divide_ri(m_size * m_symbol_size, 32u));
    }
    uint32     symbol_size() const { return m_symbol_size; }
    index_type size() const { return m_size; }

    bit_iterator         bits()         { return m_bits.begin(); }
    index_iterator       splits()       { return m_nodes.begin(); }
    index_iterator       occ()          { return m_occ.begin(); }
    const_bit_iterator   bits() const   { return m_bits.begin(); }
    const_index_iterator splits() const { return m_nodes.begin(); }
    const_index_iterator occ() const    { return m_occ.begin(); }

    operator plain_view_type()             { return plain_view_type(m_symbol_size, m_size, bits(), splits(), occ()); }
    operator const_plain_view_type() const { return const_plain_view_type(m_symbol_size, m_size, bits(), splits(), occ()); }

    uint32              m_symbol_size;
    index_type          m_size;
    bit_vector_type     m_bits;
    index_vector_type   m_nodes;
    index_vector_type   m_occ;
};

template <typename T, typename I, typename S> typename WaveletTreeStorage<T, I, S>::plain_view_type       plain_view(WaveletTreeStorage<T, I, S>& tree)       { return tree; }
template <typename T, typename I, typename S> typename WaveletTreeStorage<T, I, S>::const_plain_view_type plain_view(const WaveletTreeStorage<T, I, S>& tree) { return tree; }

namespace wavelet {

inline void check(const int err, const char* what)
{
    if (err != 0) throw std::runtime_error(std::string("nvbio wavelet tree: ") + what + " failed with hipError " + std::to_string(err));
}

template <typename string_iterator>
__global__ void unpack_kernel(const uint64 n, const string_iterator string, uint8* bytes)
{
    const uint64 i = uint64(blockIdx.x) * 256u + threadIdx.x;
    if (i < n) bytes[i] = uint8(string[i]);
}

struct device_bytes
{
    explicit device_bytes(const uint64 n) : ptr(nullptr) { check(hipMalloc(&ptr, n ? n : 1u), "hipMalloc"); }
    ~device_bytes() { if (ptr) (void)hipFree(ptr); }
    device_bytes(const device_bytes&) = delete;
    device_bytes& operator=(const device_bytes&) = delete;
    void* ptr;
};

/// what the last setup() of this thread did with its string: "bytes" (plain device bytes, read in place) or "unpacked"
inline const char*& last_path() { static thread_local const char* p = ""; return p; }

template <typename string_iterator, typename index_type, typename symbol_type>
void setup(const uint64 n, const uint32 S, const string_iterator& string, WaveletTreeStorage<device_tag, index_type, symbol_type>& tree)
{
    typedef nvbio::priv::plain_iterator<string_iterator> plain;
    const uint8* symbols = nullptr;
    device_bytes* copy = nullptr;
    if (plain::ok && sizeof(typename std::iterator_traits<string_iterator>::value_type) == 1u)
    {
        symbols = reinterpret_cast<const uint8*>(plain::get(string));
        last_path() = "bytes";
    }
    else
    {
        copy = new device_bytes(n);
        hipLaunchKernelGGL((unpack_kernel<string_iterator>), dim3(uint32((n + 255u) / 256u)), dim3(256), 0, 0, n, string, reinterpret_cast<uint8*>(copy->ptr));
        symbols = reinterpret_cast<const uint8*>(copy->ptr);
        last_path() = "unpacked";
    }
    const uint64 tb = nvbio_hip_wavelet_setup_temp_bytes(n, S);
    device_bytes temp(tb);
    const int err = nvbio_hip_wavelet_setup(symbols, S, n, reinterpret_cast<uint32*>(tree.m_bits.words()), reinterpret_cast<uint32*>(raw_pointer(tree.m_nodes)),
                                            reinterpret_cast<uint32*>(raw_pointer(tree.m_occ)), temp.ptr, tb, nullptr);
    const int done = hipDeviceSynchronize();
    delete copy;
    check(err, "nvbio_hip_wavelet_setup");
    check(done, "hipDeviceSynchronize");
}

template <typename string_iterator, typename index_type, typename symbol_type>
void setup(const uint64 n, const uint32 S, const string_iterator& string, WaveletTreeStorage<host_tag, index_type, symbol_type>& tree)
{
    std::vector<uint8> bytes(n);
    for (uint64 i = 0; i < n; ++i) bytes[i] = uint8(string[i]);
    last_path() = "host";
    check(nvbio_hip_wavelet_setup_host(bytes.data(), S, n, reinterpret_cast<uint32*>(tree.m_bits.words()), reinterpret_cast<uint32*>(raw_pointer(tree.m_nodes)),
                                       reinterpret_cast<uint32*>(raw_pointer(tree.m_occ)), 0), "nvbio_hip_wavelet_setup_host");
}

} // namespace wavelet

/// build the wavelet tree of string[0 .. string_len): stream_traits<string_iterator>::SYMBOL_SIZE bits a symbol
template <typename system_tag, typename string_iterator, typename index_type, typename symbol_type>
void setup(const index_type string_len, const string_iterator& string, WaveletTreeStorage<system_tag, index_type, symbol_type>& out_tree)
{
    const uint32 S = stream_traits<string_iterator>::SYMBOL_SIZE;
    if (S < 1u || S > 8u || sizeof(index_type) != 4u) throw std::runtime_error("nvbio wavelet tree: only symbols of 1 to 8 bits and 32-bit indices are supported");
    if (string_len == 0u || uint64(string_len) * S > 0xFFFFFFFFull) throw std::runtime_error("nvbio wavelet tree: the string must hold between 1 and (2^32 - 1) / SYMBOL_SIZE symbols");
    out_tree.resize(string_len, S);
    wavelet::setup(uint64(string_len), S, string, out_tree);
}

} // namespace nvbio
