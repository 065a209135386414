// tests/compat/wavelet_callers.hip -- callers of the wavelet tree written in the reference's vocabulary (nvbio/strings/wavelet_tree.h as
// nvbio-test/wavelet_test.cu and examples/waveletfm/waveletfm.cu use it): setup() of a WaveletTreeStorage from plain device bytes, from
// a 5-bit device PackedVector and from a host PackedVector, text() and rank() as thrust functors on the device and in host loops,
// cuda::bwt / cuda::suffix_sort / cuda::find_primary of an 8-bit PackedVector, and fm_index<WaveletTree, ..>::match over the tree of
// a BWT.  It includes the reference's header names and is compiled with `hipcc -I include/nvbio_hip/compat`.  The extern "C" entry
// points take and return host memory so that the Python tests can drive it.
#include <nvbio/basic/types.h>
#include <nvbio/basic/vector.h>
#include <nvbio/basic/primitives.h>
#include <nvbio/basic/packed_vector.h>
#include <nvbio/strings/alphabet.h>
#include <nvbio/strings/wavelet_tree.h>
#include <nvbio/sufsort/sufsort.h>
#include <nvbio/fmindex/fmindex.h>
#include <thrust/device_vector.h>
#include <thrust/iterator/counting_iterator.h>
#include <thrust/copy.h>
#include <stdio.h>
#include <string.h>
#include <exception>

using namespace nvbio;

#define API extern "C" __attribute__((visibility("default")))

template <typename tree_type>
struct text_of
{
    typedef uint32 argument_type;
    typedef uint8  result_type;
    NVBIO_HOST_DEVICE text_of(const tree_type t) : tree(t) {}
    NVBIO_HOST_DEVICE uint8 operator()(const uint32 i) const { return text(tree, i); }
    tree_type tree;
};
template <typename tree_type>
struct rank_of
{
    NVBIO_HOST_DEVICE rank_of(const tree_type t, const uint32* p, const uint8* c) : tree(t), positions(p), symbols(c) {}
    NVBIO_HOST_DEVICE uint32 operator()(const uint32 k) const { return rank(tree, positions[k], uint32(symbols[k])); }
    tree_type tree; const uint32* positions; const uint8* symbols;
};

template <typename storage_type>
static void arrays_out(const storage_type& tree, uint32* out_bits, uint32* out_splits, uint32* out_occ)
{
    thrust::copy(tree.m_bits.m_storage.begin(), tree.m_bits.m_storage.end(), out_bits);
    thrust::copy(tree.m_nodes.begin(), tree.m_nodes.end(), out_splits);
    thrust::copy(tree.m_occ.begin(), tree.m_occ.end(), out_occ);
}

/// text and ranks of a device tree, computed on the device through the generic walks
template <typename storage_type>
static void device_queries(const storage_type& tree, const uint32 n, const uint32* h_positions, const uint8* h_symbols, const uint32 nq, uint8* out_text, uint32* out_rank)
{
    typedef typename storage_type::const_plain_view_type view_type;
    const view_type view = plain_view(tree);
    nvbio::vector<device_tag, uint8> d_text(n);
    nvbio::transform<device_tag>(n, thrust::make_counting_iterator<uint32>(0), d_text.begin(), text_of<view_type>(view));
    thrust::copy(d_text.begin(), d_text.end(), out_text);
    thrust::device_vector<uint32> d_pos(h_positions, h_positions + nq), d_rank(nq);
    thrust::device_vector<uint8>  d_sym(h_symbols, h_symbols + nq);
    nvbio::transform<device_tag>(nq, thrust::make_counting_iterator<uint32>(0), d_rank.begin(),
                                 rank_of<view_type>(view, thrust::raw_pointer_cast(d_pos.data()), thrust::raw_pointer_cast(d_sym.data())));
    thrust::copy(d_rank.begin(), d_rank.end(), out_rank);
}

// ---- plain device bytes (8 bits a symbol): setup reads them in place
API int compat_wavelet_bytes(const uint8* h_text, uint32 n, const uint32* h_positions, const uint8* h_symbols, uint32 nq,
                             uint32* out_bits, uint32* out_splits, uint32* out_occ, uint8* out_text, uint32* out_rank, char* out_path)
{
    try {
        nvbio::vector<host_tag, uint8>   h(n);
        for (uint32 i = 0; i < n; ++i) h[i] = h_text[i];
        nvbio::vector<device_tag, uint8> d_text(h);
        WaveletTreeStorage<device_tag> tree;
        setup(n, d_text.begin(), tree);
        strcpy(out_path, wavelet::last_path());
        arrays_out(tree, out_bits, out_splits, out_occ);
        device_queries(tree, n, h_positions, h_symbols, nq, out_text, out_rank);
        return 0;
    } catch (const std::exception& e) { fprintf(stderr, "compat_wavelet_bytes: %s\n", e.what()); return -1; }
}

// ---- a 5-bit PackedVector: the device tree (unpacked first) and a host-tag tree of the same text, queried in host loops
API int compat_wavelet_packed5(const uint8* h_symbols_in, uint32 n, const uint32* h_positions, const uint8* h_symbols, uint32 nq,
                               uint32* out_bits, uint32* out_splits, uint32* out_occ, uint8* out_text, uint32* out_rank, char* out_path,
                               uint32* host_bits, uint32* host_splits, uint32* host_occ, uint8* host_text, uint32* host_rank, uint32* host_range)
{
    try {
        PackedVector<host_tag, 5, true> h_text(n);
        for (uint32 i = 0; i < n; ++i) h_text[i] = h_symbols_in[i];
        PackedVector<device_tag, 5, true> d_text(h_text);
        WaveletTreeStorage<device_tag> tree;
        setup(n, d_text.begin(), tree);
        strcpy(out_path, wavelet::last_path());
        arrays_out(tree, out_bits, out_splits, out_occ);
        device_queries(tree, n, h_positions, h_symbols, nq, out_text, out_rank);

        WaveletTreeStorage<host_tag> h_tree;
        setup(n, h_text.begin(), h_tree);
        arrays_out(h_tree, host_bits, host_splits, host_occ);
        const WaveletTreeStorage<host_tag>::const_plain_view_type view = plain_view((const WaveletTreeStorage<host_tag>&)h_tree);
        for (uint32 i = 0; i < n; ++i) host_text[i] = view[i];
        for (uint32 k = 0; k < nq; ++k) host_rank[k] = rank(view, h_positions[k], uint32(h_symbols[k]));
        for (uint32 k = 0; k + 1u < nq; k += 2u)
        {
            const uint2 r = rank(view, make_uint2(h_positions[k], h_positions[k + 1u]), uint32(h_symbols[k]));
            host_range[k] = r.x; host_range[k + 1u] = r.y;
        }
        return 0;
    } catch (const std::exception& e) { fprintf(stderr, "compat_wavelet_packed5: %s\n", e.what()); return -1; }
}

// ---- an 8-bit PackedVector through the plain-string sorter: suffix array, BWT symbols and both primaries
API int compat_wavelet_bwt8(const uint8* h_symbols_in, uint32 n, uint32* out_sa, uint8* out_bwt, uint32* out_primary, uint32* out_found_primary)
{
    try {
        PackedVector<host_tag, 8, true> h_text(n);
        for (uint32 i = 0; i < n; ++i) h_text[i] = h_symbols_in[i];
        PackedVector<device_tag, 8, true> d_text(h_text);
        PackedVector<device_tag, 8, true> d_bwt(n + 1u);
        thrust::device_vector<uint32> d_sa(n + 1u);
        BWTParams params;
        cuda::suffix_sort(n, d_text.begin(), d_sa.begin(), &params);
        thrust::copy(d_sa.begin(), d_sa.end(), out_sa);
        *out_primary = cuda::bwt(n, d_text.begin(), d_bwt.begin(), &params);
        *out_found_primary = cuda::find_primary(n, d_text.begin());
        PackedVector<host_tag, 8, true> h_bwt(d_bwt);
        for (uint32 i = 0; i < n; ++i) out_bwt[i] = h_bwt[i];
        return 0;
    } catch (const std::exception& e) { fprintf(stderr, "compat_wavelet_bwt8: %s\n", e.what()); return -1; }
}

// ---- what examples/waveletfm does: the BWT of a protein string, its wavelet tree, L2 by host-side ranks, fm_index match of every suffix
API int compat_wavelet_fm(const char* proteins, uint32 n, char* out_bwt_string, uint32* out_primary, uint32* out_ranges)
{
    try {
        const uint32 bits = AlphabetTraits<PROTEIN>::SYMBOL_SIZE;
        PackedVector<host_tag, bits, true> h_text(n);
        from_string<PROTEIN>(proteins, proteins + n, h_text.begin());
        PackedVector<device_tag, bits, true> d_text(h_text);
        PackedVector<device_tag, bits, true> d_bwt(n + 1u);
        BWTParams params;
        const uint32 primary = cuda::bwt(n, d_text.begin(), d_bwt.begin(), &params);
        *out_primary = primary;
        to_string<PROTEIN>(d_bwt.begin(), d_bwt.begin() + n, out_bwt_string);

        typedef WaveletTreeStorage<device_tag>                         tree_type;
        typedef tree_type::const_plain_view_type                       view_type;
        typedef nvbio::vector<device_tag, uint32>::const_iterator      l2_iterator;
        typedef fm_index<view_type, null_type, l2_iterator>            fm_index_type;
        tree_type tree;
        setup(n, d_bwt.begin(), tree);
        const view_type view = plain_view((const tree_type&)tree);
        const uint32 K = 1u << bits;
        nvbio::vector<device_tag, uint32> L2(K + 1u);
        L2[0] = 0;
        for (uint32 i = 1; i <= K; ++i) L2[i] = L2[i - 1] + rank(view, n, i - 1u);
        const fm_index_type fmi(n, primary, L2.begin(), view, null_type());
        for (uint32 i = 0; i < n; ++i)
        {
            const uint2 range = match(fmi, d_text.begin() + i, n - i);
            out_ranges[2 * i] = range.x; out_ranges[2 * i + 1] = range.y;
        }
        return 0;
    } catch (const std::exception& e) { fprintf(stderr, "compat_wavelet_fm: %s\n", e.what()); return -1; }
}
