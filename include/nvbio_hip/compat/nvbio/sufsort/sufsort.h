// compat/nvbio/sufsort/sufsort.h -- the plain-string front door of the reference's suffix sorting module (nvbio/sufsort/sufsort.h):
//
//   BWTParams                                                   the construction parameters (kept for source compatibility; the sorter
//                                                               here works in device memory only and reads none of them)
//   cuda::find_primary(string_len, string)                      the row of suffix 0 among the string_len + 1 sorted suffixes
//   cuda::suffix_sort(string_len, string, output, params)       output[0] = string_len (the empty suffix), output[1 .. string_len] the
//                                                               suffixes in order: string_len + 1 entries (sufsort_inl.h:149-162)
//   cuda::bwt(string_len, string, output, params) -> primary    string_len symbols: T[SA[row] - 1] over the rows but the primary, the
//                                                               '$' removed and the symbols after it shifted back (sufsort_inl.h:239-265,
//                                                               sufsort_utils.h:358-366, :412); the primary counts the empty suffix's row
//
//   cuda::suffix_sort(string_set, handler, params)              the suffixes of every string of a device-side set, the empty ones
//                                                               included, sorted; handler.process(n_suffixes, d_suffixes, d_string_ids,
//                                                               d_cum_lengths) is called once, with device pointers (sufsort.h:207-233)
//   SetBWTHandler                                               the base of the string-set BWT handlers (sufsort_utils.h:57-81)
//   cuda::bwt<SYMBOL_SIZE,BIG_ENDIAN>(string_set, handler, params)
//                                                               the BWT of a device-side packed-concatenated set; handler.process(
//                                                               n_suffixes, h_bwt, n_dollars, h_dollar_pos, h_dollar_ids) is called once,
//                                                               with host arrays: one byte a row, 255 = '$', the '$' rows as absolute
//                                                               positions and their string ids as uint64 (what DollarExtractor::extract
//                                                               hands on, sufsort_priv.cu:453-527; the reference calls it once per batch)
//
// `string` is a device-side iterator over a 2-bit alphabet.  A PackedStream over a word pointer that starts on a word boundary goes to
// nvbio_hip_suffix_sort / nvbio_hip_bwt (include/nvbio_hip.h) in place; any other 2-bit iterator is packed into
// big-endian words first, then takes the same call.  An iterator over any other alphabet of up to 8 bits (an 8-bit PackedVector of
// proteins, plain bytes) is unpacked to one symbol per byte and goes to nvbio_hip_suffix_sort_bytes / nvbio_hip_bwt_bytes; wider symbols
// throw.  A string set is a ConcatenatedStringSet over a 2-bit
// PackedStream on a word pointer with device offsets; it goes to nvbio_hip_set_suffix_sort / nvbio_hip_set_bwt in place, at whatever
// symbol its stream starts.  blockwise_suffix_sort, large_bwt (sets that do not fit the device), the file handlers and 4-bit sets are
// not provided.  Needs a translation unit compiled by hipcc and linked with libnvbio_hip.
#pragma once
#include "../basic/types.h"
#include "../basic/packedstream.h"
#include "../basic/packed_view.h"
#include "../basic/vector.h"
#include "../strings/string_set.h"
#include "../../../../nvbio_hip.h"
#include <hip/hip_runtime.h>
#include <stdexcept>
#include <string>
#include <vector>

namespace nvbio {

/// BWT construction parameters (sufsort.h:92-107)
struct BWTParams
{
    BWTParams() :
        host_memory(8u * 1024u * 1024u * 1024llu),
        device_memory(2u * 1024u * 1024u * 1024llu),
        bucketing_bits(16u),
        radix_slice(4u),
        cpu_bucketing(0u) {}

    uint64 host_memory;
    uint64 device_memory;
    uint32 bucketing_bits;
    uint32 radix_slice;
    uint32 cpu_bucketing;
};

namespace sufsort {

inline void check(const int err, const char* what)
{
    if (err != 0) throw std::runtime_error(std::string("nvbio::cuda sufsort: ") + what + " failed with hipError " + std::to_string(err));
}

/// device scratch that lives for one call
struct scratch
{
    explicit scratch(const uint64 bytes) : ptr(nullptr) { check(hipMalloc(&ptr, bytes ? bytes : 1u), "hipMalloc"); }
    ~scratch() { if (ptr) (void)hipFree(ptr); }
    scratch(const scratch&) = delete;
    scratch& operator=(const scratch&) = delete;
    template <typename T> T* as() const { return reinterpret_cast<T*>(ptr); }
    void* ptr;
};

/// the position, in symbols from a word boundary, at which an iterator's first symbol lies when it is a PackedStream (0 otherwise):
/// lanes that each own 16 symbols aligned to it own whole words
template <typename It> struct word_phase { NVBIO_HOST_DEVICE static uint32 get(const It&) { return 0u; } };
template <typename I, typename S, uint32 B, bool E, typename X>
struct word_phase< PackedStream<I, S, B, E, X> > { NVBIO_HOST_DEVICE static uint32 get(const PackedStream<I, S, B, E, X>& s) { return uint32(uint64(s.index()) & 15u); } };

/// word w of the big-endian 2-bit packing of string[0 .. n)
template <typename string_type>
__global__ void pack_kernel(const uint64 n, const string_type string, const uint64 n_words, uint32* words)
{
    const uint64 w = uint64(blockIdx.x) * 256u + threadIdx.x;
    if (w >= n_words) return;
    uint32 out = 0u;
    for (uint32 q = 0; q < 16u; ++q)
    {
        const uint64 i = w * 16u + q;
        if (i < n) out |= (uint32(string[i]) & 3u) << (30u - 2u * q);
    }
    words[w] = out;
}

/// output[i] = symbol i of big-endian 2-bit words; lane t owns the symbols whose position from the output's word boundary is in
/// [16 t, 16 t + 16), so no two lanes write one word of a packed output
template <typename output_iterator>
__global__ void unpack_kernel(const uint64 n, const uint32* words, output_iterator output, const uint32 phase, const uint64 n_lanes)
{
    const uint64 t = uint64(blockIdx.x) * 256u + threadIdx.x;
    if (t >= n_lanes) return;
    for (uint32 q = 0; q < 16u; ++q)
    {
        const uint64 at = t * 16u + q;                   // from the word boundary
        if (at < phase) continue;
        const uint64 i = at - phase;
        if (i < n) output[i] = uint8((words[i >> 4] >> (30u - 2u * uint32(i & 15u))) & 3u);
    }
}

template <typename output_iterator>
__global__ void copy_kernel(const uint64 n, const uint32* in, output_iterator output)
{
    const uint64 i = uint64(blockIdx.x) * 256u + threadIdx.x;
    if (i < n) output[i] = in[i];
}

/// a 2-bit text as the C-ABI takes it: the caller's own words where the string is a word-aligned PackedStream over a word pointer,
/// else a packed copy
template <typename string_type>
struct packed_text
{
    typedef nvbio::priv::packed_stream_where<string_type> where_type;

    packed_text(const uint64 n, const string_type& string) : words(nullptr), big_endian(1u), copy(nullptr)
    {
        if (stream_traits<string_type>::SYMBOL_SIZE != 2u)
            throw std::runtime_error("nvbio::cuda sufsort: only 2-bit alphabets are supported");
        if (!in_place(n, string, std::integral_constant<bool, where_type::ok && where_type::BITS == 2u>()))
        {
            const uint64 n_words = (n + 15u) / 16u;
            copy = new scratch(n_words * 4u);
            hipLaunchKernelGGL((pack_kernel<string_type>), dim3(uint32((n_words + 255u) / 256u)), dim3(256), 0, 0, n, string, n_words, copy->template as<uint32>());
            check(hipGetLastError(), "pack_kernel");
            words = copy->template as<uint32>();
        }
    }
    ~packed_text() { delete copy; }
    packed_text(const packed_text&) = delete;
    packed_text& operator=(const packed_text&) = delete;

    bool in_place(const uint64, const string_type&, std::false_type) { return false; }
    bool in_place(const uint64, const string_type& string, std::true_type)
    {
        uint64 word0; uint32 first;
        where_type::where(string, word0, first);
        if (first != 0u) return false;
        words = reinterpret_cast<const uint32*>(uintptr_t(word0) * 4u);
        big_endian = where_type::BE ? 1u : 0u;
        return true;
    }

    const uint32* words;
    uint32        big_endian;
    scratch*      copy;
};

/// the caller's own memory when the output iterator walks plain 32-bit words, else NULL
template <typename It, bool OK = nvbio::priv::plain_iterator<It>::ok> struct plain_words { static uint32* get(It) { return nullptr; } };
template <typename It> struct plain_words<It, true>
{
    typedef nvbio::priv::plain_iterator<It> plain;
    static uint32* get(It it) { return sizeof(typename plain::value_type) == 4u ? reinterpret_cast<uint32*>(plain::get(it)) : nullptr; }
};

inline void check_length(const uint64 n)
{
    if (n == 0u || n > 0xFFFFFFFEull) throw std::runtime_error("nvbio::cuda sufsort: the string must hold between 1 and 2^32 - 2 symbols");
}

/// ---- alphabets other than 2-bit, up to 8 bits a symbol: the string as one symbol per byte, for the `_bytes` entries ----

template <typename string_type>
__global__ void to_bytes_kernel(const uint64 n, const string_type string, uint8* bytes)
{
    const uint64 i = uint64(blockIdx.x) * 256u + threadIdx.x;
    if (i < n) bytes[i] = uint8(string[i]);
}

/// how an output iterator shares words: a PackedStream holds `per` symbols a word and starts `phase` symbols into one; anything else
/// owns each element
template <typename It> struct output_words { static uint32 per(const It&) { return 1u; } static uint32 phase(const It&) { return 0u; } };
template <typename I, typename S, uint32 B, bool E, typename X>
struct output_words< PackedStream<I, S, B, E, X> >
{
    typedef PackedStream<I, S, B, E, X> stream;
    static uint32 per(const stream&) { return stream::SYMBOLS_PER_WORD; }
    static uint32 phase(const stream& s) { return uint32(uint64(s.index()) % stream::SYMBOLS_PER_WORD); }
};

/// output[i] = in[i]; lane t owns the symbols whose position from the output's word boundary is in [per t, per t + per), so no two
/// lanes write one word of a packed output
template <typename output_iterator>
__global__ void from_bytes_kernel(const uint64 n, const uint8* in, output_iterator output, const uint32 phase, const uint32 per, const uint64 n_lanes)
{
    const uint64 t = uint64(blockIdx.x) * 256u + threadIdx.x;
    if (t >= n_lanes) return;
    for (uint32 q = 0; q < per; ++q)
    {
        const uint64 at = t * per + q;
        if (at < phase) continue;
        const uint64 i = at - phase;
        if (i < n) output[i] = in[i];
    }
}

template <typename string_type>
struct byte_text
{
    static const uint32 SYMBOL_SIZE = stream_traits<string_type>::SYMBOL_SIZE;
    byte_text(const uint64 n, const string_type& string) : bytes(n)
    {
        if (SYMBOL_SIZE < 1u || SYMBOL_SIZE > 8u) throw std::runtime_error("nvbio::cuda sufsort: only alphabets of up to 8 bits a symbol are supported");
        hipLaunchKernelGGL((to_bytes_kernel<string_type>), dim3(uint32((n + 255u) / 256u)), dim3(256), 0, 0, n, string, bytes.template as<uint8>());
        check(hipGetLastError(), "to_bytes_kernel");
    }
    scratch bytes;
};

template <typename string_type, typename output_iterator>
void suffix_sort_bytes(const uint64 n, const string_type& string, output_iterator output)
{
    byte_text<string_type> text(n, string);
    const uint64 tb = nvbio_hip_suffix_sort_bytes_temp_bytes(n);
    scratch temp(tb);
    if (uint32* direct = plain_words<output_iterator>::get(output))
    {
        check(nvbio_hip_suffix_sort_bytes(text.bytes.template as<uint8>(), text.SYMBOL_SIZE, n, direct, temp.ptr, tb, nullptr), "nvbio_hip_suffix_sort_bytes");
        return;
    }
    scratch sa((n + 1u) * 4u);
    check(nvbio_hip_suffix_sort_bytes(text.bytes.template as<uint8>(), text.SYMBOL_SIZE, n, sa.as<uint32>(), temp.ptr, tb, nullptr), "nvbio_hip_suffix_sort_bytes");
    hipLaunchKernelGGL((copy_kernel<output_iterator>), dim3(uint32((n + 256u) / 256u)), dim3(256), 0, 0, n + 1u, sa.as<uint32>(), output);
    check(hipGetLastError(), "copy_kernel");
    check(hipDeviceSynchronize(), "hipDeviceSynchronize");
}

/// the BWT symbols into `output` (NULL: the primary alone); returns the primary
template <typename string_type, typename output_iterator>
uint32 bwt_bytes(const uint64 n, const string_type& string, output_iterator* output)
{
    byte_text<string_type> text(n, string);
    const uint64 tb = nvbio_hip_bwt_bytes_temp_bytes(n);
    scratch temp(tb);
    scratch out(n);
    uint32 primary = 0;
    check(nvbio_hip_bwt_bytes(text.bytes.template as<uint8>(), text.SYMBOL_SIZE, n, 0u, out.as<uint8>(), &primary, nullptr, nullptr, temp.ptr, tb, nullptr), "nvbio_hip_bwt_bytes");
    if (output)
    {
        const uint32 per = output_words<output_iterator>::per(*output), phase = output_words<output_iterator>::phase(*output);
        const uint64 n_lanes = (n + phase + per - 1u) / per;
        hipLaunchKernelGGL((from_bytes_kernel<output_iterator>), dim3(uint32((n_lanes + 255u) / 256u)), dim3(256), 0, 0, n, out.as<uint8>(), *output, phase, per, n_lanes);
        check(hipGetLastError(), "from_bytes_kernel");
        check(hipDeviceSynchronize(), "hipDeviceSynchronize");
    }
    return primary;
}

/// begin[s] = first + offsets[s] and length[s] of every string of a concatenated set, as the C-ABI takes them; ends[0 .. 1] = the
/// first and the last offset
template <typename offset_iterator>
__global__ void set_offsets_kernel(const uint32 n_strings, const offset_iterator offsets, const uint64 first, uint64* begin, uint32* length, uint64* ends)
{
    const uint32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_strings) return;
    const uint64 b = uint64(offsets[i]), e = uint64(offsets[i + 1u]);
    begin[i]  = first + b;
    length[i] = uint32(e - b);
    if (i == 0u) ends[0] = b;
    if (i + 1u == n_strings) ends[1] = e;
}

static __global__ void widen_kernel(const uint32 n, const uint32* in, uint64* out)
{
    const uint32 i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) out[i] = in[i];
}

/// a device-side ConcatenatedStringSet over a 2-bit PackedStream as the C-ABI's nvbio_hip_string_set, its strings' words in place
template <typename string_set_type>
struct packed_set
{
    typedef typename string_set_type::symbol_iterator                stream_type;
    typedef nvbio::priv::packed_stream_where<stream_type>            where_type;

    explicit packed_set(const string_set_type& string_set) : n_strings(string_set.size()), n_suffixes(0), arrays(nullptr)
    {
        init(string_set, std::integral_constant<bool, where_type::ok && where_type::BITS == 2u>());
    }
    ~packed_set() { delete arrays; }
    packed_set(const packed_set&) = delete;
    packed_set& operator=(const packed_set&) = delete;

    void init(const string_set_type&, std::false_type) { throw std::runtime_error("nvbio::cuda sufsort: only sets of 2-bit packed strings over 32-bit words are supported"); }
    void init(const string_set_type& string_set, std::true_type)
    {
        if (n_strings == 0u) throw std::runtime_error("nvbio::cuda sufsort: the set must hold at least one string");
        uint64 word0; uint32 first;
        where_type::where(string_set.base_string(), word0, first);
        // begin (8 N) | ends (16) | length (4 N)
        arrays = new scratch(uint64(n_strings) * 12u + 16u);
        uint64* begin  = arrays->template as<uint64>();
        uint64* ends   = begin + n_strings;
        uint32* length = reinterpret_cast<uint32*>(ends + 2);
        hipLaunchKernelGGL((set_offsets_kernel<typename string_set_type::offset_iterator>), dim3((n_strings + 255u) / 256u), dim3(256), 0, 0,
                           n_strings, string_set.offsets(), uint64(first), begin, length, ends);
        check(hipGetLastError(), "set_offsets_kernel");
        uint64 h_ends[2] = { 0u, 0u };
        check(hipMemcpy(h_ends, ends, 16u, hipMemcpyDeviceToHost), "hipMemcpy");
        n_suffixes = (h_ends[1] - h_ends[0]) + n_strings;
        if (n_suffixes > 0xFFFFFFFEull) throw std::runtime_error("nvbio::cuda sufsort: the set must hold at most 2^32 - 2 symbols and strings together");
        set.words      = reinterpret_cast<const uint32*>(uintptr_t(word0) * 4u);
        set.n_words    = (uint64(first) + h_ends[1] + 15u) / 16u;
        set.bits       = 2u;
        set.big_endian = where_type::BE ? 1u : 0u;
        set.begin      = begin;
        set.length     = length;
        set.fixed_length = 0u;
        set._pad       = 0u;
    }

    nvbio_hip_string_set set;
    uint32               n_strings;
    uint64               n_suffixes;
    scratch*             arrays;
};

} // namespace sufsort

/// base virtual interface used by all string-set BWT handlers (sufsort_utils.h:57-81)
struct SetBWTHandler
{
    virtual ~SetBWTHandler() {}

    /// process a batch of BWT symbols, packed
    virtual void process(
        const uint32  n_suffixes,
        const uint32  bits_per_symbol,
        const uint32* bwt,
        const uint32  n_dollars,
        const uint64* dollar_pos,
        const uint64* dollar_ids) {}

    /// process a batch of BWT symbols, one byte each
    virtual void process(
        const uint32  n_suffixes,
        const uint8*  bwt,
        const uint32  n_dollars,
        const uint64* dollar_pos,
        const uint64* dollar_ids) {}
};

namespace cuda {

/// Sort all the suffixes of a given string: string_len + 1 entries, the empty suffix first
template <typename string_type, typename output_iterator>
void suffix_sort(
    const typename stream_traits<string_type>::index_type   string_len,
    const string_type                                       string,
    output_iterator                                         output,
    BWTParams*                                              params)
{
    (void)params;
    const uint64 n = string_len;
    sufsort::check_length(n);
    if constexpr (stream_traits<string_type>::SYMBOL_SIZE != 2u) { sufsort::suffix_sort_bytes(n, string, output); return; }
    sufsort::packed_text<string_type> text(n, string);
    const uint64 tb = nvbio_hip_suffix_sort_temp_bytes(n);
    sufsort::scratch temp(tb);
    if (uint32* direct = sufsort::plain_words<output_iterator>::get(output))
    {
        sufsort::check(nvbio_hip_suffix_sort(text.words, 2u, text.big_endian, n, direct, temp.ptr, tb, nullptr), "nvbio_hip_suffix_sort");
        return;
    }
    sufsort::scratch sa((n + 1u) * 4u);
    sufsort::check(nvbio_hip_suffix_sort(text.words, 2u, text.big_endian, n, sa.as<uint32>(), temp.ptr, tb, nullptr), "nvbio_hip_suffix_sort");
    hipLaunchKernelGGL((sufsort::copy_kernel<output_iterator>), dim3(uint32((n + 256u) / 256u)), dim3(256), 0, 0, n + 1u, sa.as<uint32>(), output);
    sufsort::check(hipGetLastError(), "copy_kernel");
    sufsort::check(hipDeviceSynchronize(), "hipDeviceSynchronize");
}

/// Compute the bwt of a device-side string: string_len symbols, the '$' removed; returns the position of the primary suffix
template <typename string_type, typename output_iterator>
typename string_type::index_type bwt(
    const typename string_type::index_type  string_len,
    string_type                             string,
    output_iterator                         output,
    BWTParams*                              params)
{
    (void)params;
    const uint64 n = string_len;
    sufsort::check_length(n);
    if constexpr (stream_traits<string_type>::SYMBOL_SIZE != 2u) return typename string_type::index_type(sufsort::bwt_bytes(n, string, &output));
    sufsort::packed_text<string_type> text(n, string);
    const uint64 tb = nvbio_hip_bwt_temp_bytes(n);
    sufsort::scratch temp(tb);
    sufsort::scratch words(4u * ((n + 63u) / 64u) * 4u);
    uint32 primary = 0;
    sufsort::check(nvbio_hip_bwt(text.words, 2u, text.big_endian, n, 0u, words.as<uint32>(), &primary, nullptr, nullptr, temp.ptr, tb, nullptr), "nvbio_hip_bwt");
    const uint32 phase   = sufsort::word_phase<output_iterator>::get(output);
    const uint64 n_lanes = (n + phase + 15u) / 16u;
    hipLaunchKernelGGL((sufsort::unpack_kernel<output_iterator>), dim3(uint32((n_lanes + 255u) / 256u)), dim3(256), 0, 0, n, words.as<uint32>(), output, phase, n_lanes);
    sufsort::check(hipGetLastError(), "unpack_kernel");
    sufsort::check(hipDeviceSynchronize(), "hipDeviceSynchronize");
    return typename string_type::index_type(primary);
}

/// return the position of the primary suffix of a string
template <typename string_type>
typename string_type::index_type find_primary(
    const typename string_type::index_type  string_len,
    const string_type                       string)
{
    const uint64 n = string_len;
    sufsort::check_length(n);
    if constexpr (stream_traits<string_type>::SYMBOL_SIZE != 2u) return typename string_type::index_type(sufsort::bwt_bytes(n, string, (uint8**)nullptr));
    sufsort::packed_text<string_type> text(n, string);
    const uint64 tb = nvbio_hip_bwt_temp_bytes(n);
    sufsort::scratch temp(tb);
    sufsort::scratch words(4u * ((n + 63u) / 64u) * 4u);
    uint32 primary = 0;
    sufsort::check(nvbio_hip_bwt(text.words, 2u, text.big_endian, n, 0u, words.as<uint32>(), &primary, nullptr, nullptr, temp.ptr, tb, nullptr), "nvbio_hip_bwt");
    return typename string_type::index_type(primary);
}

/// Sort the suffixes of all the strings in the given string set; the handler is a SetSuffixOutputHandler (sufsort.h:207-233)
template <typename string_set_type, typename output_handler>
void suffix_sort(
    const string_set_type&   string_set,
          output_handler&    output,
    BWTParams*               params = NULL)
{
    (void)params;
    sufsort::packed_set<string_set_type> set(string_set);
    const uint64 n = set.n_suffixes;
    const uint64 tb = nvbio_hip_set_suffix_sort_temp_bytes(n, set.n_strings);
    sufsort::scratch temp(tb);
    sufsort::scratch out(n * 8u + uint64(set.n_strings) * 4u);           // suffixes | string ids | cumulative lengths
    uint32* d_suffixes = out.as<uint32>();
    sufsort::check(nvbio_hip_set_suffix_sort(&set.set, set.n_strings, n, d_suffixes, d_suffixes + n, d_suffixes + 2u * n, temp.ptr, tb, nullptr), "nvbio_hip_set_suffix_sort");
    output.process(uint32(n), d_suffixes, d_suffixes + n, d_suffixes + 2u * n);
}

/// Build the bwt of a device-side string set; the handler is a SetBWTHandler
template <uint32 SYMBOL_SIZE, bool BIG_ENDIAN, typename storage_type, typename output_handler>
void bwt(
    const ConcatenatedStringSet<
        PackedStream<storage_type,uint8,SYMBOL_SIZE,BIG_ENDIAN,uint64>,
        uint64*>                    string_set,
        output_handler&             output,
        BWTParams*                  params = NULL)
{
    typedef ConcatenatedStringSet<PackedStream<storage_type,uint8,SYMBOL_SIZE,BIG_ENDIAN,uint64>, uint64*> string_set_type;
    (void)params;
    if (SYMBOL_SIZE != 2u) throw std::runtime_error("nvbio::cuda sufsort: only 2-bit alphabets are supported");
    sufsort::packed_set<string_set_type> set(string_set);
    const uint64 n = set.n_suffixes;
    const uint32 N = set.n_strings;
    const uint64 tb = nvbio_hip_set_bwt_temp_bytes(n, N);
    sufsort::scratch temp(tb);
    // dollar rows and ids as 64-bit (16 N) | the same as the entry writes them (8 N) | bwt (n)
    sufsort::scratch out(uint64(N) * 24u + n);
    uint64* d_pos64 = out.as<uint64>();
    uint32* d_rows  = reinterpret_cast<uint32*>(d_pos64 + 2u * uint64(N));
    uint8*  d_bwt   = reinterpret_cast<uint8*>(d_rows + 2u * uint64(N));
    sufsort::check(nvbio_hip_set_bwt(&set.set, N, n, d_bwt, d_rows, d_rows + N, nullptr, temp.ptr, tb, nullptr), "nvbio_hip_set_bwt");
    hipLaunchKernelGGL(sufsort::widen_kernel, dim3((2u * N + 255u) / 256u), dim3(256), 0, 0, 2u * N, d_rows, d_pos64);
    sufsort::check(hipGetLastError(), "widen_kernel");
    std::vector<uint8>  h_bwt(n);
    std::vector<uint64> h_dollars(2u * uint64(N));
    sufsort::check(hipMemcpy(h_bwt.data(), d_bwt, n, hipMemcpyDeviceToHost), "hipMemcpy");
    sufsort::check(hipMemcpy(h_dollars.data(), d_pos64, uint64(N) * 16u, hipMemcpyDeviceToHost), "hipMemcpy");
    output.process(uint32(n), h_bwt.data(), N, h_dollars.data(), h_dollars.data() + N);
}

} // namespace cuda
} // namespace nvbio
