// include/nvbio_hip/sufsort.h -- the C++ host layer of the suffix sorter and BWT builder (nvbio/sufsort/sufsort.h for one plain string):
// thin callers of nvbio_hip_suffix_sort / nvbio_hip_bwt (include/nvbio_hip.h) over the project's device vectors.
// No HIP headers are needed to include it.
//
//   PackedTextView<BIG_ENDIAN>   a 2-bit packed text in device memory: words + length
//   suffix_sort(text, sa)        sa: n + 1 rows, sa[0] = n, a suffix that is a proper prefix of another first
//   bwt(text, sa_int, out)       the BWT with the '$' row dropped (big-endian words, what nvbio_hip_build_bwt_occ takes), the primary,
//                                and on request the sampled and the whole suffix array
//   suffix_sort_bytes / bwt_bytes  the same for a byte text of 1 to 8 bits a symbol (nvbio_hip_suffix_sort_bytes / nvbio_hip_bwt_bytes)
//
// and of the same module's string-set front door, thin callers of nvbio_hip_set_suffix_sort / nvbio_hip_set_bwt:
//
//   set_slot_count(set)                      the set's slots: its symbols + its strings (every string has an empty suffix too)
//   set_suffix_sort(set, n_suffixes, out)    the global suffix indices in sorted order, the string of every index, the cumulative lengths
//   set_bwt(set, n_suffixes, out)            one byte a row, 255 = '$', the '$' rows and their strings, on request the (position, string) pairs
#pragma once
#include "types.h"
#include "strings.h"

namespace nvbio {
namespace hip {

/// a 2-bit packed text in device memory (PackedStream order: big- or little-endian words), `length` symbols in ceil(length / 16) words
template <bool BIG_ENDIAN_T>
struct PackedTextView
{
    static const bool big_endian = BIG_ENDIAN_T;
    PackedTextView() : words(nullptr), length(0) {}
    PackedTextView(const uint32* w, const uint64 n) : words(w), length(n) {}
    const uint32* words;
    uint64        length;
};

/// what bwt() returns beside the words
struct BWTResult
{
    BWTResult() : primary(0) {}
    uint32                 primary;        ///< the row whose suffix is 0
    device_vector<uint32>  bwt_words;      ///< 4 * ceil(n / 64) big-endian 2-bit words, zero padded
    device_vector<uint32>  ssa;            ///< ceil((n + 1) / sa_int) samples, ssa[0] = 0xFFFFFFFF (empty unless asked for)
    device_vector<uint32>  sa;             ///< n + 1 rows (empty unless asked for)
};

/// the suffix array of `text` into `sa` (resized to n + 1).  `temp` is the call's scratch, kept by the caller between calls.
/// The call waits for the stream once per sorting round and has finished when it returns.
template <bool BE>
inline void suffix_sort(const PackedTextView<BE>& text, device_vector<uint32>& sa, device_vector<uint8>& temp, void* stream = nullptr)
{
    const uint64 tb = nvbio_hip_suffix_sort_temp_bytes(text.length);
    if (temp.size() < tb) temp.resize(tb);
    sa.resize(text.length + 1u);
    hip_check(nvbio_hip_suffix_sort(text.words, 2u, BE ? 1u : 0u, text.length, sa.data(), temp.data(), temp.size(), stream), "nvbio_hip_suffix_sort");
}
template <bool BE>
inline void suffix_sort(const PackedTextView<BE>& text, device_vector<uint32>& sa, void* stream = nullptr)
{
    device_vector<uint8> temp;
    suffix_sort(text, sa, temp, stream);
}

/// BWT, primary and (want_ssa) the suffix array sampled every sa_int rows, (want_sa) the whole suffix array
template <bool BE>
inline void bwt(const PackedTextView<BE>& text, const uint32 sa_int, BWTResult& out, device_vector<uint8>& temp,
                const bool want_ssa = true, const bool want_sa = false, void* stream = nullptr)
{
    const uint64 n = text.length;
    const uint64 tb = nvbio_hip_bwt_temp_bytes(n);
    if (temp.size() < tb) temp.resize(tb);
    out.bwt_words.resize(4u * ((n + 63u) / 64u));
    if (want_ssa) out.ssa.resize(sa_int ? (n + sa_int) / sa_int : 0u);
    if (want_sa)  out.sa.resize(n + 1u);
    hip_check(nvbio_hip_bwt(text.words, 2u, BE ? 1u : 0u, n, sa_int, out.bwt_words.data(), &out.primary, want_ssa ? out.ssa.data() : nullptr,
                            want_sa ? out.sa.data() : nullptr, temp.data(), temp.size(), stream), "nvbio_hip_bwt");
}
template <bool BE>
inline void bwt(const PackedTextView<BE>& text, const uint32 sa_int, BWTResult& out, const bool want_ssa = true, const bool want_sa = false, void* stream = nullptr)
{
    device_vector<uint8> temp;
    bwt(text, sa_int, out, temp, want_ssa, want_sa, stream);
}

/// what bwt_bytes() returns
struct ByteBWTResult
{
    ByteBWTResult() : primary(0) {}
    uint32                 primary;        ///< the row whose suffix is 0
    device_vector<uint8>   bwt;            ///< n symbols, one byte each, the '$' row dropped
    device_vector<uint32>  ssa;            ///< ceil((n + 1) / sa_int) samples, ssa[0] = 0xFFFFFFFF (empty unless asked for)
    device_vector<uint32>  sa;             ///< n + 1 rows (empty unless asked for)
};

/// suffix_sort for a byte text in device memory: one symbol per byte, of which the low symbol_size (1 to 8) bits are read
inline void suffix_sort_bytes(const uint8* symbols, const uint32 symbol_size, const uint64 n, device_vector<uint32>& sa, device_vector<uint8>& temp, void* stream = nullptr)
{
    const uint64 tb = nvbio_hip_suffix_sort_bytes_temp_bytes(n);
    if (temp.size() < tb) temp.resize(tb);
    sa.resize(n + 1u);
    hip_check(nvbio_hip_suffix_sort_bytes(symbols, symbol_size, n, sa.data(), temp.data(), temp.size(), stream), "nvbio_hip_suffix_sort_bytes");
}

/// bwt for a byte text: the BWT symbols, the primary and (want_ssa) the sampled, (want_sa) the whole suffix array
inline void bwt_bytes(const uint8* symbols, const uint32 symbol_size, const uint64 n, const uint32 sa_int, ByteBWTResult& out, device_vector<uint8>& temp,
                      const bool want_ssa = true, const bool want_sa = false, void* stream = nullptr)
{
    const uint64 tb = nvbio_hip_bwt_bytes_temp_bytes(n);
    if (temp.size() < tb) temp.resize(tb);
    out.bwt.resize(n);
    if (want_ssa) out.ssa.resize(sa_int ? (n + sa_int) / sa_int : 0u);
    if (want_sa)  out.sa.resize(n + 1u);
    hip_check(nvbio_hip_bwt_bytes(symbols, symbol_size, n, sa_int, out.bwt.data(), &out.primary, want_ssa ? out.ssa.data() : nullptr,
                                  want_sa ? out.sa.data() : nullptr, temp.data(), temp.size(), stream), "nvbio_hip_bwt_bytes");
}

/// the slots of a 2-bit string set, the n_suffixes of the calls below: the sum of length + 1 (one copy of the lengths to the host, unless
/// they are fixed)
template <bool BE>
inline uint64 set_slot_count(const PackedStringSetView<2, BE>& set, void* stream = nullptr)
{
    if (!set.m_length) return uint64(set.size()) * (uint64(set.m_fixed_length) + 1u);
    std::vector<uint32> len(set.size());
    hip_check(nvbio_hip_memcpy(len.data(), set.m_length, uint64(set.size()) * 4u, 2, stream), "nvbio_hip_memcpy(d2h)");
    hip_check(nvbio_hip_stream_synchronize(stream), "nvbio_hip_stream_synchronize");
    uint64 n = set.size();
    for (size_t i = 0; i < len.size(); ++i) n += len[i];
    return n;
}

/// what set_suffix_sort() returns
struct SetSuffixSortResult
{
    device_vector<uint32>  suffixes;       ///< n_suffixes global suffix indices, in sorted order
    device_vector<uint32>  string_ids;     ///< the string of every global index
    device_vector<uint32>  cum_lengths;    ///< the inclusive sums of length + 1: string s owns the indices [cum_lengths[s - 1], cum_lengths[s])
};

/// what set_bwt() returns
struct SetBWTResult
{
    device_vector<uint8>   bwt;            ///< n_suffixes bytes: the symbol before the suffix on each row, 255 where it is a whole string
    device_vector<uint32>  dollar_rows;    ///< the rows that hold 255, ascending: one per string
    device_vector<uint32>  dollar_ids;     ///< the string each of them starts
    device_vector<uint32>  suffixes;       ///< 2 * n_suffixes: the (position, string) of every row (empty unless asked for)
};

/// Sort the suffixes of all the strings of `set`, the empty ones included; a proper prefix first, equal suffixes by string id.
/// `temp` is the call's scratch, kept by the caller between calls.  A wrong n_suffixes throws.
template <bool BE>
inline void set_suffix_sort(const PackedStringSetView<2, BE>& set, const uint64 n_suffixes, SetSuffixSortResult& out, device_vector<uint8>& temp, void* stream = nullptr)
{
    const uint64 tb = nvbio_hip_set_suffix_sort_temp_bytes(n_suffixes, set.size());
    if (temp.size() < tb) temp.resize(tb);
    out.suffixes.resize(n_suffixes);
    out.string_ids.resize(n_suffixes);
    out.cum_lengths.resize(set.size());
    const nvbio_hip_string_set s = set.abi();
    hip_check(nvbio_hip_set_suffix_sort(&s, set.size(), n_suffixes, out.suffixes.data(), out.string_ids.data(), out.cum_lengths.data(), temp.data(), temp.size(), stream),
              "nvbio_hip_set_suffix_sort");
}
template <bool BE>
inline void set_suffix_sort(const PackedStringSetView<2, BE>& set, const uint64 n_suffixes, SetSuffixSortResult& out, void* stream = nullptr)
{
    device_vector<uint8> temp;
    set_suffix_sort(set, n_suffixes, out, temp, stream);
}

/// The BWT of the set, its '$' rows and (want_suffixes) the (position, string) pair of every row
template <bool BE>
inline void set_bwt(const PackedStringSetView<2, BE>& set, const uint64 n_suffixes, SetBWTResult& out, device_vector<uint8>& temp,
                    const bool want_suffixes = false, void* stream = nullptr)
{
    const uint64 tb = nvbio_hip_set_bwt_temp_bytes(n_suffixes, set.size());
    if (temp.size() < tb) temp.resize(tb);
    out.bwt.resize(n_suffixes);
    out.dollar_rows.resize(set.size());
    out.dollar_ids.resize(set.size());
    if (want_suffixes) out.suffixes.resize(2u * n_suffixes);
    const nvbio_hip_string_set s = set.abi();
    hip_check(nvbio_hip_set_bwt(&s, set.size(), n_suffixes, out.bwt.data(), out.dollar_rows.data(), out.dollar_ids.data(),
                                want_suffixes ? out.suffixes.data() : nullptr, temp.data(), temp.size(), stream), "nvbio_hip_set_bwt");
}
template <bool BE>
inline void set_bwt(const PackedStringSetView<2, BE>& set, const uint64 n_suffixes, SetBWTResult& out, const bool want_suffixes = false, void* stream = nullptr)
{
    device_vector<uint8> temp;
    set_bwt(set, n_suffixes, out, temp, want_suffixes, stream);
}

} // namespace hip
} // namespace nvbio
