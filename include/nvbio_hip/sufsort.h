// include/nvbio_hip/sufsort.h -- the C++ host layer of the suffix sorter and BWT builder (nvbio/sufsort/sufsort.h for one plain string):
// thin callers of nvbio_hip_suffix_sort / nvbio_hip_bwt (include/nvbio_hip.h) over the project's device vectors.
// No HIP headers are needed to include it.
//
//   PackedTextView<BIG_ENDIAN>   a 2-bit packed text in device memory: words + length
//   suffix_sort(text, sa)        sa: n + 1 rows, sa[0] = n, a suffix that is a proper prefix of another first
//   bwt(text, sa_int, out)       the BWT with the '$' row dropped (big-endian words, what nvbio_hip_build_bwt_occ takes), the primary,
//                                and on request the sampled and the whole suffix array
#pragma once
#include "types.h"

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

} // namespace hip
} // namespace nvbio
