// compat/nvbio/fmindex/bidir.h -- extend_forward / extend_backwards on a bidirectional FM-index (nvbio/fmindex/bidir.h,
// bidir_inl.h:48-144): a forward index of the text T and an index of its reverse, searched in step.  For a string P whose
// range is f_range in the forward index and whose reverse P^R has r_range in the reverse index, extend_forward yields the
// two ranges of Pc and extend_backwards those of cP.
//
// Two things differ from the reference:
//   * the row of the suffix that IS the string.  The forward rows of P are, in order: the suffix that equals P (present iff P
//     ends the text, i.e. iff the reverse index's primary row lies in r_range), then the suffixes that start with P0, P1, P2,
//     P3.  The reference counts only the Pd, d < c, in front of Pc, so from the ranges of the empty string, (0, length) for both
//     indices, every range it returns sits one row too low (row 0, the empty suffix, is never counted).  Here the offset also
//     counts that row, and the ranges equal match()'s at every step;
//   * the counts of every d <= c come from one rank4 per end of the range, two records a step, instead of up to 2(c+1) range
//     ranks.
#pragma once
#include "fmindex.h"

namespace nvbio {

namespace priv {
template <typename vec4_type>
NVBIO_FORCEINLINE NVBIO_HOST_DEVICE uint32 comp4(const vec4_type& v, const uint32 c) { return c <= 1u ? (c == 0u ? v.x : v.y) : (c == 2u ? v.z : v.w); }

/// how many 64-symbol records of the production layout a step from `range` reads: one per end of (x - 1, y) that is a row of the
/// BWT, one for both when they fall in the same record (what the device kernels load; the accounting of the `_host` twins)
template <typename index_type, typename range_type>
NVBIO_FORCEINLINE NVBIO_HOST_DEVICE uint32 range_records(const index_type& index, const range_type range)
{
    typedef typename index_type::index_type coord_type;
    coord_type k[2] = { coord_type(range.x - 1), coord_type(range.y) };
    bool need[2];
    for (uint32 e = 0; e < 2u; ++e)
    {
        need[e] = !(k[e] == coord_type(-1) || k[e] == index.length());
        if (need[e] && k[e] >= index.primary()) --k[e];
        if (need[e] && k[e] == coord_type(-1)) need[e] = false;
    }
    if (need[0] && need[1]) return (k[0] >> 6) == (k[1] >> 6) ? 1u : 2u;
    return (need[0] || need[1]) ? 1u : 0u;
}

/// one step on `index` (the range of cS from the range of S) and how many rows of S sort before those that continue with c
template <typename index_type, typename range_type>
NVBIO_FORCEINLINE NVBIO_HOST_DEVICE uint32 bidir_step(const index_type& index, range_type& range, const uint8 c)
{
    typedef typename index_type::index_type coord_type;
    typename index_type::rank_dictionary_type::vec4_type lo, hi;
    rank4(index, make_vector(coord_type(range.x - 1), range.y), &lo, &hi);
    // the row whose BWT symbol is '$' belongs to the occurrence that nothing precedes: it sorts first in the other index
    uint32 before = (range.x <= index.primary() && index.primary() <= range.y) ? 1u : 0u;
    for (uint32 d = 0; d < c; ++d) before += comp4(hi, d) - comp4(lo, d);
    range.x = index.L2(c) + comp4(lo, c) + 1;
    range.y = index.L2(c) + comp4(hi, c);
    return before;
}
} // namespace priv

/// the ranges of Pc from those of P   (bidir_inl.h:48-87)
template <typename R1, typename S1, typename L1, typename R2, typename S2, typename L2>
NVBIO_FORCEINLINE NVBIO_HOST_DEVICE
void extend_forward(const fm_index<R1, S1, L1>& f_fmi, const fm_index<R2, S2, L2>& r_fmi,
                    typename fm_index<R1, S1, L1>::range_type& f_range, typename fm_index<R2, S2, L2>::range_type& r_range, const uint8 c)
{
    (void)f_fmi;
    const uint32 x = priv::bidir_step(r_fmi, r_range, c);
    const uint32 y = 1u + r_range.y - r_range.x;
    f_range.y = f_range.x + x + y - 1u;
    f_range.x = f_range.x + x;
}

/// the ranges of cP from those of P   (bidir_inl.h:105-144)
template <typename R1, typename S1, typename L1, typename R2, typename S2, typename L2>
NVBIO_FORCEINLINE NVBIO_HOST_DEVICE
void extend_backwards(const fm_index<R1, S1, L1>& f_fmi, const fm_index<R2, S2, L2>& r_fmi,
                      typename fm_index<R1, S1, L1>::range_type& f_range, typename fm_index<R2, S2, L2>::range_type& r_range, const uint8 c)
{
    (void)r_fmi;
    const uint32 x = priv::bidir_step(f_fmi, f_range, c);
    const uint32 y = 1u + f_range.y - f_range.x;
    r_range.y = r_range.x + x + y - 1u;
    r_range.x = r_range.x + x;
}

} // namespace nvbio
