// fm_bidir.h -- per-lane steps on a bidirectional FM-index (a forward index and the index of the reversed text): the reference's
// extend_forward / extend_backwards (nvbio/fmindex/bidir_inl.h:48-144) on the reference-layout records every index carries.
//
// For a string P with rows [f.x, f.y] in the forward index, and P reversed with rows [r.x, r.y] in the reverse index, the rows of Pc
// follow, inside [f.x, f.y], the row of the suffix that IS P (there iff the reverse index's primary row lies in [r.x, r.y]) and the
// rows of every Pd, d < c.  The reference leaves that one row out, so from (0, length) all its ranges sit one row low (DESIGN.md
// 3.12).  The counts of all d <= c come from one rank4 at each end of the range -- two records a step where the reference's loop
// issues up to 2(c+1) range ranks.
#pragma once
#include "fmindex_device.h"

namespace nvb {

// one step on `g`: range <- the rows of cS from the rows of S; returns how many rows of S sort, in the OTHER index, before those of Sc
__device__ __forceinline__ uint32_t bidir_step(const Fmi& g, uint2& range, const uint32_t c)
{
    uint4 lo, hi;
    fm_rank4_range(g, range.x - 1u, range.y, lo, hi);
    uint32_t before = (range.x <= g.primary && g.primary <= range.y) ? 1u : 0u;
    before += c > 0u ? hi.x - lo.x : 0u;
    before += c > 1u ? hi.y - lo.y : 0u;
    before += c > 2u ? hi.z - lo.z : 0u;
    range.x = g.L2[c] + comp(lo, c) + 1u;
    range.y = g.L2[c] + comp(hi, c);
    return before;
}

// (f, r) of P -> (f, r) of Pc; r_fmi is the reverse index
__device__ __forceinline__ void fm_extend_forward(const Fmi& r_fmi, uint2& f, uint2& r, const uint32_t c)
{
    const uint32_t x = bidir_step(r_fmi, r, c);
    f.x += x;
    f.y = f.x + (r.y - r.x);             // an emptied range keeps y = x - 1
}
// (f, r) of P -> (f, r) of cP; f_fmi is the forward index
__device__ __forceinline__ void fm_extend_backwards(const Fmi& f_fmi, uint2& f, uint2& r, const uint32_t c)
{
    const uint32_t x = bidir_step(f_fmi, f, c);
    r.x += x;
    r.y = r.x + (f.y - f.x);
}

} // namespace nvb
