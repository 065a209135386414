// tests/compat/mem_split_callers.hip -- callers of MEMFilter::rank with its last two arguments, split_len and split_width, written in
// the reference's vocabulary as nvmem/mem-search.cu:128-129 calls it: MEMFilterHost and MEMFilterDevice over a string set.  It
// includes the reference's header names and is compiled with `hipcc -I include/nvbio_hip/compat`; the fm_index is the production
// layout exactly as nvbio/io/fmindex/fmindex.h:159-174 composes it.  The extern "C" entry points exist so that the Python tests can
// drive it.
#include <nvbio/basic/types.h>
#include <nvbio/basic/packedstream.h>
#include <nvbio/basic/deinterleaved_iterator.h>
#include <nvbio/strings/string_set.h>
#include <nvbio/fmindex/ssa.h>
#include <nvbio/fmindex/fmindex.h>
#include <nvbio/fmindex/bidir.h>
#include <nvbio/fmindex/mem.h>
#include <string.h>
#include <stdio.h>

using namespace nvbio;

#define API extern "C" __attribute__((visibility("default")))

typedef deinterleaved_iterator<2, 0, const uint4*>                  bwt_words_type;
typedef deinterleaved_iterator<2, 1, const uint4*>                  occ_type;
typedef PackedStream<bwt_words_type, uint8, 2, true>                bwt_type;
typedef rank_dictionary<2, 64, bwt_type, occ_type, null_type>       rank_dict_type;
typedef SSA_index_multiple_context<4, const uint32*>                ssa_type;
typedef fm_index<rank_dict_type, ssa_type>                          fm_index_type;
typedef PackedStream<const uint32*, uint8, 4, true>                 read_stream;
typedef SparseStringSet<read_stream, const uint2*>                  read_set;

static fm_index_type make_index(const uint32 n, const uint32 primary, const uint32* L2, const uint32* bwt_occ, const uint32* ssa)
{
    const uint4* base = reinterpret_cast<const uint4*>(bwt_occ);
    return fm_index_type(n, primary, L2, rank_dict_type(bwt_type(bwt_words_type(base)), occ_type(base), null_type()), ssa_type(ssa));
}

// ---- MEMFilterHost: rank with re-seeding, first_hit, locate -- everything in host memory
API int compat_mem_split_host(uint32 n, uint32 f_primary, const uint32* f_L2, const uint32* f_bwt_occ, const uint32* f_ssa,
                              uint32 r_primary, const uint32* r_L2, const uint32* r_bwt_occ, const uint32* r_ssa,
                              const uint32* read_words, const uint2* read_ranges, uint32 n_reads, uint32 min_intv, uint32 max_intv, uint32 min_span,
                              uint32 split_len, uint32 split_width,
                              unsigned long long* out_n_mems, unsigned long long* out_n_ranges, uint4* out_ranges, unsigned long long* out_slots, uint32 capacity,
                              unsigned long long* out_first_hit, unsigned long long begin, unsigned long long end, uint4* out_hits)
{
    try {
        const fm_index_type f_index = make_index(n, f_primary, f_L2, f_bwt_occ, f_ssa);
        const fm_index_type r_index = make_index(n, r_primary, r_L2, r_bwt_occ, r_ssa);
        const read_set reads(n_reads, read_stream(read_words), read_ranges);

        typedef MEMFilterHost<fm_index_type> mem_filter_type;
        mem_filter_type mem_filter;
        *out_n_mems   = mem_filter.rank(f_index, r_index, reads, min_intv, max_intv, min_span, split_len, split_width);
        *out_n_ranges = mem_filter.n_ranges();
        if (mem_filter.n_ranges() > capacity || mem_filter.n_hits() != mem_filter.n_mems()) return -2;
        for (uint64 k = 0; k < mem_filter.n_ranges(); ++k)
        {
            const mem_filter_type::rank_type rk = mem_filter.ranges()[k];
            out_ranges[k] = make_uint4(rk.range().x, rk.range().y, rk.string_id() | (rk.group_flag() ? 1u << 31 : 0u), rk.span().x | (rk.span().y << 16));
            out_slots[k]  = mem_filter.ranks()[k];
        }
        for (uint32 i = 0; i < n_reads; ++i) out_first_hit[i] = mem_filter.first_hit(i);
        std::vector<mem_filter_type::mem_type> mems(end - begin);
        mem_filter.locate(begin, end, mems.begin());
        for (uint64 h = 0; h < end - begin; ++h) out_hits[h] = make_uint4(mems[h].index_pos(), mems[h].string_id(), mems[h].span().x, mems[h].span().y);
        return 0;
    } catch (const std::exception& e) { fprintf(stderr, "compat_mem_split_host: %s\n", e.what()); return -1; }
}

// ---- MEMFilterDevice: every pointer is device memory.  bits = 4: the reads are 4-bit packed words (the filter's tuned execution,
// unless tuned = 0); bits = 8: one byte a symbol, which the C-ABI does not take (the per-lane templates rank).  path / locate_path
// receive last_path() after rank / locate.
template <typename read_set_type>
static int run_device_filter(const bool tuned, const fm_index_type& f_index, const fm_index_type& r_index, const read_set_type& reads, uint32 n_reads,
                             uint32 min_intv, uint32 max_intv, uint32 min_span, uint32 split_len, uint32 split_width,
                             unsigned long long* out_n_mems, unsigned long long* out_n_ranges,
                             uint4* out_ranges, unsigned long long* out_slots, unsigned long long* out_index, uint32 capacity, unsigned long long* out_first_hit,
                             unsigned long long begin, unsigned long long end, uint4* out_hits, char* path, char* locate_path)
{
    typedef MEMFilterDevice<fm_index_type> mem_filter_type;
    mem_filter_type mem_filter;
    mem_filter.set_tuned(tuned);
    *out_n_mems   = mem_filter.rank(f_index, r_index, reads, min_intv, max_intv, min_span, split_len, split_width);
    *out_n_ranges = mem_filter.n_ranges();
    strncpy(path, mem_filter.last_path(), 15);
    if (mem_filter.n_ranges() > capacity || mem_filter.n_hits() != mem_filter.n_mems()) return -2;
    (void)hipMemcpy(out_ranges, mem_filter.ranges(), sizeof(uint4) * mem_filter.n_ranges(), hipMemcpyDeviceToDevice);
    (void)hipMemcpy(out_slots, mem_filter.ranks(), sizeof(uint64) * mem_filter.n_ranges(), hipMemcpyDeviceToDevice);
    (void)hipMemcpy(out_index, mem_filter.index(), sizeof(uint64) * (n_reads + 1u), hipMemcpyDeviceToDevice);
    for (uint32 i = 0; i < n_reads; ++i) out_first_hit[i] = mem_filter.first_hit(i);      // host array
    mem_filter.locate(begin, end, reinterpret_cast<mem_filter_type::mem_type*>(out_hits));
    strncpy(locate_path, mem_filter.last_path(), 15);
    return int(hipDeviceSynchronize());
}

API int compat_mem_split_filter_device(uint32 bits, uint32 tuned, uint32 n, uint32 f_primary, const uint32* f_L2, const uint32* f_bwt_occ, const uint32* f_ssa,
                                       uint32 r_primary, const uint32* r_L2, const uint32* r_bwt_occ, const uint32* r_ssa,
                                       const void* read_symbols, const uint2* read_ranges, uint32 n_reads, uint32 min_intv, uint32 max_intv, uint32 min_span,
                                       uint32 split_len, uint32 split_width,
                                       unsigned long long* out_n_mems, unsigned long long* out_n_ranges, uint4* out_ranges, unsigned long long* out_slots,
                                       unsigned long long* out_index, uint32 capacity, unsigned long long* out_first_hit,
                                       unsigned long long begin, unsigned long long end, uint4* out_hits, char* path, char* locate_path)
{
    try {
        const fm_index_type f_index = make_index(n, f_primary, f_L2, f_bwt_occ, f_ssa);
        const fm_index_type r_index = make_index(n, r_primary, r_L2, r_bwt_occ, r_ssa);
        if (bits == 4)
            return run_device_filter(tuned != 0u, f_index, r_index, read_set(n_reads, read_stream(reinterpret_cast<const uint32*>(read_symbols)), read_ranges), n_reads,
                                     min_intv, max_intv, min_span, split_len, split_width,
                                     out_n_mems, out_n_ranges, out_ranges, out_slots, out_index, capacity, out_first_hit, begin, end, out_hits, path, locate_path);
        return run_device_filter(tuned != 0u, f_index, r_index, SparseStringSet<const uint8*, const uint2*>(n_reads, reinterpret_cast<const uint8*>(read_symbols), read_ranges), n_reads,
                                 min_intv, max_intv, min_span, split_len, split_width,
                                 out_n_mems, out_n_ranges, out_ranges, out_slots, out_index, capacity, out_first_hit, begin, end, out_hits, path, locate_path);
    } catch (const std::exception& e) { fprintf(stderr, "compat_mem_split_filter_device: %s\n", e.what()); return -1; }
}
