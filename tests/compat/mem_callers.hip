// tests/compat/mem_callers.hip -- callers of the bidirectional FM-index interface written in the reference's vocabulary
// (nvbio/fmindex/bidir.h, nvbio/fmindex/mem.h, as examples/mem/mem.cu uses it): MEMFilterHost and MEMFilterDevice over a string set, and a kernel
// in which every thread runs find_kmems / extend_forward / extend_backwards itself, with a delegate of the interface of
// mem.h:56-68.  It includes the reference's header names and is compiled with `hipcc -I include/nvbio_hip/compat`; the
// fm_index is the production layout exactly as nvbio/io/fmindex/fmindex.h:159-174 composes it.  The extern "C" entry points
// exist so that the Python tests can drive it.
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

// ---- MEMFilterHost: rank, first_hit, string_batch_bound, locate -- everything in host memory
API int compat_mem_host(uint32 n, uint32 f_primary, const uint32* f_L2, const uint32* f_bwt_occ, const uint32* f_ssa,
                        uint32 r_primary, const uint32* r_L2, const uint32* r_bwt_occ, const uint32* r_ssa,
                        const uint32* read_words, const uint2* read_ranges, uint32 n_reads, uint32 min_intv, uint32 max_intv, uint32 min_span,
                        unsigned long long* out_n_mems, unsigned long long* out_n_ranges, uint4* out_ranges, unsigned long long* out_slots, uint32 capacity,
                        unsigned long long* out_first_hit, uint32 bound_count, uint32* out_bound,
                        unsigned long long begin, unsigned long long end, uint4* out_hits)
{
    try {
        const fm_index_type f_index = make_index(n, f_primary, f_L2, f_bwt_occ, f_ssa);
        const fm_index_type r_index = make_index(n, r_primary, r_L2, r_bwt_occ, r_ssa);
        const read_set reads(n_reads, read_stream(read_words), read_ranges);

        typedef MEMFilterHost<fm_index_type> mem_filter_type;
        mem_filter_type mem_filter;
        *out_n_mems   = mem_filter.rank(f_index, r_index, reads, min_intv, max_intv, min_span);
        *out_n_ranges = mem_filter.n_ranges();
        if (mem_filter.n_ranges() > capacity || mem_filter.n_hits() != mem_filter.n_mems()) return -2;
        for (uint64 k = 0; k < mem_filter.n_ranges(); ++k)
        {
            const mem_filter_type::rank_type rk = mem_filter.ranges()[k];
            // through the record's own accessors
            out_ranges[k] = make_uint4(rk.range().x, rk.range().y, rk.string_id() | (rk.group_flag() ? 1u << 31 : 0u), rk.span().x | (rk.span().y << 16));
            out_slots[k]  = mem_filter.ranks()[k];
        }
        for (uint32 i = 0; i < n_reads; ++i) out_first_hit[i] = mem_filter.first_hit(i);
        *out_bound = string_batch_bound(mem_filter, bound_count);
        std::vector<mem_filter_type::mem_type> mems(end - begin);
        mem_filter.locate(begin, end, mems.begin());
        for (uint64 h = 0; h < end - begin; ++h) out_hits[h] = make_uint4(mems[h].index_pos(), mems[h].string_id(), mems[h].span().x, mems[h].span().y);
        return 0;
    } catch (const std::exception& e) { fprintf(stderr, "compat_mem_host: %s\n", e.what()); return -1; }
}

// ---- the per-thread templates in a kernel: one thread per read walks it with find_kmems into its own slice of the outputs
struct mem_writer
{
    typedef fm_index_type::range_type range_type;
    uint4* out; uint32 n, capacity, string_id, max_intv;
    NVBIO_HOST_DEVICE void output(const range_type range, const uint2 span)
    {
        if (1u + range.y - range.x > max_intv) return;
        if (n < capacity) out[n] = MEMRange<uint32>(range, string_id, span).coords;
        ++n;
    }
};

__global__ void __launch_bounds__(64) mem_kernel(const fm_index_type f_index, const fm_index_type r_index, const read_set reads, const uint32 n_reads,
                                                 const uint32 min_intv, const uint32 max_intv, const uint32 min_span,
                                                 uint4* store, const uint32 max_len, uint4* out, const uint32 per_read, uint32* counts)
{
    const uint32 id = blockIdx.x * 64u + threadIdx.x;
    if (id >= n_reads) return;
    const read_set::string_type read = reads[id];
    const uint32 len = length(read) < max_len ? length(read) : max_len;
    uint4* my_store = store + size_t(id) * max_len;
    mem_writer writer = { out + size_t(id) * per_read, 0u, per_read, id, max_intv };
    for (uint32 x = 0; x < len;)
    {
        const uint32 e = find_kmems(len, read, x, f_index, r_index, writer, min_intv, min_span, my_store);
        x = nvbio::max(e, x + 1u);
    }
    counts[id] = writer.n;
}

// one thread per read: grow the read symbol by symbol with extend_forward from the empty string, then shrink-side with
// extend_backwards from the empty string over the same symbols; the final four ranges go out
__global__ void __launch_bounds__(64) extend_kernel(const fm_index_type f_index, const fm_index_type r_index, const read_set reads, const uint32 n_reads, uint2* out)
{
    const uint32 id = blockIdx.x * 64u + threadIdx.x;
    if (id >= n_reads) return;
    const read_set::string_type read = reads[id];
    const uint32 len = length(read);
    fm_index_type::range_type f = make_uint2(0u, f_index.length()), r = make_uint2(0u, r_index.length());
    for (uint32 i = 0; i < len && f.x <= f.y; ++i) { if (read[i] > 3) { f = r = make_uint2(1u, 0u); break; } extend_forward(f_index, r_index, f, r, read[i]); }
    out[4 * id] = f; out[4 * id + 1] = r;
    f = make_uint2(0u, f_index.length()); r = make_uint2(0u, r_index.length());
    for (int32 i = int32(len) - 1; i >= 0 && f.x <= f.y; --i) { if (read[i] > 3) { f = r = make_uint2(1u, 0u); break; } extend_backwards(f_index, r_index, f, r, read[i]); }
    out[4 * id + 2] = f; out[4 * id + 3] = r;
}

/// every pointer is device memory; store: n_reads * max_len uint4 of scratch; out: per_read records a read
API int compat_mem_device(uint32 n, uint32 f_primary, const uint32* f_L2, const uint32* f_bwt_occ, const uint32* f_ssa,
                          uint32 r_primary, const uint32* r_L2, const uint32* r_bwt_occ, const uint32* r_ssa,
                          const uint32* read_words, const uint2* read_ranges, uint32 n_reads, uint32 min_intv, uint32 max_intv, uint32 min_span,
                          uint4* store, uint32 max_len, uint4* out, uint32 per_read, uint32* counts, uint2* out_extend)
{
    const fm_index_type f_index = make_index(n, f_primary, f_L2, f_bwt_occ, f_ssa);
    const fm_index_type r_index = make_index(n, r_primary, r_L2, r_bwt_occ, r_ssa);
    const read_set reads(n_reads, read_stream(read_words), read_ranges);
    if (n_reads == 0) return 0;
    hipLaunchKernelGGL(mem_kernel, dim3((n_reads + 63u) / 64u), dim3(64), 0, 0, f_index, r_index, reads, n_reads, min_intv, max_intv, min_span,
                       store, max_len, out, per_read, counts);
    if (hipError_t e = hipGetLastError()) return int(e);
    hipLaunchKernelGGL(extend_kernel, dim3((n_reads + 63u) / 64u), dim3(64), 0, 0, f_index, r_index, reads, n_reads, out_extend);
    if (hipError_t e = hipGetLastError()) return int(e);
    return int(hipDeviceSynchronize());
}

// ---- MEMFilterDevice, as examples/mem/mem.cu holds it (a `MEMFilterDevice<fm_index_type> mem_filter` member: rank the reads, loop
// over batches of hits with locate): every pointer is device memory.  bits = 4: the reads are 4-bit packed words (the filter's tuned
// execution, unless tuned = 0); bits = 8: one byte a symbol, which the C-ABI does not take (the per-lane templates rank; locate, which
// reads no string, still takes the C-ABI unless tuned = 0).  path / locate_path receive last_path() after rank / locate.
template <typename read_set_type>
static int run_device_filter(const bool tuned, const fm_index_type& f_index, const fm_index_type& r_index, const read_set_type& reads, uint32 n_reads,
                             uint32 min_intv, uint32 max_intv, uint32 min_span, unsigned long long* out_n_mems, unsigned long long* out_n_ranges,
                             uint4* out_ranges, unsigned long long* out_slots, unsigned long long* out_index, uint32 capacity, unsigned long long* out_first_hit,
                             unsigned long long begin, unsigned long long end, uint4* out_hits, char* path, char* locate_path)
{
    typedef MEMFilterDevice<fm_index_type> mem_filter_type;
    mem_filter_type mem_filter;
    mem_filter.set_tuned(tuned);
    *out_n_mems   = mem_filter.rank(f_index, r_index, reads, min_intv, max_intv, min_span);
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

API int compat_mem_filter_device(uint32 bits, uint32 tuned, uint32 n, uint32 f_primary, const uint32* f_L2, const uint32* f_bwt_occ, const uint32* f_ssa,
                                 uint32 r_primary, const uint32* r_L2, const uint32* r_bwt_occ, const uint32* r_ssa,
                                 const void* read_symbols, const uint2* read_ranges, uint32 n_reads, uint32 min_intv, uint32 max_intv, uint32 min_span,
                                 unsigned long long* out_n_mems, unsigned long long* out_n_ranges, uint4* out_ranges, unsigned long long* out_slots,
                                 unsigned long long* out_index, uint32 capacity, unsigned long long* out_first_hit,
                                 unsigned long long begin, unsigned long long end, uint4* out_hits, char* path, char* locate_path)
{
    try {
        const fm_index_type f_index = make_index(n, f_primary, f_L2, f_bwt_occ, f_ssa);
        const fm_index_type r_index = make_index(n, r_primary, r_L2, r_bwt_occ, r_ssa);
        if (bits == 4)
            return run_device_filter(tuned != 0u, f_index, r_index, read_set(n_reads, read_stream(reinterpret_cast<const uint32*>(read_symbols)), read_ranges), n_reads, min_intv, max_intv, min_span,
                                     out_n_mems, out_n_ranges, out_ranges, out_slots, out_index, capacity, out_first_hit, begin, end, out_hits, path, locate_path);
        return run_device_filter(tuned != 0u, f_index, r_index, SparseStringSet<const uint8*, const uint2*>(n_reads, reinterpret_cast<const uint8*>(read_symbols), read_ranges), n_reads,
                                 min_intv, max_intv, min_span, out_n_mems, out_n_ranges, out_ranges, out_slots, out_index, capacity, out_first_hit, begin, end, out_hits, path, locate_path);
    } catch (const std::exception& e) { fprintf(stderr, "compat_mem_filter_device: %s\n", e.what()); return -1; }
}
