// fm_mem_args.h -- the argument checks shared by the four MEM rank entries: nvbio_hip_fm_mem_rank / _rank_split (fm_mem.hip) and their
// `_host` twins (host_twins.hip).  Host only.
#pragma once
#include <hip/hip_runtime_api.h>
#include "../../include/nvbio_hip.h"

namespace nvb {

// what mem_rank_admission answers besides an error code
enum { MEM_ARGS_GO = -1, MEM_ARGS_EMPTY = -2 };

// An error code, MEM_ARGS_EMPTY (no string has a symbol: the caller zeroes the n + 1 entries of out_index and succeeds) or MEM_ARGS_GO.
// *out_n_ranges is zeroed once the pointers are known to be there, and zero_outputs() then zeroes what else the caller can write from
// the host (the twins: *out_records and out_index[0]).  hipErrorNotSupported (a symbol width the kernels do not read) comes
// before any check a caller adds -- the temp size, the twins' scan of the lengths: the drop-in layer falls back to its templates on it.
template <typename ZeroOutputs>
inline int mem_rank_admission(const nvbio_hip_fmindex* f, const nvbio_hip_fmindex* r, const nvbio_hip_string_set* strings,
                              const uint32_t n, const uint32_t max_pattern_len, const uint32_t min_intv,
                              const uint32_t* out_ranges, const uint64_t capacity, const uint64_t* out_index, const uint64_t* out_slots, uint64_t* out_n_ranges,
                              const ZeroOutputs zero_outputs)
{
    if (!f || !r || !f->bwt_occ || !r->bwt_occ || f->length != r->length) return hipErrorInvalidValue;
    if (!out_index || !out_n_ranges || min_intv == 0u) return hipErrorInvalidValue;
    if (n >= 0x80000000u || max_pattern_len > 65535u) return hipErrorInvalidValue;
    if (capacity != 0u && (!out_ranges || !out_slots)) return hipErrorInvalidValue;
    *out_n_ranges = 0;
    zero_outputs();
    if (n == 0 || max_pattern_len == 0) return MEM_ARGS_EMPTY;
    if (!strings || !strings->words || !strings->begin || strings->n_words == 0) return hipErrorInvalidValue;
    if (!(strings->bits == 2 || strings->bits == 4)) return hipErrorNotSupported;
    if (!strings->length && strings->fixed_length > max_pattern_len) return hipErrorInvalidValue;
    return MEM_ARGS_GO;
}

} // namespace nvb
