// tests/cxx/mem_split_shim.cpp -- the C++ host layer's MEMFilterDevice (include/nvbio_hip/fmindex.h) with rank's split_len /
// split_width behind one C entry point that tests/test_mem_split_gpu.py calls.  g++, no HIP.
#include "nvbio_hip/fmindex.h"
#include <stdio.h>
#include <exception>

using namespace nvbio;

namespace {
struct Set
{
    nvbio_hip_string_set s; uint32 n;
    nvbio_hip_string_set abi() const { return s; }
    uint32 size() const { return n; }
};
}

/// rank with re-seeding, then copy out the rank records (at most `cap`), their slots, the index and every string's first hit; locate
/// [begin, end) into d_hits
extern "C" __attribute__((visibility("default")))
int mem_split_host_class(const nvbio_hip_fmindex* f, const nvbio_hip_fmindex* r, const nvbio_hip_string_set* strings, unsigned n,
                         unsigned min_intv, unsigned max_intv, unsigned min_span, unsigned split_len, unsigned split_width, unsigned long long cap,
                         unsigned* ranges, unsigned long long* slots, unsigned long long* index, unsigned long long* first_hits,
                         unsigned long long* n_ranges, unsigned long long* n_mems, unsigned long long begin, unsigned long long end, unsigned* d_hits)
{
    try {
        fm_index_device fi, ri;
        fi.m = *f; ri.m = *r;
        const Set set = { *strings, n };
        MEMFilterDevice filter;
        *n_mems = filter.rank(fi, ri, set, min_intv, max_intv, min_span, split_len, split_width);
        *n_ranges = filter.n_ranges();
        if (filter.n_hits() != *n_mems || filter.n_ranges() > cap) return -2;
        if (filter.n_ranges())
        {
            hip_check(nvbio_hip_memcpy(ranges, filter.ranges(), filter.n_ranges() * 16u, 2, nullptr), "nvbio_hip_memcpy");
            hip_check(nvbio_hip_memcpy(slots, filter.ranks(), filter.n_ranges() * 8u, 2, nullptr), "nvbio_hip_memcpy");
        }
        hip_check(nvbio_hip_memcpy(index, filter.index(), (uint64(n) + 1u) * 8u, 2, nullptr), "nvbio_hip_memcpy");
        for (unsigned i = 0; i < n; ++i) first_hits[i] = filter.first_hit(i);
        filter.locate(begin, end, reinterpret_cast<uint4*>(d_hits));
        hip_check(nvbio_hip_stream_synchronize(nullptr), "nvbio_hip_stream_synchronize");
        return 0;
    } catch (const std::exception& e) { fprintf(stderr, "mem_split_host_class: %s\n", e.what()); return -1; }
}
