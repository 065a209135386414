// fm_mem.hip -- maximal exact matches on a bidirectional FM-index for gfx950: the device side of the reference's MEMFilter
// (nvbio/fmindex/mem.h, mem_inl.h) and the batched extend_forward / extend_backwards of nvbio/fmindex/bidir.h.
//
// What is computed is defined in DESIGN.md 3.12 (the k-SMEMs of every string, filtered by min_span and max_intv, ordered by
// begin), not the reference's output: see fm_bidir.h for the start row the reference leaves out.
//
// One lane = one string; a lane walks its string with the reference's skeleton (mem_inl.h:36-171), corrected:
//   from x, extend right on the reverse index, keeping (SA range, end) of each extension whose range is larger than the next one's,
//   and of the last; for each kept range, shortest first, search backwards from x - 1 on the forward index: begins can only grow
//   with the length, and a span is a k-SMEM exactly when it begins before the next longer one; then x = max(right-most end, x + 1).
// Every step is a dependent gather of one or two 32-byte records of the reference layout (the line-native records and the k-mer
// table are not used: a bidirectional step needs all four counts at both ends, which is what a bwt|occ record holds).  Jobs are
// independent, so the kernel sits on the same random-line bound as fm_match_kernel and is launched the same way: 256 lanes a
// block, as many waves in flight as the registers allow.
//
// The kept ranges (at most L - x of them, 12 bytes each) live in caller-provided temp, lane-interleaved within a wave: entry j of
// lane l is three dwords at ((wave * max_len + j) * 3 + w) * 64 + l, so a wave's store of one word is one 256-byte line.  The
// lanes are persistent (a grid-stride loop over the strings), which bounds that memory by the lanes in flight, not by n.
//
// rank is two passes of the same walk: the first counts the reported MEMs of every string, a scan turns the counts into the
// exclusive index, the second writes each record to its place.  Nothing is written past `capacity`.
//
// The plain and the re-seeding entry differ in their kernels and in what follows the first pass.  What they share is written once:
// the argument checks (mem_rank_admission, fm_mem_args.h, with the `_host` twins), the temp layout (MemTemp: mem_temp_carve places
// it, and the size queries ask the same function), the first pass (mem_count_pass) and a lane's view of its string (mem_lane_string).
#include "fm_bidir.h"
#include "fm_mem_args.h"
#include <hipcub/hipcub.hpp>

namespace nvb {

static const uint32_t MEM_MAX_BLOCKS = 2048u;       // 256 CUs x 4 SIMDs x 8 waves: every wave slot of the chip once

// 16 symbols of the pattern at a time, kept across the steps that stay inside the group
struct PatternCursor {
    uint64_t grp; uint32_t g0;
};
__device__ __forceinline__ uint32_t pattern_symbol(const Stream& s, const uint64_t begin, PatternCursor& pc, const uint32_t i)
{
    const uint32_t g = i & ~15u;
    if (g != pc.g0) { pc.g0 = g; pc.grp = (s.bits == 4) ? fetch16_4bit(s, begin + g) : expand_2to4(fetch16_2bit(s, begin + g)); }
    return uint32_t(pc.grp >> (4u * (i & 15u))) & 15u;
}

// one group of the walk: the k-SMEMs (k = min_intv) that cover symbol x go to report(range, begin, end), begin ascending; returns the
// next x.  `st` holds the kept ranges: entry j, word w at st[(j * 3 + w) * 64].
template <typename Report>
__device__ __forceinline__ uint32_t mem_group(const Fmi& f, const Fmi& r, const StringSet& strings, const uint64_t pbegin, PatternCursor& pc,
                                              const uint32_t len, const uint32_t x, const uint32_t min_intv, uint32_t* const st, Report&& report)
{
    // ---- right extension from x
    uint32_t m = 0, i;
    {
        uint2 fr = make_uint2(0u, f.length), rr = make_uint2(0u, r.length);
        for (i = x; i < len; ++i)
        {
            const uint32_t c = pattern_symbol(strings.s, pbegin, pc, i);
            if (c > 3u) break;
            uint2 nf = fr, nr = rr;
            fm_extend_forward(r, nf, nr, c);
            const uint32_t size = nf.y - nf.x + 1u;
            if (size < min_intv) break;
            if (i > x && size != fr.y - fr.x + 1u)
            {
                st[(m * 3u + 0u) * 64u] = fr.x; st[(m * 3u + 1u) * 64u] = fr.y; st[(m * 3u + 2u) * 64u] = i;
                ++m;
            }
            fr = nf; rr = nr;
        }
        if (i > x)
        {
            st[(m * 3u + 0u) * 64u] = fr.x; st[(m * 3u + 1u) * 64u] = fr.y; st[(m * 3u + 2u) * 64u] = i;
            ++m;
        }
    }
    // ---- left extension of each kept range, shortest first; a span is held until the next one's begin is known
    bool held = false;
    uint2 hg = make_uint2(0u, 0u);
    uint32_t hb = 0, he = 0;
    for (uint32_t j = 0; j < m; ++j)
    {
        uint2 g = make_uint2(st[(j * 3u + 0u) * 64u], st[(j * 3u + 1u) * 64u]);
        const uint32_t e = st[(j * 3u + 2u) * 64u];
        int32_t l;
        for (l = int32_t(x) - 1; l >= 0; --l)
        {
            const uint32_t c = pattern_symbol(strings.s, pbegin, pc, uint32_t(l));
            if (c > 3u) break;
            const uint2 k = fm_rank2(f, g.x - 1u, g.y, c);
            const uint2 ng = make_uint2(f.L2[c] + k.x + 1u, f.L2[c] + k.y);
            if (ng.y - ng.x + 1u < min_intv) break;
            g = ng;
        }
        const uint32_t b = uint32_t(l + 1);
        if (held && hb < b) report(hg, hb, he);
        held = true; hg = g; hb = b; he = e;
    }
    if (held) report(hg, hb, he);
    return (m != 0u && i > x + 1u) ? i : x + 1u;
}

// what a lane walks of string id: where it begins, and its length.  A string longer than max_len is refused by the entry -- the
// counting pass raises the flag for it -- and walked up to max_len, which is what the store has room for.
template <bool EMIT>
__device__ __forceinline__ uint32_t mem_lane_string(const StringSet& strings, const uint64_t id, const uint32_t max_len, uint32_t* const too_long, uint64_t& pbegin)
{
    pbegin = strings.begin[id];
    uint32_t len = strings.length ? strings.length[id] : strings.fixed_length;
    if (len > max_len)
    {
        if (!EMIT) *too_long = 1u;
        len = max_len;
    }
    return len;
}

template <bool EMIT>
__global__ void __launch_bounds__(256)
fm_mem_kernel(const Fmi f, const Fmi r, const StringSet strings, const uint32_t n, const uint32_t max_len,
              const uint32_t min_intv, const uint32_t max_intv, const uint32_t min_span,
              uint32_t* __restrict__ store, uint64_t* __restrict__ counts, const uint64_t* __restrict__ index,
              uint4* __restrict__ out, uint64_t* __restrict__ sizes, const uint64_t capacity, uint32_t* __restrict__ too_long)
{
    const uint32_t tid  = blockIdx.x * 256u + threadIdx.x;
    uint32_t* const st  = store + size_t(tid >> 6) * max_len * 192u + (tid & 63u);        // entry j, word w: st[(j * 3 + w) * 64]
    for (uint64_t id = tid; id < n; id += uint64_t(gridDim.x) * 256u)
    {
        uint64_t pbegin;
        const uint32_t len = mem_lane_string<EMIT>(strings, id, max_len, too_long, pbegin);
        const uint64_t base = EMIT ? index[id] : 0ull;
        uint32_t count = 0;
        PatternCursor pc; pc.g0 = 0xFFFFFFFFu; pc.grp = 0;

        auto report = [&](const uint2 g, const uint32_t b, const uint32_t e)
        {
            const uint32_t size = g.y - g.x + 1u;
            if (e - b < min_span || size > max_intv) return;
            if (EMIT)
            {
                const uint64_t at = base + count;
                if (at < capacity) { out[at] = make_uint4(g.x, g.y, uint32_t(id), b | (e << 16)); sizes[at] = size; }
            }
            ++count;
        };

        for (uint32_t x = 0; x < len;) x = mem_group(f, r, strings, pbegin, pc, len, x, min_intv, st, report);
        if (!EMIT) counts[id] = count;
    }
}

// ---- re-seeding (split_len / split_width).  A reported MEM [b, e) that is at least split_len long and occurs at
// most split_width times is a candidate; its re-seeds are the (occ + 1)-SMEMs that cover its midpoint, which is one group of the walk
// above (mem_group): from x = (b + e) >> 1, right on the reverse index at the larger threshold, then left from x - 1 for every kept
// range -- and no advance of x.
//
// Work shape: the persistent lane that ranks a string re-seeds its candidates the moment it reports them, so the re-seed's pattern
// words and the first records of both walks are the ones the lane has just read.  The kept ranges of the re-seed need a second
// lane-interleaved scratch area of max_len entries, because the base group's are still being consumed when a span is reported.
// The union is made per lane inside the string's own segment of a staging table (caller's temp): every span is inserted at its
// place by (begin, end), from the back -- the base MEMs arrive in order, a re-seed lands next to its candidate -- and a span that
// is already there is dropped.  The first pass counts the spans before duplicates are removed; that count sizes the segments and
// is what the entry reports when the capacity is too small.  A last kernel moves the kept records to their final places.

// begin, then end, of a record's span word (begin | end << 16) as one ordered key
__device__ __forceinline__ uint32_t span_key(const uint32_t w) { return (w << 16) | (w >> 16); }

template <bool EMIT>
__global__ void __launch_bounds__(256)
fm_mem_split_kernel(const Fmi f, const Fmi r, const StringSet strings, const uint32_t n, const uint32_t max_len,
                    const uint32_t min_intv, const uint32_t max_intv, const uint32_t min_span, const uint32_t split_len, const uint32_t split_width,
                    uint32_t* __restrict__ store, uint64_t* __restrict__ raw_counts, const uint64_t* __restrict__ raw_index,
                    uint4* __restrict__ staging, uint64_t* __restrict__ kept_counts, uint32_t* __restrict__ too_long)
{
    const uint32_t tid  = blockIdx.x * 256u + threadIdx.x;
    uint32_t* const st  = store + size_t(tid >> 6) * max_len * 384u + (tid & 63u);        // the base group's entries, then the re-seed's
    uint32_t* const st2 = st + size_t(max_len) * 192u;
    for (uint64_t id = tid; id < n; id += uint64_t(gridDim.x) * 256u)
    {
        uint64_t pbegin;
        const uint32_t len = mem_lane_string<EMIT>(strings, id, max_len, too_long, pbegin);
        uint4* const seg = EMIT ? staging + raw_index[id] : nullptr;       // room for every span counted by the first pass
        uint32_t raw = 0, kept = 0;
        PatternCursor pc; pc.g0 = 0xFFFFFFFFu; pc.grp = 0;

        auto emit = [&](const uint2 g, const uint32_t b, const uint32_t e)
        {
            ++raw;
            if (!EMIT) return;
            const uint32_t w = b | (e << 16), key = span_key(w);
            uint32_t p = kept;
            for (; p > 0u; --p)
            {
                const uint32_t other = span_key(seg[p - 1u].w);
                if (other == key) return;              // found before, by the base walk or through another candidate
                if (other < key) break;
            }
            for (uint32_t q = kept; q > p; --q) seg[q] = seg[q - 1u];
            seg[p] = make_uint4(g.x, g.y, uint32_t(id), w);
            ++kept;
        };
        auto reseed = [&](const uint2 g, const uint32_t b, const uint32_t e)
        {
            if (e - b < min_span || g.y - g.x + 1u > max_intv) return;
            emit(g, b, e);
        };
        auto base = [&](const uint2 g, const uint32_t b, const uint32_t e)
        {
            const uint32_t occ = g.y - g.x + 1u;
            if (e - b < min_span || occ > max_intv) return;
            emit(g, b, e);
            if (e - b < split_len || occ > split_width) return;
            const uint32_t k = occ == 0xFFFFFFFFu ? occ : occ + 1u;       // cannot wrap
            (void)mem_group(f, r, strings, pbegin, pc, len, (b + e) >> 1, k, st2, reseed);
        };
        for (uint32_t x = 0; x < len;) x = mem_group(f, r, strings, pbegin, pc, len, x, min_intv, st, base);

        if (!EMIT) raw_counts[id] = raw;
        else
        {
            for (uint32_t q = kept; q < raw; ++q) seg[q] = make_uint4(0u, 0u, uint32_t(id), 0u);      // the compaction reads every slot's string
            kept_counts[id] = kept;
        }
    }
}

// one thread per staged slot: the first out_index[id + 1] - out_index[id] slots of string id's segment are its records
__global__ void __launch_bounds__(256)
fm_mem_compact_kernel(const uint4* __restrict__ staging, const uint64_t* __restrict__ raw_index, const uint64_t* __restrict__ out_index,
                      const uint64_t n_raw, uint4* __restrict__ out, uint64_t* __restrict__ sizes)
{
    const uint64_t t = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    if (t >= n_raw) return;
    const uint4 rec = staging[t];
    const uint64_t first = out_index[rec.z], pos = t - raw_index[rec.z];
    if (pos >= out_index[rec.z + 1u] - first) return;
    out[first + pos] = rec; sizes[first + pos] = rec.y - rec.x + 1u;
}

__global__ void __launch_bounds__(256)
fm_mem_locate_kernel(const Fmi f, const uint4* __restrict__ ranges, const uint64_t* __restrict__ slots,
                     const uint64_t n_ranges, const uint64_t begin, const uint64_t count, uint4* __restrict__ hits)
{
    const uint64_t id = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    if (id >= count) return;
    const uint64_t h = begin + id;
    uint64_t lo = 0, hi = n_ranges;           // upper_bound(slots, h)
    while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if (slots[mid] <= h) lo = mid + 1; else hi = mid; }
    if (lo >= n_ranges) { hits[id] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u); return; }     // h past the last hit
    const uint4 rg = ranges[lo];
    const uint64_t first = lo ? slots[lo - 1] : 0ull;
    const uint2 it = fm_locate_it(f, rg.x + uint32_t(h - first));
    hits[id] = make_uint4(f.ssa[it.x / f.sa_int] + it.y, rg.z & 0x7FFFFFFFu, rg.w & 0xFFFFu, rg.w >> 16);
}

__global__ void __launch_bounds__(256)
fm_extend_kernel(const int32_t direction, const Fmi f, const Fmi r, const uint2* __restrict__ f_ranges, const uint2* __restrict__ r_ranges,
                 const uint8_t* __restrict__ c, const uint32_t n, uint2* __restrict__ out_f, uint2* __restrict__ out_r)
{
    const uint32_t id = blockIdx.x * 256u + threadIdx.x;
    if (id >= n) return;
    uint2 fr = f_ranges[id], rr = r_ranges[id];
    const uint32_t sym = c[id];
    if (sym > 3u) { fr = make_uint2(1u, 0u); rr = make_uint2(1u, 0u); }
    else if (direction == 0) fm_extend_forward(r, fr, rr, sym);
    else                     fm_extend_backwards(f, fr, rr, sym);
    out_f[id] = fr; out_r[id] = rr;
}

static inline uint64_t mem_align256(uint64_t x) { return (x + 255ull) & ~255ull; }
static inline uint32_t mem_blocks(uint32_t n) { const uint64_t b = (uint64_t(n) + 255u) / 256u; return uint32_t(b < MEM_MAX_BLOCKS ? b : MEM_MAX_BLOCKS); }

// The temp of a rank entry, in this order.  The plain entry (split == false) has neither raw_index nor staging, and half the store.
struct MemTemp {
    uint32_t* store;        // the kept ranges of the lanes in flight: max_len entries a lane, and as many again for the re-seeds
    uint64_t* counts;       // n counts (split: before, then after, the duplicates go), then 256 bytes that hold
    uint32_t* too_long;     //   the flag of a string longer than max_len
    uint64_t* raw_index;    // split: the n + 1 segment bounds of the staging table
    void*     scan;         // hipCUB's: n counts, then the sizes of the stored records
    size_t    scan_bytes;
    uint4*    staging;      // split: at most `capacity` records (never more than 2^31 - 1)
    uint64_t  bytes;        // all of it; the split entry runs the plain one for the no-split sentinel, so never less than the plain layout
};
// a null `temp` gives the sizes alone
static MemTemp mem_temp_carve(void* temp, const uint32_t n, const uint32_t max_len, const bool split, const uint64_t capacity)
{
    const uint64_t staged = std::min<uint64_t>(capacity, 0x7FFFFFFFull);
    const uint64_t most   = split ? std::max<uint64_t>(staged, n) : std::max<uint64_t>(std::min<uint64_t>(uint64_t(n) * max_len, 0x7FFFFFFFull), n);
    size_t scan = 0;
    (void)hipcub::DeviceScan::InclusiveSum(nullptr, scan, (const uint64_t*)nullptr, (uint64_t*)nullptr, int(most));      // size query only

    uintptr_t p = reinterpret_cast<uintptr_t>(temp);
    auto take = [&p](const uint64_t bytes) { const uintptr_t at = p; p += bytes; return at; };
    MemTemp t;
    t.store      = reinterpret_cast<uint32_t*>(take((split ? 2u : 1u) * mem_align256(uint64_t(mem_blocks(n)) * 256u * max_len * 12u)));
    t.counts     = reinterpret_cast<uint64_t*>(take(mem_align256(uint64_t(n) * 8u) + 256u));
    t.too_long   = reinterpret_cast<uint32_t*>(p - 256u);
    t.raw_index  = reinterpret_cast<uint64_t*>(take(split ? mem_align256((uint64_t(n) + 1u) * 8u) : 0u));
    t.scan_bytes = size_t(mem_align256(scan) + 256u);
    t.scan       = reinterpret_cast<void*>(take(t.scan_bytes));
    t.staging    = reinterpret_cast<uint4*>(take(split ? mem_align256(staged * 16u) : 0u));
    t.bytes      = uint64_t(p - reinterpret_cast<uintptr_t>(temp));
    if (split) t.bytes = std::max<uint64_t>(t.bytes, mem_temp_carve(nullptr, n, max_len, false, 0u).bytes);
    return t;
}
// what the size queries answer: 256 for a shape the entries refuse or have nothing to do for
static uint64_t mem_temp_bytes(const uint32_t n, const uint32_t max_len, const bool split, const uint64_t capacity)
{
    if (n == 0 || max_len == 0 || max_len > 65535u || n >= 0x80000000u) return 256u;
    return mem_temp_carve(nullptr, n, max_len, split, capacity).bytes;
}

// The first pass of both entries: count() launches the <false> kernel on t.counts and t.too_long, the counts are scanned into
// index + 1, and the total comes back with the flag.  Synchronises the stream; refuses a batch that holds a string longer than
// max_pattern_len.
template <typename Count>
static int mem_count_pass(MemTemp& t, const uint32_t n, uint64_t* out_index, uint64_t* index, hipStream_t s, Count&& count, uint64_t& total)
{
    if (hipError_t e = hipMemsetAsync(out_index, 0, 8u, s)) return e;
    if (index != out_index) if (hipError_t e = hipMemsetAsync(index, 0, 8u, s)) return e;
    if (hipError_t e = hipMemsetAsync(t.too_long, 0, 4u, s)) return e;
    count();
    if (hipError_t e = hipGetLastError()) return e;
    if (hipError_t e = hipcub::DeviceScan::InclusiveSum(t.scan, t.scan_bytes, t.counts, index + 1, int(n), s)) return e;
    uint32_t refused = 0;
    if (hipError_t e = hipMemcpyAsync(&total, index + n, 8u, hipMemcpyDeviceToHost, s)) return e;
    if (hipError_t e = hipMemcpyAsync(&refused, t.too_long, 4u, hipMemcpyDeviceToHost, s)) return e;
    if (hipError_t e = hipStreamSynchronize(s)) return e;
    return refused ? hipErrorInvalidValue : hipSuccess;
}

} // namespace nvb

using namespace nvb;

static int check_bidir(const nvbio_hip_fmindex* f, const nvbio_hip_fmindex* r)
{
    if (!f || !r || !f->bwt_occ || !r->bwt_occ || f->length != r->length) return hipErrorInvalidValue;
    return hipSuccess;
}

NVB_API int nvbio_hip_fm_extend(int32_t direction, const nvbio_hip_fmindex* f_fmi, const nvbio_hip_fmindex* r_fmi,
                                const uint32_t* f_ranges, const uint32_t* r_ranges, const uint8_t* c, uint32_t n,
                                uint32_t* out_f_ranges, uint32_t* out_r_ranges, void* stream)
{
    if (int e = check_bidir(f_fmi, r_fmi)) return e;
    if (direction != NVBIO_HIP_EXTEND_FORWARD && direction != NVBIO_HIP_EXTEND_BACKWARDS) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    if (!f_ranges || !r_ranges || !c || !out_f_ranges || !out_r_ranges) return hipErrorInvalidValue;
    g_last_kernel = "fm_extend_kernel";
    hipLaunchKernelGGL(fm_extend_kernel, dim3((n + 255u) / 256u), dim3(256), 0, to_stream(stream), direction, make_fmi(f_fmi), make_fmi(r_fmi),
                       reinterpret_cast<const uint2*>(f_ranges), reinterpret_cast<const uint2*>(r_ranges), c, n,
                       reinterpret_cast<uint2*>(out_f_ranges), reinterpret_cast<uint2*>(out_r_ranges));
    return hipGetLastError();
}

NVB_API uint64_t nvbio_hip_fm_mem_temp_bytes(uint32_t n, uint32_t max_pattern_len) { return mem_temp_bytes(n, max_pattern_len, false, 0u); }

NVB_API int nvbio_hip_fm_mem_rank(const nvbio_hip_fmindex* f_fmi, const nvbio_hip_fmindex* r_fmi, const nvbio_hip_string_set* strings,
                                  uint32_t n, uint32_t max_pattern_len, uint32_t min_intv, uint32_t max_intv, uint32_t min_span,
                                  uint32_t* out_ranges, uint64_t capacity, uint64_t* out_index, uint64_t* out_slots, uint64_t* out_n_ranges,
                                  void* temp, uint64_t temp_bytes, void* stream)
{
    hipStream_t s = to_stream(stream);
    const int admitted = mem_rank_admission(f_fmi, r_fmi, strings, n, max_pattern_len, min_intv, out_ranges, capacity, out_index, out_slots, out_n_ranges, [] {});
    if (admitted == MEM_ARGS_EMPTY) return hipMemsetAsync(out_index, 0, (uint64_t(n) + 1u) * 8u, s);
    if (admitted != MEM_ARGS_GO) return admitted;
    MemTemp t = mem_temp_carve(temp, n, max_pattern_len, false, 0u);
    if (!temp || temp_bytes < t.bytes) return hipErrorInvalidValue;
    const dim3 grid(mem_blocks(n)), block(256);
    const Fmi f = make_fmi(f_fmi), r = make_fmi(r_fmi);
    const StringSet set = make_string_set(strings);

    g_last_kernel = "fm_mem_kernel";
    uint64_t total = 0;
    if (int e = mem_count_pass(t, n, out_index, out_index, s, [&] {
            hipLaunchKernelGGL(fm_mem_kernel<false>, grid, block, 0, s, f, r, set, n, max_pattern_len, min_intv, max_intv, min_span,
                               t.store, t.counts, (const uint64_t*)nullptr, (uint4*)nullptr, (uint64_t*)nullptr, 0ull, t.too_long); }, total)) return e;
    *out_n_ranges = total;
    const uint64_t stored = total < capacity ? total : capacity;
    if (stored > 0x7FFFFFFFull) return hipErrorInvalidValue;           // the scan below counts in 31 bits
    if (stored)
    {
        hipLaunchKernelGGL(fm_mem_kernel<true>, grid, block, 0, s, f, r, set, n, max_pattern_len, min_intv, max_intv, min_span,
                           t.store, t.counts, out_index, reinterpret_cast<uint4*>(out_ranges), out_slots, capacity, (uint32_t*)nullptr);
        if (hipError_t e = hipGetLastError()) return e;
        if (hipError_t e = hipcub::DeviceScan::InclusiveSum(t.scan, t.scan_bytes, out_slots, out_slots, int(stored), s)) return e;
    }
    return total > capacity ? NVBIO_HIP_ERROR_CAPACITY : hipSuccess;
}

NVB_API uint64_t nvbio_hip_fm_mem_split_temp_bytes(uint32_t n, uint32_t max_pattern_len, uint64_t capacity) { return mem_temp_bytes(n, max_pattern_len, true, capacity); }

NVB_API int nvbio_hip_fm_mem_rank_split(const nvbio_hip_fmindex* f_fmi, const nvbio_hip_fmindex* r_fmi, const nvbio_hip_string_set* strings,
                                        uint32_t n, uint32_t max_pattern_len, uint32_t min_intv, uint32_t max_intv, uint32_t min_span,
                                        uint32_t split_len, uint32_t split_width,
                                        uint32_t* out_ranges, uint64_t capacity, uint64_t* out_index, uint64_t* out_slots, uint64_t* out_n_ranges,
                                        void* temp, uint64_t temp_bytes, void* stream)
{
    if (split_len == 0xFFFFFFFFu)                      // no re-seeding: the plain entry, word for word
        return nvbio_hip_fm_mem_rank(f_fmi, r_fmi, strings, n, max_pattern_len, min_intv, max_intv, min_span, out_ranges, capacity, out_index, out_slots,
                                     out_n_ranges, temp, temp_bytes, stream);
    hipStream_t s = to_stream(stream);
    const int admitted = mem_rank_admission(f_fmi, r_fmi, strings, n, max_pattern_len, min_intv, out_ranges, capacity, out_index, out_slots, out_n_ranges, [] {});
    if (admitted == MEM_ARGS_EMPTY) return hipMemsetAsync(out_index, 0, (uint64_t(n) + 1u) * 8u, s);
    if (admitted != MEM_ARGS_GO) return admitted;
    MemTemp t = mem_temp_carve(temp, n, max_pattern_len, true, capacity);
    if (!temp || temp_bytes < t.bytes) return hipErrorInvalidValue;
    const dim3 grid(mem_blocks(n)), block(256);
    const Fmi f = make_fmi(f_fmi), r = make_fmi(r_fmi);
    const StringSet set = make_string_set(strings);

    g_last_kernel = "fm_mem_split_kernel";
    uint64_t raw = 0, total = 0;
    if (int e = mem_count_pass(t, n, out_index, t.raw_index, s, [&] {
            hipLaunchKernelGGL(fm_mem_split_kernel<false>, grid, block, 0, s, f, r, set, n, max_pattern_len, min_intv, max_intv, min_span, split_len, split_width,
                               t.store, t.counts, (const uint64_t*)nullptr, (uint4*)nullptr, (uint64_t*)nullptr, t.too_long); }, raw)) return e;
    if (raw > capacity) { *out_n_ranges = raw; return NVBIO_HIP_ERROR_CAPACITY; }       // the staging table has room for `capacity` spans
    if (raw > 0x7FFFFFFFull) return hipErrorInvalidValue;              // the scans count in 31 bits
    if (raw == 0) return hipMemsetAsync(out_index, 0, (uint64_t(n) + 1u) * 8u, s);

    hipLaunchKernelGGL(fm_mem_split_kernel<true>, grid, block, 0, s, f, r, set, n, max_pattern_len, min_intv, max_intv, min_span, split_len, split_width,
                       t.store, (uint64_t*)nullptr, t.raw_index, t.staging, t.counts, (uint32_t*)nullptr);
    if (hipError_t e = hipGetLastError()) return e;
    if (hipError_t e = hipcub::DeviceScan::InclusiveSum(t.scan, t.scan_bytes, t.counts, out_index + 1, int(n), s)) return e;
    hipLaunchKernelGGL(fm_mem_compact_kernel, dim3(uint32_t((raw + 255u) / 256u)), block, 0, s, t.staging, t.raw_index, out_index, raw,
                       reinterpret_cast<uint4*>(out_ranges), out_slots);
    if (hipError_t e = hipGetLastError()) return e;
    if (hipError_t e = hipMemcpyAsync(&total, out_index + n, 8u, hipMemcpyDeviceToHost, s)) return e;
    if (hipError_t e = hipStreamSynchronize(s)) return e;
    if (hipError_t e = hipcub::DeviceScan::InclusiveSum(t.scan, t.scan_bytes, out_slots, out_slots, int(total), s)) return e;
    *out_n_ranges = total;
    return hipSuccess;
}

NVB_API int nvbio_hip_fm_mem_locate(const nvbio_hip_fmindex* f_fmi, const uint32_t* ranges, const uint64_t* slots, uint64_t n_ranges,
                                    uint64_t begin, uint64_t end, uint32_t* out_hits, void* stream)
{
    if (!f_fmi || !f_fmi->bwt_occ || !f_fmi->ssa || f_fmi->sa_int == 0 || (f_fmi->sa_int & (f_fmi->sa_int - 1)) != 0) return hipErrorInvalidValue;
    if (end < begin) return hipErrorInvalidValue;
    if (end == begin) return hipSuccess;
    if (!ranges || !slots || !out_hits || n_ranges == 0) return hipErrorInvalidValue;
    if (end - begin > 0xFFFFFF00ull * 256ull) return hipErrorInvalidValue;
    g_last_kernel = "fm_mem_locate_kernel";
    hipLaunchKernelGGL(fm_mem_locate_kernel, dim3(uint32_t((end - begin + 255u) / 256u)), dim3(256), 0, to_stream(stream), make_fmi(f_fmi),
                       reinterpret_cast<const uint4*>(ranges), slots, n_ranges, begin, end - begin, reinterpret_cast<uint4*>(out_hits));
    return hipGetLastError();
}
