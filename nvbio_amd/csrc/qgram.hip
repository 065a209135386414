// qgram.hip -- q-gram indices over 2-bit strings and string sets, and the q-gram filter (rank / locate / merge): the reference's
// nvbio/qgram (QGramIndexDevice, QGramSetIndexDevice, generate_qgrams, QGramFilterDevice).  DESIGN.md 3.14.
//
// A q-gram is the 64-bit word sum_j sym(i + j) << 2j, j < q, the first symbol lowest and symbols past the string's end 0.  A
// little-endian 2-bit stream already has that bit order; a big-endian word has its 2-bit fields reversed first (rev2), so every kernel
// below works on "canonical" words and a q-gram is a funnel shift of two or three of them and a mask.
//
// Build: keys | sort (rocPRIM radix sort over 2q bits, stable, so the coordinates of one q-gram stay in enumeration order) | run-length
// encode | exclusive scan of the counts | one lower bound per LUT key.
// Scratch of a build over n q-grams: keys A (8 n) | keys B (8 n) | coordinates (4 n; 8 n for a set) | counts (4 n) | the run count
// (256) | for a set: cum, the 64-bit inclusive sums of the per-string seed counts (8 N) | rocPRIM's.
// Scratch of rank: rocPRIM's scan only.  Scratch of merge: keys A | keys B (4 n each; 8 n for a set) | the run count (256) | rocPRIM's.
#include "common.h"
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
#include <algorithm>

namespace nvb {

static constexpr uint64_t QG_MAX_N = 0xFFFFFFFFull;     // coordinates, slots and ranges are 32-bit words

static inline uint64_t qg_align(uint64_t x) { return (x + 255ull) & ~255ull; }
static inline uint32_t qg_blocks(uint64_t items, uint32_t per_block = 256u) { return uint32_t((items + per_block - 1u) / per_block); }

// word w of the stream in canonical order, the load clamped to [0, n_words)
__device__ __forceinline__ uint32_t qg_word(const uint32_t* __restrict__ words, const uint64_t w, const uint64_t n_words, const uint32_t be)
{
    const uint32_t x = words[w < n_words ? w : n_words - 1u];
    return be ? rev2(x) : x;
}

// the low 2 * symbols bits, symbols in [0, 32]
__device__ __forceinline__ uint64_t qg_mask(const uint32_t symbols) { return symbols >= 32u ? ~0ull : ((1ull << (2u * symbols)) - 1ull); }

// the q-gram at position pos of the string [begin, begin + len) of the stream: three words, two funnel shifts, one mask
__device__ __forceinline__ uint64_t qg_at(const uint32_t* __restrict__ words, const uint64_t n_words, const uint32_t be, const uint64_t begin,
                                          const uint64_t len, const uint64_t pos, const uint32_t q)
{
    if (pos >= len) return 0ull;
    const uint64_t p = begin + pos, w = p >> 4;
    const uint32_t sh = 2u * uint32_t(p & 15u);
    const uint32_t w0 = qg_word(words, w, n_words, be), w1 = qg_word(words, w + 1u, n_words, be), w2 = qg_word(words, w + 2u, n_words, be);
    const uint64_t v = (uint64_t(funnel(w1, w2, sh)) << 32) | funnel(w0, w1, sh);
    const uint64_t rem = len - pos;
    return v & qg_mask(rem < q ? uint32_t(rem) : q);
}

// Every position of one string that starts at symbol 0 of the stream.  A lane takes the 16 positions of one word: it loads that word
// and the two after it once, and slides a 64-bit window over the 96 bits two bits a position -- nothing is read per symbol.
// ids (may be NULL) gets 0 .. n - 1, the coordinates of a string index.
__global__ __launch_bounds__(256) void qgram_generate_kernel(const uint32_t* __restrict__ words, const uint64_t n_words, const uint32_t be, const uint64_t len,
                                                             const uint32_t q, const uint64_t n, uint64_t* __restrict__ qgrams, uint32_t* __restrict__ ids)
{
    const uint64_t t = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    const uint64_t i0 = t * 16u;
    if (i0 >= n) return;
    uint64_t win = (uint64_t(qg_word(words, t + 1u, n_words, be)) << 32) | qg_word(words, t, n_words, be);
    uint32_t next = qg_word(words, t + 2u, n_words, be);
    const uint64_t full = qg_mask(q);
    #pragma unroll
    for (uint32_t k = 0; k < 16u; ++k)
    {
        const uint64_t i = i0 + k;
        if (i < n)
        {
            uint64_t g = 0ull;
            if (i < len)
            {
                const uint64_t rem = len - i;
                g = win & (rem < q ? qg_mask(uint32_t(rem)) : full);
            }
            qgrams[i] = g;
            if (ids) ids[i] = uint32_t(i);
        }
        win = (win >> 2) | (uint64_t(next & 3u) << 62);
        next >>= 2;
    }
}

// The coordinate-list form.  SET: coords holds (string id, position) pairs and the string comes from the set's arrays (an id that is
// not below n_strings selects nothing: q-gram 0); otherwise coords holds positions of the one string [0, len).
template <bool SET>
__global__ __launch_bounds__(256) void qgram_generate_coords_kernel(const uint32_t* __restrict__ words, const uint64_t n_words, const uint32_t be,
                                                                    const uint64_t* __restrict__ begin, const uint32_t* __restrict__ length,
                                                                    const uint32_t fixed_length, const uint32_t n_strings, const uint64_t len,
                                                                    const uint32_t q, const uint32_t* __restrict__ coords, const uint64_t n,
                                                                    uint64_t* __restrict__ qgrams)
{
    const uint64_t i = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    if (i >= n) return;
    if (SET)
    {
        const uint32_t id = coords[2u * i], pos = coords[2u * i + 1u];
        qgrams[i] = id < n_strings ? qg_at(words, n_words, be, begin[id], length ? length[id] : fixed_length, pos, q) : 0ull;
    }
    else
        qgrams[i] = qg_at(words, n_words, be, 0u, len, coords[i], q);
}

// seeds of a string under uniform_seeds_functor(q, interval): positions 0, interval, .. while pos + q <= length
__host__ __device__ __forceinline__ uint64_t qg_seed_count(const uint32_t len, const uint32_t q, const uint32_t interval)
{
    return len >= q ? uint64_t(len - q) / interval + 1u : 0u;
}

__global__ __launch_bounds__(256) void qgram_seed_counts_kernel(const uint32_t* __restrict__ length, const uint32_t fixed_length, const uint32_t n_strings,
                                                                const uint32_t q, const uint32_t interval, uint64_t* __restrict__ counts)
{
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= n_strings) return;
    counts[s] = qg_seed_count(length ? length[s] : fixed_length, q, interval);
}

// Seed o of the set, in (string, position) order: its string by one upper bound in the inclusive sums (a division where the lengths are
// fixed), its q-gram and its coordinate.  Nothing is written unless the sums end at n, the count the caller's buffers were sized for.
__global__ __launch_bounds__(256) void qgram_set_seeds_kernel(const uint32_t* __restrict__ words, const uint64_t n_words, const uint32_t be,
                                                              const uint64_t* __restrict__ begin, const uint32_t* __restrict__ length,
                                                              const uint32_t fixed_length, const uint32_t n_strings, const uint64_t* __restrict__ cum,
                                                              const uint32_t q, const uint32_t interval, const uint64_t n,
                                                              uint64_t* __restrict__ qgrams, uint64_t* __restrict__ coords)
{
    const uint64_t o = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    if (o >= n) return;
    uint32_t s;
    uint64_t pos;
    if (length)
    {
        if (cum[n_strings - 1u] != n) return;
        uint32_t lo = 0u, hi = n_strings;
        while (lo < hi)
        {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (cum[mid] <= o) lo = mid + 1u; else hi = mid;
        }
        s = lo;                                                       // < n_strings, because o < cum[n_strings - 1]
        pos = (o - (s ? cum[s - 1u] : 0ull)) * interval;
    }
    else                                                              // every string has the same seeds: no sums are needed (cum is not set)
    {
        const uint64_t per = n / n_strings;                           // the host has checked n == n_strings * per
        s = uint32_t(o / per);
        pos = (o % per) * interval;
    }
    qgrams[o] = qg_at(words, n_words, be, begin[s], length ? length[s] : fixed_length, pos, q);
    coords[o] = (pos << 32) | s;                                      // the uint2 (string id, position)
}

__device__ __forceinline__ uint32_t qg_lower_bound(const uint64_t* __restrict__ a, uint32_t lo, uint32_t hi, const uint64_t g)
{
    while (lo < hi)
    {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (a[mid] < g) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// slots[n_unique] = n, and the LUT: lut[k] = the lower bound of k << QLS among the distinct q-grams, lut[4^QL] = n_unique
__global__ __launch_bounds__(256) void qgram_lut_kernel(const uint64_t* __restrict__ qgrams, const uint32_t n_unique, const uint32_t n, const uint32_t q,
                                                        const uint32_t ql, uint32_t* __restrict__ slots, uint32_t* __restrict__ lut)
{
    const uint64_t k = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    if (k == 0u) slots[n_unique] = n;
    if (ql == 0u) return;
    const uint64_t n_keys = 1ull << (2u * ql);
    if (k > n_keys) return;
    lut[k] = k == n_keys ? n_unique : qg_lower_bound(qgrams, 0u, n_unique, k << (2u * (q - ql)));
}

struct QgView
{
    const uint64_t* qgrams;
    const uint32_t* slots;
    const uint32_t* lut;
    uint32_t q, ql, n_unique;
};

// the slots of q-gram g: the LUT's bucket if there is one, a lower bound inside it, two slot reads
__device__ __forceinline__ uint2 qg_range(const QgView& v, const uint64_t g)
{
    if (v.q < 32u && (g >> (2u * v.q))) return make_uint2(0u, 0u);     // no q symbols make this word; it would index past the LUT too
    uint32_t lo = 0u, hi = v.n_unique;
    if (v.ql)                                                         // with QL == 0 the shift, 64 bits at q == 32, is never evaluated
    {
        const uint64_t k = g >> (2u * (v.q - v.ql));
        lo = v.lut[k]; hi = v.lut[k + 1u];
    }
    const uint32_t i = qg_lower_bound(v.qgrams, lo, hi, g);
    if (i >= v.n_unique || v.qgrams[i] != g) return make_uint2(0u, 0u);
    return make_uint2(v.slots[i], v.slots[i + 1u]);
}

__global__ __launch_bounds__(256) void qgram_range_kernel(const QgView v, const uint64_t* __restrict__ queries, const uint64_t n, uint2* __restrict__ ranges)
{
    const uint64_t i = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    if (i >= n) return;
    ranges[i] = qg_range(v, queries[i]);
}

struct qg_range_size
{
    __host__ __device__ uint64_t operator()(const uint2 r) const { return uint64_t(r.y - r.x); }
};
typedef rocprim::transform_iterator<const uint2*, qg_range_size, uint64_t> qg_size_iterator;

__device__ __forceinline__ uint32_t qg_upper_bound(const uint64_t* __restrict__ a, uint32_t lo, uint32_t hi, const uint64_t o)
{
    while (lo < hi)
    {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (a[mid] <= o) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// Hits [begin, end) of the ranked queries.  A block covers 1024 consecutive outputs: two lanes find the slots of its first and of its
// last output by a search over all the queries, and every output then searches only between those two, which are a few queries apart
// unless the ranges are tiny.  The upper bound is the same number whatever interval it is taken in, so the output does not depend on
// the tiling.  An output at or past the total, or a range that leaves the index, gives a zero hit.
template <bool SET>
__global__ __launch_bounds__(256) void qgram_locate_kernel(const uint32_t* __restrict__ index, const uint32_t n_qgrams, const uint32_t n_queries,
                                                           const uint2* __restrict__ ranges, const uint64_t* __restrict__ slots,
                                                           const uint32_t* __restrict__ indices, const uint64_t begin, const uint64_t end,
                                                           uint32_t* __restrict__ hits)
{
    __shared__ uint32_t s_bounds[2];
    const uint64_t o0 = begin + uint64_t(blockIdx.x) * 1024u;
    const uint64_t o1 = o0 + 1024u < end ? o0 + 1024u : end;          // this block's outputs: [o0, o1), not empty
    if (threadIdx.x < 2u)
        s_bounds[threadIdx.x] = qg_upper_bound(slots, 0u, n_queries, threadIdx.x ? o1 - 1u : o0);
    __syncthreads();
    const uint32_t s_lo = s_bounds[0], s_hi = s_bounds[1];
    #pragma unroll
    for (uint32_t k = 0; k < 4u; ++k)
    {
        const uint64_t o = o0 + k * 256u + threadIdx.x;
        if (o >= o1) continue;
        const uint32_t slot = qg_upper_bound(slots, s_lo, s_hi, o);
        uint32_t h0 = 0u, h1 = 0u, h2 = 0u;
        if (slot < n_queries)
        {
            const uint64_t at = uint64_t(ranges[slot].x) + (o - (slot ? slots[slot - 1u] : 0ull));       // 64 bits in both forms
            if (at < n_qgrams)
            {
                if (SET) { h0 = index[2u * at]; h1 = index[2u * at + 1u]; h2 = indices[slot]; }
                else     { h0 = index[at]; h1 = indices[slot]; }
            }
        }
        const uint64_t out = o - begin;
        if (SET) reinterpret_cast<uint4*>(hits)[out] = make_uint4(h0, h1, h2, 0u);
        else     reinterpret_cast<uint2*>(hits)[out] = make_uint2(h0, h1);
    }
}

// the reference's util::round(diag, interval) as it is written: the multiple of interval at or below diag, plus ONE where the
// remainder is more than half the interval
__host__ __device__ __forceinline__ uint32_t qg_snap(const uint32_t diag, const uint32_t interval)
{
    const uint32_t r = (diag / interval) * interval;
    return uint32_t((diag - r) * 2u) > interval ? r + 1u : r;
}

// string index: hit (index pos, query idx) -> the snapped diagonal query idx - index pos
__global__ __launch_bounds__(256) void qgram_diagonals_kernel(const uint2* __restrict__ hits, const uint32_t n, const uint32_t interval, uint32_t* __restrict__ keys)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint2 h = hits[i];
    keys[i] = qg_snap(h.y - h.x, interval);
}

// set index: hit (string id, pos, query idx, 0) -> (snapped diagonal, string id), the string id in the high half of the sort word
__global__ __launch_bounds__(256) void qgram_set_diagonals_kernel(const uint4* __restrict__ hits, const uint32_t n, const uint32_t interval, uint64_t* __restrict__ keys)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint4 h = hits[i];
    keys[i] = (uint64_t(h.x) << 32) | qg_snap(h.z - h.y, interval);
}

// ---- host side ----

template <typename V>
static uint64_t qg_build_prim_bytes(uint64_t n, uint64_t n_strings)
{
    size_t sort = 0, rle = 0, scan = 0, cum = 0;
    (void)rocprim::radix_sort_pairs(nullptr, sort, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const V*)nullptr, (V*)nullptr, size_t(n), 0u, 64u);
    (void)rocprim::run_length_encode(nullptr, rle, (const uint64_t*)nullptr, size_t(n), (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr);
    (void)rocprim::exclusive_scan(nullptr, scan, (const uint32_t*)nullptr, (uint32_t*)nullptr, 0u, size_t(n), rocprim::plus<uint32_t>());
    if (n_strings)
        (void)rocprim::inclusive_scan(nullptr, cum, (const uint64_t*)nullptr, (uint64_t*)nullptr, size_t(n_strings), rocprim::plus<uint64_t>());
    return qg_align(std::max<uint64_t>(std::max<uint64_t>(sort, rle), std::max<uint64_t>(scan, cum))) + 256u;
}

template <typename V>
static uint64_t qg_build_fixed_bytes(uint64_t n, uint64_t n_strings)
{
    return 2u * qg_align(n * 8u) + qg_align(n * sizeof(V)) + qg_align(n * 4u) + 256u + qg_align(n_strings * 8u);
}

template <typename V>
struct qg_build_arrays
{
    uint64_t *keysA, *keysB, *cum;
    V*        vals;
    uint32_t *counts, *n_runs;
    void*     prim;
    size_t    prim_bytes;
};

template <typename V>
static qg_build_arrays<V> qg_build_carve(void* temp, uint64_t temp_bytes, uint64_t n, uint64_t n_strings)
{
    qg_build_arrays<V> a;
    uint8_t* p = reinterpret_cast<uint8_t*>(temp);
    a.keysA  = reinterpret_cast<uint64_t*>(p);   p += qg_align(n * 8u);
    a.keysB  = reinterpret_cast<uint64_t*>(p);   p += qg_align(n * 8u);
    a.vals   = reinterpret_cast<V*>(p);          p += qg_align(n * sizeof(V));
    a.counts = reinterpret_cast<uint32_t*>(p);   p += qg_align(n * 4u);
    a.n_runs = reinterpret_cast<uint32_t*>(p);   p += 256u;
    a.cum    = reinterpret_cast<uint64_t*>(p);   p += qg_align(n_strings * 8u);
    a.prim = p;
    a.prim_bytes = size_t(temp_bytes - uint64_t(p - reinterpret_cast<uint8_t*>(temp)));
    return a;
}

// keysA / vals hold the n q-grams and their coordinates in enumeration order: sort, encode, scan, LUT.  Waits for the stream once, for
// the number of distinct q-grams.
template <typename V>
static int qg_build_finish(const qg_build_arrays<V>& a, uint64_t n, uint32_t q, uint32_t ql, uint64_t* qgrams_out, uint32_t* slots_out, V* index_out,
                           uint32_t* lut_out, uint32_t* n_unique_out, hipStream_t s)
{
    uint32_t n_unique = 0u;
    size_t prim_bytes = a.prim_bytes;
    if (n)
    {
        if (hipError_t e = rocprim::radix_sort_pairs(a.prim, prim_bytes, (const uint64_t*)a.keysA, a.keysB, (const V*)a.vals, index_out, size_t(n), 0u, 2u * q, s)) return e;
        if (hipError_t e = rocprim::run_length_encode(a.prim, prim_bytes, (const uint64_t*)a.keysB, size_t(n), qgrams_out, a.counts, a.n_runs, s)) return e;
        if (hipError_t e = hipMemcpyAsync(&n_unique, a.n_runs, 4u, hipMemcpyDeviceToHost, s)) return e;
        if (hipError_t e = hipStreamSynchronize(s)) return e;
        if (hipError_t e = rocprim::exclusive_scan(a.prim, prim_bytes, (const uint32_t*)a.counts, slots_out, 0u, size_t(n_unique), rocprim::plus<uint32_t>(), s)) return e;
    }
    const uint64_t lut_items = ql ? (1ull << (2u * ql)) + 1u : 1u;
    g_last_kernel = "qgram_lut_kernel";
    hipLaunchKernelGGL(qgram_lut_kernel, dim3(qg_blocks(lut_items)), dim3(256), 0, s, (const uint64_t*)qgrams_out, n_unique, uint32_t(n), q, ql, slots_out, lut_out);
    if (hipError_t e = hipGetLastError()) return e;
    *n_unique_out = n_unique;
    return hipSuccess;
}

static inline bool qg_params_ok(uint32_t bits, uint32_t q, uint32_t ql)
{
    return bits == 2u && q >= 1u && q <= 32u && ql <= (q < 16u ? q : 16u);
}

// a set of no strings needs no begin array
static inline bool qg_set_ok(const nvbio_hip_string_set* set, uint32_t n_strings)
{
    return set && set->words && set->n_words && (set->begin || n_strings == 0u) && set->bits == 2u;
}

static uint64_t qg_scan64_prim_bytes(uint64_t n)
{
    size_t b = 0;
    (void)rocprim::inclusive_scan(nullptr, b, (const uint64_t*)nullptr, (uint64_t*)nullptr, size_t(n), rocprim::plus<uint64_t>());
    return qg_align(b) + 256u;
}

// cum = the inclusive sums of the per-string seed counts; *total = their sum, brought to the host with one wait
static int qg_seed_sums(const nvbio_hip_string_set* set, uint32_t n_strings, uint32_t q, uint32_t interval, uint64_t* cum, void* prim, size_t prim_bytes,
                        uint64_t* total, hipStream_t s)
{
    *total = 0u;
    if (n_strings == 0u) return hipSuccess;
    hipLaunchKernelGGL(qgram_seed_counts_kernel, dim3(qg_blocks(n_strings)), dim3(256), 0, s, set->length, set->fixed_length, n_strings, q, interval, cum);
    if (hipError_t e = hipGetLastError()) return e;
    if (hipError_t e = rocprim::inclusive_scan(prim, prim_bytes, (const uint64_t*)cum, cum, size_t(n_strings), rocprim::plus<uint64_t>(), s)) return e;
    if (hipError_t e = hipMemcpyAsync(total, cum + (n_strings - 1u), 8u, hipMemcpyDeviceToHost, s)) return e;
    return hipStreamSynchronize(s);
}

template <typename K>
static uint64_t qg_merge_prim_bytes(uint64_t n)
{
    size_t sort = 0, rle = 0;
    (void)rocprim::radix_sort_keys(nullptr, sort, (const K*)nullptr, (K*)nullptr, size_t(n), 0u, uint32_t(8u * sizeof(K)));
    (void)rocprim::run_length_encode(nullptr, rle, (const K*)nullptr, size_t(n), (K*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr);
    return qg_align(std::max<uint64_t>(sort, rle)) + 256u;
}

template <typename K>
static uint64_t qg_merge_temp_bytes(uint64_t n) { return 2u * qg_align(n * sizeof(K)) + 256u + qg_merge_prim_bytes<K>(n); }

// keys A holds the n snapped diagonals: sort, run-length encode, one wait for the number of runs
template <typename K>
static int qg_merge_finish(K* keysA, K* keysB, uint32_t* n_runs, void* prim, size_t prim_bytes, uint32_t n, K* merged_out, uint32_t* counts_out,
                           uint32_t* n_merged_out, hipStream_t s)
{
    if (hipError_t e = rocprim::radix_sort_keys(prim, prim_bytes, (const K*)keysA, keysB, size_t(n), 0u, uint32_t(8u * sizeof(K)), s)) return e;
    if (hipError_t e = rocprim::run_length_encode(prim, prim_bytes, (const K*)keysB, size_t(n), merged_out, counts_out, n_runs, s)) return e;
    uint32_t runs = 0u;
    if (hipError_t e = hipMemcpyAsync(&runs, n_runs, 4u, hipMemcpyDeviceToHost, s)) return e;
    if (hipError_t e = hipStreamSynchronize(s)) return e;
    *n_merged_out = runs;
    return hipSuccess;
}

static inline bool qg_index_ok(const nvbio_hip_qgram_index* ix)
{
    if (!ix || !ix->slots || !qg_params_ok(2u, ix->q, ix->ql) || ix->n_unique > ix->n_qgrams) return false;
    if (ix->n_unique && !ix->qgrams) return false;
    if (ix->ql && !ix->lut) return false;
    return true;
}

static inline QgView qg_view(const nvbio_hip_qgram_index* ix)
{
    QgView v;
    v.qgrams = ix->qgrams; v.slots = ix->slots; v.lut = ix->ql ? ix->lut : nullptr; v.q = ix->q; v.ql = ix->ql; v.n_unique = ix->n_unique;
    return v;
}

template <bool SET>
static int qg_locate(const nvbio_hip_qgram_index* ix, uint32_t n_queries, const uint32_t* ranges, const uint64_t* slots, const uint32_t* indices,
                     uint64_t begin, uint64_t end, uint32_t* hits_out, hipStream_t s)
{
    if (!qg_index_ok(ix) || begin > end) return hipErrorInvalidValue;
    if (begin == end) return hipSuccess;
    if (n_queries == 0u || !ranges || !slots || !indices || !hits_out || !ix->index) return hipErrorInvalidValue;
    if ((end - begin + 1023u) / 1024u > 0x7FFFFFFFull) return hipErrorInvalidValue;
    g_last_kernel = SET ? "qgram_set_locate_kernel" : "qgram_locate_kernel";
    hipLaunchKernelGGL(qgram_locate_kernel<SET>, dim3(qg_blocks(end - begin, 1024u)), dim3(256), 0, s, ix->index, ix->n_qgrams, n_queries,
                       reinterpret_cast<const uint2*>(ranges), slots, indices, begin, end, hits_out);
    return hipGetLastError();
}

} // namespace nvb

using namespace nvb;

NVB_API int nvbio_hip_qgram_generate(const uint32_t* words, uint64_t n_words, uint32_t bits, uint32_t big_endian, uint64_t len, uint32_t q,
                                     const uint32_t* positions, uint64_t n, uint64_t* qgrams_out, void* stream)
{
    if (!words || !n_words || !qg_params_ok(bits, q, 0u) || len > QG_MAX_N || n > QG_MAX_N) return hipErrorInvalidValue;
    if (n == 0u) return hipSuccess;
    if (!qgrams_out) return hipErrorInvalidValue;
    const uint32_t be = big_endian ? 1u : 0u;
    if (positions)
    {
        g_last_kernel = "qgram_generate_coords_kernel";
        hipLaunchKernelGGL(qgram_generate_coords_kernel<false>, dim3(qg_blocks(n)), dim3(256), 0, to_stream(stream), words, n_words, be,
                           (const uint64_t*)nullptr, (const uint32_t*)nullptr, 0u, 0u, len, q, positions, n, qgrams_out);
    }
    else
    {
        g_last_kernel = "qgram_generate_kernel";
        hipLaunchKernelGGL(qgram_generate_kernel, dim3(qg_blocks(n, 4096u)), dim3(256), 0, to_stream(stream), words, n_words, be, len, q, n, qgrams_out,
                           (uint32_t*)nullptr);
    }
    return hipGetLastError();
}

NVB_API int nvbio_hip_qgram_set_generate(const nvbio_hip_string_set* set, uint32_t n_strings, uint32_t q, const uint32_t* coords, uint64_t n,
                                         uint64_t* qgrams_out, void* stream)
{
    if (!qg_set_ok(set, n_strings) || !qg_params_ok(2u, q, 0u) || n > QG_MAX_N) return hipErrorInvalidValue;
    if (n == 0u) return hipSuccess;
    if (!coords || !qgrams_out) return hipErrorInvalidValue;
    g_last_kernel = "qgram_generate_coords_kernel";
    hipLaunchKernelGGL(qgram_generate_coords_kernel<true>, dim3(qg_blocks(n)), dim3(256), 0, to_stream(stream), set->words, set->n_words,
                       set->big_endian ? 1u : 0u, set->begin, set->length, set->fixed_length, n_strings, uint64_t(0), q, coords, n, qgrams_out);
    return hipGetLastError();
}

NVB_API uint64_t nvbio_hip_qgram_index_build_temp_bytes(uint64_t n)
{
    if (n > QG_MAX_N) return 256u;
    return qg_build_fixed_bytes<uint32_t>(n, 0u) + qg_build_prim_bytes<uint32_t>(n, 0u);
}

NVB_API int nvbio_hip_qgram_index_build(const uint32_t* words, uint64_t n_words, uint32_t bits, uint32_t big_endian, uint64_t len, uint32_t q, uint32_t ql,
                                        uint64_t* qgrams_out, uint32_t* slots_out, uint32_t* index_out, uint32_t* lut_out, uint32_t* n_unique_out,
                                        void* temp, uint64_t temp_bytes, void* stream)
{
    if (!words || !n_words || !qg_params_ok(bits, q, ql) || len > QG_MAX_N) return hipErrorInvalidValue;
    if (!slots_out || !n_unique_out || (len && (!qgrams_out || !index_out)) || (ql && !lut_out)) return hipErrorInvalidValue;
    if (!temp || temp_bytes < nvbio_hip_qgram_index_build_temp_bytes(len)) return hipErrorInvalidValue;
    const hipStream_t s = to_stream(stream);
    const qg_build_arrays<uint32_t> a = qg_build_carve<uint32_t>(temp, temp_bytes, len, 0u);
    if (len)
    {
        hipLaunchKernelGGL(qgram_generate_kernel, dim3(qg_blocks(len, 4096u)), dim3(256), 0, s, words, n_words, big_endian ? 1u : 0u, len, q, len, a.keysA, a.vals);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return qg_build_finish<uint32_t>(a, len, q, ql, qgrams_out, slots_out, index_out, lut_out, n_unique_out, s);
}

NVB_API uint64_t nvbio_hip_qgram_set_count_seeds_temp_bytes(uint32_t n_strings)
{
    return qg_align(uint64_t(n_strings) * 8u) + qg_scan64_prim_bytes(n_strings);
}

NVB_API int nvbio_hip_qgram_set_count_seeds(const nvbio_hip_string_set* set, uint32_t n_strings, uint32_t q, uint32_t interval, uint64_t* n_qgrams_out,
                                            void* temp, uint64_t temp_bytes, void* stream)
{
    if (!qg_set_ok(set, n_strings) || !qg_params_ok(2u, q, 0u) || interval == 0u || !n_qgrams_out) return hipErrorInvalidValue;
    if (!set->length) { *n_qgrams_out = uint64_t(n_strings) * qg_seed_count(set->fixed_length, q, interval); return hipSuccess; }
    if (!temp || temp_bytes < nvbio_hip_qgram_set_count_seeds_temp_bytes(n_strings)) return hipErrorInvalidValue;
    uint8_t* p = reinterpret_cast<uint8_t*>(temp);
    uint64_t* cum = reinterpret_cast<uint64_t*>(p);   p += qg_align(uint64_t(n_strings) * 8u);
    uint64_t total = 0u;
    g_last_kernel = "qgram_seed_counts_kernel";
    if (int e = qg_seed_sums(set, n_strings, q, interval, cum, p, size_t(temp_bytes - qg_align(uint64_t(n_strings) * 8u)), &total, to_stream(stream))) return e;
    *n_qgrams_out = total;
    return hipSuccess;
}

NVB_API uint64_t nvbio_hip_qgram_set_index_build_temp_bytes(uint64_t n_qgrams, uint32_t n_strings)
{
    if (n_qgrams > QG_MAX_N) return 256u;
    return qg_build_fixed_bytes<uint64_t>(n_qgrams, n_strings) + qg_build_prim_bytes<uint64_t>(n_qgrams, n_strings);
}

NVB_API int nvbio_hip_qgram_set_index_build(const nvbio_hip_string_set* set, uint32_t n_strings, uint32_t q, uint32_t interval, uint32_t ql, uint64_t n_qgrams,
                                            uint64_t* qgrams_out, uint32_t* slots_out, uint32_t* index_out, uint32_t* lut_out, uint32_t* n_unique_out,
                                            void* temp, uint64_t temp_bytes, void* stream)
{
    if (!qg_set_ok(set, n_strings) || !qg_params_ok(2u, q, ql) || interval == 0u || n_qgrams > QG_MAX_N) return hipErrorInvalidValue;
    if (!slots_out || !n_unique_out || (n_qgrams && (!qgrams_out || !index_out)) || (ql && !lut_out)) return hipErrorInvalidValue;
    if (!temp || temp_bytes < nvbio_hip_qgram_set_index_build_temp_bytes(n_qgrams, n_strings)) return hipErrorInvalidValue;
    if (!set->length && uint64_t(n_strings) * qg_seed_count(set->fixed_length, q, interval) != n_qgrams) return hipErrorInvalidValue;
    if (n_strings == 0u && n_qgrams) return hipErrorInvalidValue;
    const hipStream_t s = to_stream(stream);
    const qg_build_arrays<uint64_t> a = qg_build_carve<uint64_t>(temp, temp_bytes, n_qgrams, n_strings);
    if (set->length)                                                 // fixed lengths were checked above, without the device
    {
        uint64_t total = 0u;
        if (int e = qg_seed_sums(set, n_strings, q, interval, a.cum, a.prim, a.prim_bytes, &total, s)) return e;
        if (total != n_qgrams) return hipErrorInvalidValue;          // only the scratch has been written
    }
    if (n_qgrams)
    {
        hipLaunchKernelGGL(qgram_set_seeds_kernel, dim3(qg_blocks(n_qgrams)), dim3(256), 0, s, set->words, set->n_words, set->big_endian ? 1u : 0u, set->begin,
                           set->length, set->fixed_length, n_strings, (const uint64_t*)a.cum, q, interval, n_qgrams, a.keysA, a.vals);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return qg_build_finish<uint64_t>(a, n_qgrams, q, ql, qgrams_out, slots_out, reinterpret_cast<uint64_t*>(index_out), lut_out, n_unique_out, s);
}

NVB_API int nvbio_hip_qgram_range(const nvbio_hip_qgram_index* index, const uint64_t* queries, uint64_t n_queries, uint32_t* ranges_out, void* stream)
{
    if (!qg_index_ok(index) || n_queries > QG_MAX_N) return hipErrorInvalidValue;
    if (n_queries == 0u) return hipSuccess;
    if (!queries || !ranges_out) return hipErrorInvalidValue;
    g_last_kernel = "qgram_range_kernel";
    hipLaunchKernelGGL(qgram_range_kernel, dim3(qg_blocks(n_queries)), dim3(256), 0, to_stream(stream), qg_view(index), queries, n_queries,
                       reinterpret_cast<uint2*>(ranges_out));
    return hipGetLastError();
}

NVB_API uint64_t nvbio_hip_qgram_rank_temp_bytes(uint64_t n_queries)
{
    if (n_queries > QG_MAX_N) return 256u;
    size_t b = 0;
    (void)rocprim::inclusive_scan(nullptr, b, qg_size_iterator((const uint2*)nullptr, qg_range_size()), (uint64_t*)nullptr, size_t(n_queries), rocprim::plus<uint64_t>());
    return qg_align(b) + 256u;
}

NVB_API int nvbio_hip_qgram_rank(const nvbio_hip_qgram_index* index, const uint64_t* queries, uint64_t n_queries, uint32_t* ranges_out, uint64_t* slots_out,
                                 uint64_t* total_out, void* temp, uint64_t temp_bytes, void* stream)
{
    if (!qg_index_ok(index) || n_queries > QG_MAX_N || !total_out) return hipErrorInvalidValue;
    if (n_queries == 0u) { *total_out = 0u; return hipSuccess; }
    if (!queries || !ranges_out || !slots_out || !temp || temp_bytes < nvbio_hip_qgram_rank_temp_bytes(n_queries)) return hipErrorInvalidValue;
    const hipStream_t s = to_stream(stream);
    g_last_kernel = "qgram_range_kernel";
    hipLaunchKernelGGL(qgram_range_kernel, dim3(qg_blocks(n_queries)), dim3(256), 0, s, qg_view(index), queries, n_queries, reinterpret_cast<uint2*>(ranges_out));
    if (hipError_t e = hipGetLastError()) return e;
    size_t prim_bytes = size_t(temp_bytes);
    if (hipError_t e = rocprim::inclusive_scan(temp, prim_bytes, qg_size_iterator(reinterpret_cast<const uint2*>(ranges_out), qg_range_size()), slots_out,
                                               size_t(n_queries), rocprim::plus<uint64_t>(), s)) return e;
    uint64_t total = 0u;
    if (hipError_t e = hipMemcpyAsync(&total, slots_out + (n_queries - 1u), 8u, hipMemcpyDeviceToHost, s)) return e;
    if (hipError_t e = hipStreamSynchronize(s)) return e;
    *total_out = total;
    return hipSuccess;
}

NVB_API int nvbio_hip_qgram_locate(const nvbio_hip_qgram_index* index, uint32_t n_queries, const uint32_t* ranges, const uint64_t* slots,
                                   const uint32_t* indices, uint64_t begin, uint64_t end, uint32_t* hits_out, void* stream)
{
    return qg_locate<false>(index, n_queries, ranges, slots, indices, begin, end, hits_out, to_stream(stream));
}

NVB_API int nvbio_hip_qgram_set_locate(const nvbio_hip_qgram_index* index, uint32_t n_queries, const uint32_t* ranges, const uint64_t* slots,
                                       const uint32_t* indices, uint64_t begin, uint64_t end, uint32_t* hits_out, void* stream)
{
    return qg_locate<true>(index, n_queries, ranges, slots, indices, begin, end, hits_out, to_stream(stream));
}

NVB_API uint64_t nvbio_hip_qgram_merge_temp_bytes(uint32_t n_hits) { return qg_merge_temp_bytes<uint32_t>(n_hits); }
NVB_API uint64_t nvbio_hip_qgram_set_merge_temp_bytes(uint32_t n_hits) { return qg_merge_temp_bytes<uint64_t>(n_hits); }

NVB_API int nvbio_hip_qgram_merge(const uint32_t* hits, uint32_t n_hits, uint32_t interval, uint32_t* merged_out, uint32_t* counts_out, uint32_t* n_merged_out,
                                  void* temp, uint64_t temp_bytes, void* stream)
{
    if (interval == 0u || !n_merged_out) return hipErrorInvalidValue;
    if (n_hits == 0u) { *n_merged_out = 0u; return hipSuccess; }
    if (!hits || !merged_out || !counts_out || !temp || temp_bytes < nvbio_hip_qgram_merge_temp_bytes(n_hits)) return hipErrorInvalidValue;
    const hipStream_t s = to_stream(stream);
    uint8_t* p = reinterpret_cast<uint8_t*>(temp);
    uint32_t* keysA = reinterpret_cast<uint32_t*>(p);   p += qg_align(uint64_t(n_hits) * 4u);
    uint32_t* keysB = reinterpret_cast<uint32_t*>(p);   p += qg_align(uint64_t(n_hits) * 4u);
    uint32_t* n_runs = reinterpret_cast<uint32_t*>(p);  p += 256u;
    g_last_kernel = "qgram_diagonals_kernel";
    hipLaunchKernelGGL(qgram_diagonals_kernel, dim3(qg_blocks(n_hits)), dim3(256), 0, s, reinterpret_cast<const uint2*>(hits), n_hits, interval, keysA);
    if (hipError_t e = hipGetLastError()) return e;
    return qg_merge_finish<uint32_t>(keysA, keysB, n_runs, p, size_t(temp_bytes - uint64_t(p - reinterpret_cast<uint8_t*>(temp))), n_hits, merged_out, counts_out,
                                     n_merged_out, s);
}

NVB_API int nvbio_hip_qgram_set_merge(const uint32_t* hits, uint32_t n_hits, uint32_t interval, uint32_t* merged_out, uint32_t* counts_out, uint32_t* n_merged_out,
                                      void* temp, uint64_t temp_bytes, void* stream)
{
    if (interval == 0u || !n_merged_out) return hipErrorInvalidValue;
    if (n_hits == 0u) { *n_merged_out = 0u; return hipSuccess; }
    if (!hits || !merged_out || !counts_out || !temp || temp_bytes < nvbio_hip_qgram_set_merge_temp_bytes(n_hits)) return hipErrorInvalidValue;
    const hipStream_t s = to_stream(stream);
    uint8_t* p = reinterpret_cast<uint8_t*>(temp);
    uint64_t* keysA = reinterpret_cast<uint64_t*>(p);   p += qg_align(uint64_t(n_hits) * 8u);
    uint64_t* keysB = reinterpret_cast<uint64_t*>(p);   p += qg_align(uint64_t(n_hits) * 8u);
    uint32_t* n_runs = reinterpret_cast<uint32_t*>(p);  p += 256u;
    g_last_kernel = "qgram_set_diagonals_kernel";
    hipLaunchKernelGGL(qgram_set_diagonals_kernel, dim3(qg_blocks(n_hits)), dim3(256), 0, s, reinterpret_cast<const uint4*>(hits), n_hits, interval, keysA);
    if (hipError_t e = hipGetLastError()) return e;
    return qg_merge_finish<uint64_t>(keysA, keysB, n_runs, p, size_t(temp_bytes - uint64_t(p - reinterpret_cast<uint8_t*>(temp))), n_hits,
                                     reinterpret_cast<uint64_t*>(merged_out), counts_out, n_merged_out, s);
}
