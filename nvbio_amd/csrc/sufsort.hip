// sufsort.hip -- suffix sorting and BWT construction of one 2-bit packed text on the device: the plain-string front door of the
// reference's nvbio/sufsort (cuda::suffix_sort, cuda::bwt, cuda::find_primary).  DESIGN.md 3.13.
//
// Output convention (compat/nvbio/fmindex/bwt.h): SA has n + 1 rows, SA[0] = n is the empty suffix, and a suffix that is a proper
// prefix of another sorts first ($ < A).  Below, "row" k in [0, n) is SA row k + 1: only the n real suffixes are sorted.
//
// Round 0 sorts one 64-bit key per suffix, the doubling rounds sort only the suffixes whose group still has more than one member:
//   rank[i] = 1 + the row of the head of i's group (Larsson-Sadakane), so a finished suffix never moves again and the members of an
//   unresolved group keep the rows of their group whatever order a round gives them;  key = (rank[i], rank[i + h]), past-the-end = 0.
#include "common.h"
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <algorithm>

namespace nvb {

static constexpr uint32_t SS_K0 = 29u;                  // symbols in the round-0 key: 58 bits, beside a 6-bit length field
static constexpr uint64_t SS_MAX_N = 0xFFFFFFFEull;     // n < 2^32 - 1: n itself is a value of SA, and rank n + 0 a uint32

__device__ __forceinline__ uint32_t ss_word_be(const uint32_t* __restrict__ words, const uint64_t w, const uint64_t n_words, const uint32_t be)
{
    if (w >= n_words) return 0u;
    const uint32_t x = words[w];
    return be ? x : rev2(x);                            // symbol k of the word at bits [30 - 2k, 32 - 2k)
}

__device__ __forceinline__ uint32_t ss_symbol(const uint32_t* __restrict__ words, const uint32_t be, const uint64_t i)
{
    const uint32_t k = uint32_t(i & 15u);
    return (words[i >> 4] >> (be ? 30u - 2u * k : 2u * k)) & 3u;
}

// The round-0 key of suffix i: its first 29 symbols, most significant first, symbols past the end as 0, then min(n - i, 29).
//
// Claim: key(i) < key(j) implies suffix i < suffix j in the $ < A order, and key(i) == key(j) iff both suffixes have at least 29
// symbols and the same first 29.  Proof.  Let ri = n - i, rj = n - j (distinct for i != j), pi, pj the padded 29-symbol fields.
// (1) pi != pj, first difference at position p.  If p < min(ri, rj) both symbols are real and decide the order as the text does.
//     Otherwise one suffix has ended there, say i (p >= ri): its pad is 0, the other's symbol is c != 0, so pi < pj; and suffix j
//     shares i's ri real symbols (no difference before p, and between ri and p suffix j holds A = 0 = the pad), so i is a proper
//     prefix of a string that is <= suffix j's first p symbols followed by c > nothing: i sorts first.  Both suffixes cannot have
//     ended at p, for two pads are equal.
// (2) pi == pj.  If ri, rj >= 29 the length fields are both 29: equal keys, the same 29-prefix, one group -- as it must be.
//     Otherwise say ri < rj and ri < 29: j's symbols [ri, min(rj, 29)) equal i's pads, so they are A, and i's ri real symbols are
//     j's first ri: suffix i is a proper prefix of suffix j and sorts first; and its field ri < min(rj, 29).  So every suffix
//     shorter than 29 has a key of its own, in its right place.                                                                  []
__global__ __launch_bounds__(256) void sufsort_key0_kernel(const uint32_t* __restrict__ words, const uint32_t be, const uint64_t n, const uint64_t n_words,
                                                           uint64_t* __restrict__ keys, uint32_t* __restrict__ ids)
{
    const uint64_t i = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t w = i >> 4;
    const uint32_t o = 2u * uint32_t(i & 15u);
    const uint64_t hi = (uint64_t(ss_word_be(words, w, n_words, be)) << 32) | ss_word_be(words, w + 1u, n_words, be);
    const uint64_t lo = ss_word_be(words, w + 2u, n_words, be);
    uint64_t v = o ? ((hi << o) | (lo >> (32u - o))) : hi;            // 32 symbols from i on, the first at the top
    const uint64_t rem = n - i;
    if (rem < SS_K0) v &= ~0ull << (64u - 2u * uint32_t(rem));         // symbols past the end read as 0, whatever the last word holds
    keys[i] = (v & ~63ull) | (rem < SS_K0 ? rem : uint64_t(SS_K0));
    ids[i]  = uint32_t(i);
}

// head[k] = k where a new group starts at sorted position k, else 0; an inclusive max-scan turns it into the head of k's group
__global__ __launch_bounds__(256) void sufsort_heads_kernel(const uint64_t* __restrict__ keys, const uint64_t m, uint32_t* __restrict__ head)
{
    const uint64_t k = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    if (k >= m) return;
    head[k] = (k && keys[k] != keys[k - 1u]) ? uint32_t(k) : 0u;
}

// After a round's sort: position k of the unresolved list keeps its row (the list is in SA order and a sort permutes within groups),
// the suffix there gets the row of its new group's head + 1 as rank, and keep[k] = 1 unless it is alone in its group.
__global__ __launch_bounds__(256) void sufsort_update_kernel(const uint32_t* __restrict__ ids, const uint32_t* __restrict__ head, const uint32_t* __restrict__ urow,
                                                             const uint64_t m, uint32_t* __restrict__ rank, uint32_t* __restrict__ sa_rows, uint32_t* __restrict__ keep)
{
    const uint64_t k = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    if (k >= m) return;
    const uint32_t h = head[k];
    const bool alone = (h == uint32_t(k)) && (k + 1u == m || head[k + 1u] == uint32_t(k + 1u));
    const uint32_t id = ids[k];
    const uint32_t row = urow ? urow[k] : uint32_t(k), hrow = urow ? urow[h] : h;
    sa_rows[row] = id;
    rank[id] = hrow + 1u;
    keep[k] = alone ? 0u : 1u;
}

// incl = inclusive sum of keep: the survivors move up, in order
__global__ __launch_bounds__(256) void sufsort_compact_kernel(const uint32_t* __restrict__ ids, const uint32_t* __restrict__ urow, const uint32_t* __restrict__ incl,
                                                              const uint64_t m, uint32_t* __restrict__ ids_out, uint32_t* __restrict__ urow_out)
{
    const uint64_t k = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    if (k >= m) return;
    const uint32_t at = incl[k];
    if (at == (k ? incl[k - 1u] : 0u)) return;
    ids_out[at - 1u]  = ids[k];
    urow_out[at - 1u] = urow ? urow[k] : uint32_t(k);
}

// key = rank[i] << b | rank[i + h]: two random 4-byte reads a suffix, nothing else.  Four suffixes a lane, all eight loads issued
// before the first is used, so a wave keeps 512 lines in flight.
__global__ __launch_bounds__(256) void sufsort_key_kernel(const uint32_t* __restrict__ ids, const uint64_t m, const uint32_t* __restrict__ rank, const uint64_t n,
                                                          const uint64_t h, const uint32_t b, uint64_t* __restrict__ keys)
{
    const uint64_t base = uint64_t(blockIdx.x) * 1024u + threadIdx.x;
    uint32_t r0[4], r1[4];
    #pragma unroll
    for (uint32_t q = 0; q < 4u; ++q)
    {
        const uint64_t k = base + q * 256u;
        r0[q] = r1[q] = 0u;
        if (k < m)
        {
            const uint64_t i = ids[k];
            r0[q] = rank[i];
            if (i + h < n) r1[q] = rank[i + h];
        }
    }
    #pragma unroll
    for (uint32_t q = 0; q < 4u; ++q)
    {
        const uint64_t k = base + q * 256u;
        if (k < m) keys[k] = (uint64_t(r0[q]) << b) | r1[q];
    }
}

// one output word = 16 BWT symbols, big-endian: bwt[j] = T[SA[row] - 1] over the rows but the primary (rank[0], where SA is 0)
__global__ __launch_bounds__(256) void sufsort_bwt_kernel(const uint32_t* __restrict__ words, const uint32_t be, const uint64_t n, const uint32_t* __restrict__ sa,
                                                          const uint32_t* __restrict__ rank, const uint64_t n_out_words, uint32_t* __restrict__ bwt_words)
{
    const uint64_t w = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    if (w >= n_out_words) return;
    const uint64_t primary = rank[0];
    uint32_t s[16];
    #pragma unroll
    for (uint32_t q = 0; q < 16u; ++q)
    {
        const uint64_t j = w * 16u + q;
        s[q] = j < n ? sa[j + (j >= primary ? 1u : 0u)] : 0u;
    }
    uint32_t out = 0u;
    #pragma unroll
    for (uint32_t q = 0; q < 16u; ++q)
    {
        const uint64_t j = w * 16u + q;
        if (j < n && s[q]) out |= ss_symbol(words, be, uint64_t(s[q]) - 1u) << (30u - 2u * q);       // s is never 0 off the primary row
    }
    bwt_words[w] = out;
}

__global__ __launch_bounds__(256) void sufsort_ssa_kernel(const uint32_t* __restrict__ sa, const uint64_t n_ssa, const uint32_t sa_int, uint32_t* __restrict__ ssa)
{
    const uint64_t k = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    if (k >= n_ssa) return;
    ssa[k] = k ? sa[k * sa_int] : 0xFFFFFFFFu;
}

static inline uint64_t ss_align(uint64_t x) { return (x + 255ull) & ~255ull; }
static inline uint32_t ss_blocks(uint64_t items, uint32_t per_block = 256u) { return uint32_t((items + per_block - 1u) / per_block); }

// what rocPRIM asks for the largest sort and scan of a call (0 where no device answers the query: the entries then fail anyway)
static uint64_t ss_prim_bytes(uint64_t n)
{
    size_t sort = 0, scan_max = 0, scan_sum = 0;
    rocprim::double_buffer<uint64_t> k(nullptr, nullptr);
    rocprim::double_buffer<uint32_t> v(nullptr, nullptr);
    (void)rocprim::radix_sort_pairs(nullptr, sort, k, v, size_t(n), 0u, 64u);
    (void)rocprim::inclusive_scan(nullptr, scan_max, (const uint32_t*)nullptr, (uint32_t*)nullptr, size_t(n), rocprim::maximum<uint32_t>());
    (void)rocprim::inclusive_scan(nullptr, scan_sum, (const uint32_t*)nullptr, (uint32_t*)nullptr, size_t(n), rocprim::plus<uint32_t>());
    return ss_align(std::max<uint64_t>(sort, std::max<uint64_t>(scan_max, scan_sum))) + 256u;
}

// temp layout: keys A | keys B (8n each; the one a sort leaves free holds the round's head and keep words) | ids A | ids B | rows A |
// rows B | rank (4n each) | rocPRIM's scratch
static inline uint64_t ss_fixed_bytes(uint64_t n) { return 2u * ss_align(n * 8u) + 5u * ss_align(n * 4u); }

thread_local uint32_t g_ss_rounds = 0;
thread_local uint64_t g_ss_unresolved[64];

static int ss_sort(const uint32_t* words, uint32_t be, uint64_t n, uint32_t* sa_out, uint32_t** rank_out, void* temp, uint64_t temp_bytes, hipStream_t s)
{
    uint8_t* p = reinterpret_cast<uint8_t*>(temp);
    uint64_t* keysA = reinterpret_cast<uint64_t*>(p);   p += ss_align(n * 8u);
    uint64_t* keysB = reinterpret_cast<uint64_t*>(p);   p += ss_align(n * 8u);
    uint32_t* idsA  = reinterpret_cast<uint32_t*>(p);   p += ss_align(n * 4u);
    uint32_t* idsB  = reinterpret_cast<uint32_t*>(p);   p += ss_align(n * 4u);
    uint32_t* rowsA = reinterpret_cast<uint32_t*>(p);   p += ss_align(n * 4u);
    uint32_t* rowsB = reinterpret_cast<uint32_t*>(p);   p += ss_align(n * 4u);
    uint32_t* rank  = reinterpret_cast<uint32_t*>(p);   p += ss_align(n * 4u);
    void* prim = p;
    size_t prim_bytes = size_t(temp_bytes - uint64_t(p - reinterpret_cast<uint8_t*>(temp)));
    *rank_out = rank;

    if (hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(sa_out), int(uint32_t(n)), 1u, s)) return e;      // SA[0] = n
    uint32_t* sa_rows = sa_out + 1;
    const uint32_t b = 64u - uint32_t(__builtin_clzll(n));         // a rank is at most n
    const dim3 block(256);

    g_last_kernel = "sufsort_key0_kernel";
    g_ss_rounds = 0;
    hipLaunchKernelGGL(sufsort_key0_kernel, dim3(ss_blocks(n)), block, 0, s, words, be, n, (n + 15u) / 16u, keysA, idsA);
    if (hipError_t e = hipGetLastError()) return e;

    rocprim::double_buffer<uint64_t> keys(keysA, keysB);
    rocprim::double_buffer<uint32_t> ids(idsA, idsB);
    uint32_t* urow = nullptr;                                       // round 0: position k is row k
    uint32_t* urow_next = rowsA;
    uint64_t m = n, h = SS_K0;
    uint32_t end_bit = 64u;
    while (true)
    {
        if (hipError_t e = rocprim::radix_sort_pairs(prim, prim_bytes, keys, ids, size_t(m), 0u, end_bit, s)) return e;
        uint32_t* head = reinterpret_cast<uint32_t*>(keys.alternate());
        uint32_t* keep = head + m;
        hipLaunchKernelGGL(sufsort_heads_kernel, dim3(ss_blocks(m)), block, 0, s, keys.current(), m, head);
        if (hipError_t e = hipGetLastError()) return e;
        if (hipError_t e = rocprim::inclusive_scan(prim, prim_bytes, head, head, size_t(m), rocprim::maximum<uint32_t>(), s)) return e;
        hipLaunchKernelGGL(sufsort_update_kernel, dim3(ss_blocks(m)), block, 0, s, ids.current(), head, urow, m, rank, sa_rows, keep);
        if (hipError_t e = hipGetLastError()) return e;
        if (hipError_t e = rocprim::inclusive_scan(prim, prim_bytes, keep, keep, size_t(m), rocprim::plus<uint32_t>(), s)) return e;
        uint32_t left = 0;
        if (hipError_t e = hipMemcpyAsync(&left, keep + (m - 1u), 4u, hipMemcpyDeviceToHost, s)) return e;
        if (hipError_t e = hipStreamSynchronize(s)) return e;       // the loop's termination test: the one wait of a round
        if (g_ss_rounds < 64u) g_ss_unresolved[g_ss_rounds] = left;
        ++g_ss_rounds;
        if (left == 0u) break;
        hipLaunchKernelGGL(sufsort_compact_kernel, dim3(ss_blocks(m)), block, 0, s, ids.current(), urow, keep, m, ids.alternate(), urow_next);
        if (hipError_t e = hipGetLastError()) return e;
        ids.swap();
        urow = urow_next;
        urow_next = (urow == rowsA) ? rowsB : rowsA;
        m = left;
        g_last_kernel = "sufsort_key_kernel";
        hipLaunchKernelGGL(sufsort_key_kernel, dim3(ss_blocks(m, 1024u)), block, 0, s, ids.current(), m, rank, n, h, b, keys.current());
        if (hipError_t e = hipGetLastError()) return e;
        end_bit = 2u * b;
        h *= 2u;                                                    // the order now known covers h symbols
    }
    return hipSuccess;
}

static int ss_check(const uint32_t* words, uint32_t bits, uint64_t n)
{
    if (!words) return hipErrorInvalidValue;
    if (bits != 2u) return hipErrorInvalidValue;
    if (n == 0u || n > SS_MAX_N) return hipErrorInvalidValue;
    return hipSuccess;
}

} // namespace nvb

using namespace nvb;

NVB_API uint64_t nvbio_hip_suffix_sort_temp_bytes(uint64_t n)
{
    if (n == 0u || n > SS_MAX_N) return 256u;
    return ss_fixed_bytes(n) + ss_prim_bytes(n);
}

NVB_API int nvbio_hip_suffix_sort(const uint32_t* words, uint32_t bits, uint32_t big_endian, uint64_t n, uint32_t* sa_out,
                                  void* temp, uint64_t temp_bytes, void* stream)
{
    if (int e = ss_check(words, bits, n)) return e;
    if (!sa_out || !temp || temp_bytes < nvbio_hip_suffix_sort_temp_bytes(n)) return hipErrorInvalidValue;
    uint32_t* rank = nullptr;
    return ss_sort(words, big_endian ? 1u : 0u, n, sa_out, &rank, temp, temp_bytes, to_stream(stream));
}

NVB_API uint32_t nvbio_hip_suffix_sort_last_rounds(uint64_t* out_unresolved, uint32_t capacity)
{
    for (uint32_t r = 0; out_unresolved && r < g_ss_rounds && r < capacity && r < 64u; ++r) out_unresolved[r] = g_ss_unresolved[r];
    return g_ss_rounds;
}

NVB_API uint64_t nvbio_hip_bwt_temp_bytes(uint64_t n)
{
    if (n == 0u || n > SS_MAX_N) return 256u;
    return ss_align((n + 1u) * 4u) + nvbio_hip_suffix_sort_temp_bytes(n);         // the SA when the caller does not want it, then the sorter's
}

NVB_API int nvbio_hip_bwt(const uint32_t* words, uint32_t bits, uint32_t big_endian, uint64_t n, uint32_t sa_int, uint32_t* bwt_words_out,
                          uint32_t* primary_out, uint32_t* ssa_out, uint32_t* sa_out, void* temp, uint64_t temp_bytes, void* stream)
{
    if (int e = ss_check(words, bits, n)) return e;
    if (!bwt_words_out || !primary_out || (ssa_out && sa_int == 0u)) return hipErrorInvalidValue;
    if (!temp || temp_bytes < nvbio_hip_bwt_temp_bytes(n)) return hipErrorInvalidValue;
    hipStream_t s = to_stream(stream);
    uint8_t* p = reinterpret_cast<uint8_t*>(temp);
    uint32_t* sa = sa_out ? sa_out : reinterpret_cast<uint32_t*>(p);
    p += ss_align((n + 1u) * 4u);
    uint32_t* rank = nullptr;
    const uint32_t be = big_endian ? 1u : 0u;
    if (int e = ss_sort(words, be, n, sa, &rank, p, temp_bytes - ss_align((n + 1u) * 4u), s)) return e;
    const uint64_t n_out_words = 4u * ((n + 63u) / 64u);
    g_last_kernel = "sufsort_bwt_kernel";
    hipLaunchKernelGGL(sufsort_bwt_kernel, dim3(ss_blocks(n_out_words)), dim3(256), 0, s, words, be, n, sa, rank, n_out_words, bwt_words_out);
    if (hipError_t e = hipGetLastError()) return e;
    if (ssa_out)
    {
        const uint64_t n_ssa = (n + sa_int) / sa_int;               // ceil((n + 1) / sa_int)
        hipLaunchKernelGGL(sufsort_ssa_kernel, dim3(ss_blocks(n_ssa)), dim3(256), 0, s, sa, n_ssa, sa_int, ssa_out);
        if (hipError_t e = hipGetLastError()) return e;
    }
    if (hipError_t e = hipMemcpyAsync(primary_out, rank, 4u, hipMemcpyDeviceToHost, s)) return e;       // rank[0]: the row of suffix 0
    return hipStreamSynchronize(s);
}
