// sufsort.hip -- suffix sorting and BWT construction of one 2-bit packed text on the device: the plain-string front door of the
// reference's nvbio/sufsort (cuda::suffix_sort, cuda::bwt, cuda::find_primary).  DESIGN.md 3.13.  A byte text of 1 to 8 bits a symbol
// goes through the same rounds from a round-0 key of its own (the `_bytes` entries).
//
// Output convention (compat/nvbio/fmindex/bwt.h): SA has n + 1 rows, SA[0] = n is the empty suffix, and a suffix that is a proper
// prefix of another sorts first ($ < A).  Below, "row" k in [0, n) is SA row k + 1: only the n real suffixes are sorted.
//
// Round 0 sorts one 64-bit key per suffix, the doubling rounds sort only the suffixes whose group still has more than one member:
//   rank[i] = 1 + the row of the head of i's group (Larsson-Sadakane), so a finished suffix never moves again and the members of an
//   unresolved group keep the rows of their group whatever order a round gives them;  key = (rank[i], rank[i + h]), past-the-end = 0.
//
// The second half of the file is the same front door for a set of strings (cuda::suffix_sort(string_set, ..), cuda::bwt of a
// ConcatenatedStringSet): every string's suffixes, the empty one included, through the same rounds, with a round-0 key read per string
// and a head rule that settles equal short suffixes by string id.  Scratch of a set call: the sorter's seven arrays over the n slots
// (36 n) | string_ids (4 n) | cum, the 64-bit inclusive sums of length + 1 (8 N) | rocPRIM's; the BWT entry puts the sorted slots (4 n)
// in front.
#include "common.h"
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
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

// head[k] = k where a new group starts at sorted position k, else 0; an inclusive max-scan turns it into the head of k's group.
// SET_KEY0: the keys are the round-0 keys of a string set's slots (sufsort_set_key0_kernel), where a length field below 29 starts a
// group too.
template <bool SET_KEY0>
__global__ __launch_bounds__(256) void sufsort_heads_kernel(const uint64_t* __restrict__ keys, const uint64_t m, uint32_t* __restrict__ head)
{
    const uint64_t k = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    if (k >= m) return;
    const uint64_t key = keys[k];
    bool starts = k && key != keys[k - 1u];
    if (SET_KEY0) starts = k && (starts || uint32_t(key & 63u) < SS_K0);
    head[k] = starts ? uint32_t(k) : 0u;
}

// After a round's sort: position k of the unresolved list keeps its row (the list is in SA order and a sort permutes within groups),
// the suffix there gets the row of its new group's head + 1 as rank, and keep[k] = 1 unless it is alone in its group.
// CHECK_TOTAL (round 0 of a string set with a length array): nothing is written unless *total == m, the slot count the caller gave --
// so a wrong count reaches no output, and the host learns of it with the round's own wait.
template <bool CHECK_TOTAL>
__global__ __launch_bounds__(256) void sufsort_update_kernel(const uint32_t* __restrict__ ids, const uint32_t* __restrict__ head, const uint32_t* __restrict__ urow,
                                                             const uint64_t m, uint32_t* __restrict__ rank, uint32_t* __restrict__ sa_rows, uint32_t* __restrict__ keep,
                                                             const uint64_t* __restrict__ total)
{
    const uint64_t k = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    if (k >= m) return;
    if (CHECK_TOTAL && *total != m) return;
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

// the sorter's arrays inside the caller's scratch
struct ss_buffers
{
    uint64_t *keysA, *keysB;
    uint32_t *idsA, *idsB, *rowsA, *rowsB, *rank;
    uint8_t*  end;                                      // what follows the seven arrays
};
static ss_buffers ss_carve(void* temp, uint64_t n)
{
    ss_buffers b;
    uint8_t* p = reinterpret_cast<uint8_t*>(temp);
    b.keysA = reinterpret_cast<uint64_t*>(p);   p += ss_align(n * 8u);
    b.keysB = reinterpret_cast<uint64_t*>(p);   p += ss_align(n * 8u);
    b.idsA  = reinterpret_cast<uint32_t*>(p);   p += ss_align(n * 4u);
    b.idsB  = reinterpret_cast<uint32_t*>(p);   p += ss_align(n * 4u);
    b.rowsA = reinterpret_cast<uint32_t*>(p);   p += ss_align(n * 4u);
    b.rowsB = reinterpret_cast<uint32_t*>(p);   p += ss_align(n * 4u);
    b.rank  = reinterpret_cast<uint32_t*>(p);   p += ss_align(n * 4u);
    b.end = p;
    return b;
}

// The sorting rounds over the n round-0 keys in keysA with ids 0..n-1 in idsA: sa_rows[row] = the suffix on that row, rank[i] = its
// row + 1.  SET_KEY0: the keys are a string set's (sufsort_set_key0_kernel) and round 0 takes that head rule; d_total, if not NULL, is
// the device word that must equal n: round 0 writes nothing but scratch unless it does, and its wait brings the word to the host too.
// h0: the symbols a round-0 key orders by, the first doubling step (29 for the 2-bit keys, floor(58 / S) for a byte text's).
template <bool SET_KEY0>
static int ss_rounds(const ss_buffers& bufs, uint64_t n, uint32_t* sa_rows, void* prim, size_t prim_bytes, hipStream_t s, const uint64_t* d_total = nullptr,
                     const uint64_t h0 = SS_K0)
{
    uint32_t* const rowsA = bufs.rowsA, * const rowsB = bufs.rowsB, * const rank = bufs.rank;
    const uint32_t b = 64u - uint32_t(__builtin_clzll(n));         // a rank is at most n
    const dim3 block(256);
    g_ss_rounds = 0;

    rocprim::double_buffer<uint64_t> keys(bufs.keysA, bufs.keysB);
    rocprim::double_buffer<uint32_t> ids(bufs.idsA, bufs.idsB);
    uint32_t* urow = nullptr;                                       // round 0: position k is row k
    uint32_t* urow_next = rowsA;
    uint64_t m = n, h = h0;
    uint32_t end_bit = 64u;
    while (true)
    {
        if (hipError_t e = rocprim::radix_sort_pairs(prim, prim_bytes, keys, ids, size_t(m), 0u, end_bit, s)) return e;
        uint32_t* head = reinterpret_cast<uint32_t*>(keys.alternate());
        uint32_t* keep = head + m;
        if (SET_KEY0 && h == h0) hipLaunchKernelGGL(sufsort_heads_kernel<true>, dim3(ss_blocks(m)), block, 0, s, keys.current(), m, head);
        else hipLaunchKernelGGL(sufsort_heads_kernel<false>, dim3(ss_blocks(m)), block, 0, s, keys.current(), m, head);
        if (hipError_t e = hipGetLastError()) return e;
        if (hipError_t e = rocprim::inclusive_scan(prim, prim_bytes, head, head, size_t(m), rocprim::maximum<uint32_t>(), s)) return e;
        const bool check_total = SET_KEY0 && h == h0 && d_total;
        if (check_total) hipLaunchKernelGGL(sufsort_update_kernel<true>, dim3(ss_blocks(m)), block, 0, s, ids.current(), head, urow, m, rank, sa_rows, keep, d_total);
        else hipLaunchKernelGGL(sufsort_update_kernel<false>, dim3(ss_blocks(m)), block, 0, s, ids.current(), head, urow, m, rank, sa_rows, keep, (const uint64_t*)nullptr);
        if (hipError_t e = hipGetLastError()) return e;
        if (hipError_t e = rocprim::inclusive_scan(prim, prim_bytes, keep, keep, size_t(m), rocprim::plus<uint32_t>(), s)) return e;
        uint32_t left = 0;
        uint64_t total = n;
        if (check_total) if (hipError_t e = hipMemcpyAsync(&total, d_total, 8u, hipMemcpyDeviceToHost, s)) return e;
        if (hipError_t e = hipMemcpyAsync(&left, keep + (m - 1u), 4u, hipMemcpyDeviceToHost, s)) return e;
        if (hipError_t e = hipStreamSynchronize(s)) return e;       // the loop's termination test: the one wait of a round
        if (total != n) return hipErrorInvalidValue;
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

static int ss_sort(const uint32_t* words, uint32_t be, uint64_t n, uint32_t* sa_out, uint32_t** rank_out, void* temp, uint64_t temp_bytes, hipStream_t s)
{
    const ss_buffers bufs = ss_carve(temp, n);
    *rank_out = bufs.rank;
    if (hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(sa_out), int(uint32_t(n)), 1u, s)) return e;      // SA[0] = n
    g_last_kernel = "sufsort_key0_kernel";
    hipLaunchKernelGGL(sufsort_key0_kernel, dim3(ss_blocks(n)), dim3(256), 0, s, words, be, n, (n + 15u) / 16u, bufs.keysA, bufs.idsA);
    if (hipError_t e = hipGetLastError()) return e;
    return ss_rounds<false>(bufs, n, sa_out + 1, bufs.end, size_t(temp_bytes - uint64_t(bufs.end - reinterpret_cast<uint8_t*>(temp))), s);
}

static int ss_check(const uint32_t* words, uint32_t bits, uint64_t n)
{
    if (!words) return hipErrorInvalidValue;
    if (bits != 2u) return hipErrorInvalidValue;
    if (n == 0u || n > SS_MAX_N) return hipErrorInvalidValue;
    return hipSuccess;
}

// ---- a byte text: one symbol per byte, S = symbol_size bits of it (nvbio_hip_suffix_sort_bytes / nvbio_hip_bwt_bytes) ----
//
// The round-0 key of suffix i: its first K0 = floor(58 / S) symbols, most significant first (symbol j at bits [64 - S (j + 1), 64 - S j)),
// symbols past the end as 0, then min(n - i, K0) in the low 6 bits (K0 <= 58 fits, and S K0 <= 58 leaves them free).  The claim above
// sufsort_key0_kernel uses of the alphabet only that the pad, 0, is its smallest symbol: read 29 as K0 and A as symbol 0 and it holds as
// it stands, so the rounds take these keys with h0 = K0.
__global__ __launch_bounds__(256) void sufsort_bytes_key0_kernel(const uint8_t* __restrict__ symbols, const uint32_t S, const uint32_t k0, const uint64_t n,
                                                                 uint64_t* __restrict__ keys, uint32_t* __restrict__ ids)
{
    const uint64_t i = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t rem = n - i;
    const uint32_t len = rem < k0 ? uint32_t(rem) : k0, mask = (1u << S) - 1u;
    uint64_t v = 0u;
    uint32_t sh = 64u;
    for (uint32_t j = 0; j < len; ++j)
    {
        sh -= S;
        v |= uint64_t(symbols[i + j] & mask) << sh;
    }
    keys[i] = v | len;
    ids[i]  = uint32_t(i);
}

// bwt[j] = T[SA[row] - 1] over the rows but the primary (rank[0]), one byte a symbol.  A lane owns four rows -- one 32-bit word of the
// output -- and issues its four SA loads, then its four symbol loads, before it uses the first.
__global__ __launch_bounds__(256) void sufsort_bytes_bwt_kernel(const uint8_t* __restrict__ symbols, const uint32_t mask, const uint64_t n, const uint32_t* __restrict__ sa,
                                                                const uint32_t* __restrict__ rank, uint8_t* __restrict__ bwt_out, const uint32_t word_stores)
{
    const uint64_t w = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    const uint64_t j0 = w * 4u;
    if (j0 >= n) return;
    const uint64_t primary = rank[0];
    uint32_t s[4], sym[4];
    #pragma unroll
    for (uint32_t q = 0; q < 4u; ++q)
    {
        const uint64_t j = j0 + q;
        s[q] = j < n ? sa[j + (j >= primary ? 1u : 0u)] : 0u;
    }
    #pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) sym[q] = s[q] ? uint32_t(symbols[s[q] - 1u]) & mask : 0u;        // s is never 0 off the primary row
    if (word_stores && j0 + 4u <= n) reinterpret_cast<uint32_t*>(bwt_out)[w] = sym[0] | (sym[1] << 8) | (sym[2] << 16) | (sym[3] << 24);
    else
    {
        #pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) if (j0 + q < n) bwt_out[j0 + q] = uint8_t(sym[q]);
    }
}

static int ss_bytes_check(const uint8_t* symbols, uint32_t symbol_size, uint64_t n)
{
    if (!symbols) return hipErrorInvalidValue;
    if (symbol_size < 1u || symbol_size > 8u) return hipErrorInvalidValue;
    if (n == 0u || n > SS_MAX_N) return hipErrorInvalidValue;
    return hipSuccess;
}

static int ss_bytes_sort(const uint8_t* symbols, uint32_t S, uint64_t n, uint32_t* sa_out, uint32_t** rank_out, void* temp, uint64_t temp_bytes, hipStream_t s)
{
    const ss_buffers bufs = ss_carve(temp, n);
    *rank_out = bufs.rank;
    const uint32_t k0 = 58u / S;
    if (hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(sa_out), int(uint32_t(n)), 1u, s)) return e;      // SA[0] = n
    g_last_kernel = "sufsort_bytes_key0_kernel";
    hipLaunchKernelGGL(sufsort_bytes_key0_kernel, dim3(ss_blocks(n)), dim3(256), 0, s, symbols, S, k0, n, bufs.keysA, bufs.idsA);
    if (hipError_t e = hipGetLastError()) return e;
    return ss_rounds<false>(bufs, n, sa_out + 1, bufs.end, size_t(temp_bytes - uint64_t(bufs.end - reinterpret_cast<uint8_t*>(temp))), s, nullptr, k0);
}

// ---- the suffixes of a string set (cuda::suffix_sort(string_set, ..), cuda::bwt(ConcatenatedStringSet, ..)) ----
//
// The slots of a set of N strings are the pairs (s, p), 0 <= p <= len[s] -- the empty suffix p == len[s] included -- and slot (s, p) has
// the global index g = cum[s - 1] + p, cum[s] = the inclusive sum of len + 1.  They are ordered by their symbols with $ < A (a proper
// prefix first), equal suffixes by string id.  Below, rem(g) = len[s] - p is the number of symbols slot g has left, and a slot is
// "resolved" once it is alone in its group.

struct ss_len1 { __host__ __device__ uint64_t operator()(const uint32_t l) const { return uint64_t(l) + 1u; } };
typedef rocprim::transform_iterator<const uint32_t*, ss_len1, uint64_t> ss_len1_iterator;

__global__ __launch_bounds__(256) void sufsort_set_cum_fixed_kernel(const uint64_t n_strings, const uint64_t fixed1, uint64_t* __restrict__ cum)
{
    const uint64_t s = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    if (s < n_strings) cum[s] = (s + 1u) * fixed1;
}

// string_ids[first slot of s] = s over zeroes; an inclusive max-scan then gives every slot its string (every string has a slot).
// The bound holds whenever n is the lengths' sum; it is there for the caller whose n is not, which is found out only after round 0.
__global__ __launch_bounds__(256) void sufsort_set_first_slots_kernel(const uint64_t* __restrict__ cum, const uint64_t n_strings, const uint64_t n,
                                                                      uint32_t* __restrict__ string_ids)
{
    const uint64_t s = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    if (s + 1u >= n_strings) return;
    const uint64_t first = cum[s];
    if (first < n) string_ids[first] = uint32_t(s + 1u);
}

__global__ __launch_bounds__(256) void sufsort_set_cum32_kernel(const uint64_t* __restrict__ cum, const uint64_t n_strings, uint32_t* __restrict__ out)
{
    const uint64_t s = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    if (s < n_strings) out[s] = uint32_t(cum[s]);
}

// The round-0 key of slot g = (s, p): the first 29 symbols of the suffix within its string, symbols past the string's end as 0, then
// min(rem, 29) -- sufsort_key0_kernel's key with the string's end for the text's, read from begin[s] + p.
//
// Claim 1 (round 0).  Sort the keys stably with the ids ascending, and start a group where the key differs from its left neighbour's
// or its length field is below 29.  Then the groups stand in suffix order, a group of more than one slot holds exactly the slots that
// share their first 29 symbols and have rem >= 29, and every slot with rem < 29 is alone in its group, on its final row.
// Proof.  The claim above sufsort_key0_kernel compares two padded fields and two lengths and never uses that the suffixes lie in one
// text, except for "ri != rj".  So for two slots: key(i) < key(j) implies suffix i < suffix j, or i is a proper prefix of j; and equal
// keys with a field of 29 mean the same 29 symbols and rem >= 29 for both, one group.  What is new is equal keys with a field r < 29
// (case (2) with ri == rj): both suffixes are the same r symbols, that is, equal strings, whose order is by string id.  g grows with
// s, the ids went in ascending and the sort is stable: they already stand in that order, each is made a group of its own, and nothing
// with another key can come between them.                                                                                         []
//
// Claim 2 (doubling).  After the round that orders by h symbols, every slot with rem < h is resolved.
// Proof.  h = 29 is claim 1.  Let it hold for h, and take a slot g unresolved after that round, so rem(g) >= h, with rem(g) < 2h.  Its
// next key is (rank[g], rank[g + h]), and slot g + h -- of the same string, since h <= rem(g) -- has rem(g) - h < h symbols left, so
// it is resolved and rank[g + h] is its own row + 1, which no other slot has.  The key is unique: g is resolved after the 2h round. []
// Corollary.  An unresolved slot has rem(g) >= h, so g + h is at most its own string's empty suffix: sufsort_key_kernel never reads
// rank across a string boundary, and its `i + h < n` is the array's bound only.  Equal suffixes come out by string id because the
// ranks of the resolved slots they end in carry claim 1's order by id (at last those of the empty suffixes, rows 0 .. N - 1).
__global__ __launch_bounds__(256) void sufsort_set_key0_kernel(const uint32_t* __restrict__ words, const uint32_t be, const uint64_t n_words,
                                                               const uint64_t* __restrict__ begin, const uint64_t* __restrict__ cum,
                                                               const uint32_t* __restrict__ string_ids, const uint64_t n,
                                                               uint64_t* __restrict__ keys, uint32_t* __restrict__ ids)
{
    const uint64_t g = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    if (g >= n) return;
    const uint32_t sid = string_ids[g];
    const uint64_t first = sid ? cum[sid - 1u] : 0u;
    const uint64_t rem = cum[sid] - 1u - g;                            // len - p
    const uint64_t at = begin[sid] + (g - first);
    const uint64_t w = at >> 4;
    const uint32_t o = 2u * uint32_t(at & 15u);
    const uint64_t hi = (uint64_t(ss_word_be(words, w, n_words, be)) << 32) | ss_word_be(words, w + 1u, n_words, be);
    const uint64_t lo = ss_word_be(words, w + 2u, n_words, be);
    uint64_t v = o ? ((hi << o) | (lo >> (32u - o))) : hi;
    if (rem == 0u) v = 0u;
    else if (rem < SS_K0) v &= ~0ull << (64u - 2u * uint32_t(rem));
    keys[g] = (v & ~63ull) | (rem < SS_K0 ? rem : uint64_t(SS_K0));
    ids[g]  = uint32_t(g);
}

// the row of each string's whole suffix (p == 0: where the BWT holds '$') and the string, to be sorted by row: rank = row + 1 at the end
__global__ __launch_bounds__(256) void sufsort_set_dollars_kernel(const uint64_t* __restrict__ cum, const uint32_t* __restrict__ rank, const uint64_t n_strings,
                                                                  uint32_t* __restrict__ rows, uint32_t* __restrict__ ids)
{
    const uint64_t s = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    if (s >= n_strings) return;
    rows[s] = rank[s ? cum[s - 1u] : 0u] - 1u;
    ids[s]  = uint32_t(s);
}

// bwt[row] = the symbol before the slot on that row, 255 where it is a whole string.  A lane owns four rows -- one 32-bit word of the
// output -- and issues each stage's four loads (row -> slot -> string -> first slot and begin -> symbol) before it uses the first.
// Rows past the end take slot 0, a whole string, and read no symbol.
__global__ __launch_bounds__(256) void sufsort_set_bwt_kernel(const uint32_t* __restrict__ words, const uint32_t be, const uint64_t* __restrict__ begin,
                                                              const uint64_t* __restrict__ cum, const uint32_t* __restrict__ string_ids,
                                                              const uint32_t* __restrict__ sa, const uint64_t n, uint8_t* __restrict__ bwt_out,
                                                              uint32_t* __restrict__ pairs_out, const uint32_t word_stores)
{
    const uint64_t w = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    const uint64_t row0 = w * 4u;
    if (row0 >= n) return;
    uint32_t g[4], sid[4], sym[4];
    uint64_t first[4], beg[4];
    #pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) g[q] = row0 + q < n ? sa[row0 + q] : 0u;
    #pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) sid[q] = string_ids[g[q]];
    #pragma unroll
    for (uint32_t q = 0; q < 4u; ++q)
    {
        first[q] = cum[sid[q] ? sid[q] - 1u : 0u];
        beg[q]   = begin[sid[q]];
    }
    #pragma unroll
    for (uint32_t q = 0; q < 4u; ++q)
    {
        if (sid[q] == 0u) first[q] = 0u;
        const uint64_t p = g[q] - first[q];
        sym[q] = p ? ss_symbol(words, be, beg[q] + p - 1u) : 255u;
        g[q] = uint32_t(p);
    }
    if (word_stores && row0 + 4u <= n) reinterpret_cast<uint32_t*>(bwt_out)[w] = sym[0] | (sym[1] << 8) | (sym[2] << 16) | (sym[3] << 24);
    else
    {
        #pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) if (row0 + q < n) bwt_out[row0 + q] = uint8_t(sym[q]);
    }
    if (pairs_out)
    {
        #pragma unroll
        for (uint32_t q = 0; q < 4u; ++q)
            if (row0 + q < n) { pairs_out[2u * (row0 + q)] = g[q]; pairs_out[2u * (row0 + q) + 1u] = sid[q]; }
    }
}

// rocPRIM's scratch for a set call: the sorter's, the scan of N lengths and the sort of N '$' rows
static uint64_t ss_set_prim_bytes(uint64_t n, uint64_t n_strings)
{
    size_t scan = 0, sort = 0;
    (void)rocprim::inclusive_scan(nullptr, scan, ss_len1_iterator((const uint32_t*)nullptr, ss_len1()), (uint64_t*)nullptr, size_t(n_strings), rocprim::plus<uint64_t>());
    rocprim::double_buffer<uint32_t> k(nullptr, nullptr), v(nullptr, nullptr);
    (void)rocprim::radix_sort_pairs(nullptr, sort, k, v, size_t(n_strings), 0u, 32u);
    return std::max<uint64_t>(ss_prim_bytes(n), ss_align(std::max<uint64_t>(scan, sort)) + 256u);
}

static inline bool ss_set_counts_ok(uint64_t n, uint64_t n_strings) { return n_strings >= 1u && n_strings <= n && n <= SS_MAX_N; }

// temp layout of a set call: the sorter's seven arrays over n slots | string_ids (4 n) | cum as 64-bit sums (8 N) | rocPRIM's scratch
static inline uint64_t ss_set_fixed_bytes(uint64_t n, uint64_t n_strings) { return ss_fixed_bytes(n) + ss_align(n * 4u) + ss_align(n_strings * 8u); }

static int ss_set_check(const nvbio_hip_string_set* set, uint32_t n_strings, uint64_t n)
{
    if (!set || !set->words || !set->begin || set->bits != 2u) return hipErrorInvalidValue;
    if (!ss_set_counts_ok(n, n_strings)) return hipErrorInvalidValue;
    if (!set->length && uint64_t(n_strings) * (uint64_t(set->fixed_length) + 1u) != n) return hipErrorInvalidValue;
    return hipSuccess;
}

struct ss_set_arrays { uint32_t* rank; uint32_t* string_ids; uint64_t* cum; ss_buffers bufs; void* prim; size_t prim_bytes; };

// sa_rows[row] = the global index of the slot on that row.  With a length array the lengths' sum is known only on the device: round 0
// runs on the n the caller gave, inside the scratch that n sized -- every index below is bounded by n, N or n_words whatever the
// lengths hold -- and its last kernel, the first to write outside the scratch, writes nothing unless the sum is n
// (sufsort_update_kernel<true>).  The sum comes to the host with round 0's wait, and a wrong n returns there.
static int ss_set_sort(const nvbio_hip_string_set* set, uint32_t n_strings, uint64_t n, uint32_t* sa_rows, ss_set_arrays* out,
                       void* temp, uint64_t temp_bytes, hipStream_t s)
{
    const ss_buffers bufs = ss_carve(temp, n);
    uint8_t* p = bufs.end;
    uint32_t* string_ids = reinterpret_cast<uint32_t*>(p);   p += ss_align(n * 4u);
    uint64_t* cum        = reinterpret_cast<uint64_t*>(p);   p += ss_align(uint64_t(n_strings) * 8u);
    void* prim = p;
    size_t prim_bytes = size_t(temp_bytes - uint64_t(p - reinterpret_cast<uint8_t*>(temp)));
    out->rank = bufs.rank; out->string_ids = string_ids; out->cum = cum; out->bufs = bufs; out->prim = prim; out->prim_bytes = prim_bytes;
    const dim3 block(256);

    if (set->length)
    {
        if (hipError_t e = rocprim::inclusive_scan(prim, prim_bytes, ss_len1_iterator(set->length, ss_len1()), cum, size_t(n_strings), rocprim::plus<uint64_t>(), s)) return e;
    }
    else
    {
        hipLaunchKernelGGL(sufsort_set_cum_fixed_kernel, dim3(ss_blocks(n_strings)), block, 0, s, uint64_t(n_strings), uint64_t(set->fixed_length) + 1u, cum);
        if (hipError_t e = hipGetLastError()) return e;
    }
    if (hipError_t e = hipMemsetAsync(string_ids, 0, n * 4u, s)) return e;
    hipLaunchKernelGGL(sufsort_set_first_slots_kernel, dim3(ss_blocks(n_strings)), block, 0, s, cum, uint64_t(n_strings), n, string_ids);
    if (hipError_t e = hipGetLastError()) return e;
    if (hipError_t e = rocprim::inclusive_scan(prim, prim_bytes, string_ids, string_ids, size_t(n), rocprim::maximum<uint32_t>(), s)) return e;

    g_last_kernel = "sufsort_set_key0_kernel";
    hipLaunchKernelGGL(sufsort_set_key0_kernel, dim3(ss_blocks(n)), block, 0, s, set->words, set->big_endian ? 1u : 0u, set->n_words, set->begin, cum,
                       string_ids, n, bufs.keysA, bufs.idsA);
    if (hipError_t e = hipGetLastError()) return e;
    return ss_rounds<true>(bufs, n, sa_rows, prim, prim_bytes, s, set->length ? cum + (n_strings - 1u) : nullptr);
}

// the two by-products a caller may ask for, out of the scratch
static int ss_set_copy_out(const ss_set_arrays& a, uint32_t n_strings, uint64_t n, uint32_t* string_ids_out, uint32_t* cum_lengths_out, hipStream_t s)
{
    if (string_ids_out)
        if (hipError_t e = hipMemcpyAsync(string_ids_out, a.string_ids, n * 4u, hipMemcpyDeviceToDevice, s)) return e;
    if (cum_lengths_out)
    {
        hipLaunchKernelGGL(sufsort_set_cum32_kernel, dim3(ss_blocks(n_strings)), dim3(256), 0, s, a.cum, uint64_t(n_strings), cum_lengths_out);
        if (hipError_t e = hipGetLastError()) return e;
    }
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

NVB_API uint64_t nvbio_hip_suffix_sort_bytes_temp_bytes(uint64_t n) { return nvbio_hip_suffix_sort_temp_bytes(n); }

NVB_API int nvbio_hip_suffix_sort_bytes(const uint8_t* symbols, uint32_t symbol_size, uint64_t n, uint32_t* sa_out, void* temp, uint64_t temp_bytes, void* stream)
{
    if (int e = ss_bytes_check(symbols, symbol_size, n)) return e;
    if (!sa_out || !temp || temp_bytes < nvbio_hip_suffix_sort_bytes_temp_bytes(n)) return hipErrorInvalidValue;
    uint32_t* rank = nullptr;
    return ss_bytes_sort(symbols, symbol_size, n, sa_out, &rank, temp, temp_bytes, to_stream(stream));
}

NVB_API uint64_t nvbio_hip_bwt_bytes_temp_bytes(uint64_t n) { return nvbio_hip_bwt_temp_bytes(n); }

NVB_API int nvbio_hip_bwt_bytes(const uint8_t* symbols, uint32_t symbol_size, uint64_t n, uint32_t sa_int, uint8_t* bwt_out, uint32_t* primary_out,
                                uint32_t* ssa_out, uint32_t* sa_out, void* temp, uint64_t temp_bytes, void* stream)
{
    if (int e = ss_bytes_check(symbols, symbol_size, n)) return e;
    if (!bwt_out || !primary_out || (ssa_out && sa_int == 0u)) return hipErrorInvalidValue;
    if (!temp || temp_bytes < nvbio_hip_bwt_bytes_temp_bytes(n)) return hipErrorInvalidValue;
    hipStream_t s = to_stream(stream);
    uint8_t* p = reinterpret_cast<uint8_t*>(temp);
    uint32_t* sa = sa_out ? sa_out : reinterpret_cast<uint32_t*>(p);
    p += ss_align((n + 1u) * 4u);
    uint32_t* rank = nullptr;
    if (int e = ss_bytes_sort(symbols, symbol_size, n, sa, &rank, p, temp_bytes - ss_align((n + 1u) * 4u), s)) return e;
    g_last_kernel = "sufsort_bytes_bwt_kernel";
    const uint32_t word_stores = (reinterpret_cast<uintptr_t>(bwt_out) & 3u) == 0u ? 1u : 0u;
    hipLaunchKernelGGL(sufsort_bytes_bwt_kernel, dim3(ss_blocks((n + 3u) / 4u)), dim3(256), 0, s, symbols, (1u << symbol_size) - 1u, n, sa, rank, bwt_out, word_stores);
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

NVB_API uint64_t nvbio_hip_set_suffix_sort_temp_bytes(uint64_t n_suffixes, uint32_t n_strings)
{
    if (!ss_set_counts_ok(n_suffixes, n_strings)) return 256u;
    return ss_set_fixed_bytes(n_suffixes, n_strings) + ss_set_prim_bytes(n_suffixes, n_strings);
}

NVB_API int nvbio_hip_set_suffix_sort(const nvbio_hip_string_set* set, uint32_t n_strings, uint64_t n_suffixes, uint32_t* suffixes_out,
                                      uint32_t* string_ids_out, uint32_t* cum_lengths_out, void* temp, uint64_t temp_bytes, void* stream)
{
    if (int e = ss_set_check(set, n_strings, n_suffixes)) return e;
    if (!suffixes_out || !temp || temp_bytes < nvbio_hip_set_suffix_sort_temp_bytes(n_suffixes, n_strings)) return hipErrorInvalidValue;
    hipStream_t s = to_stream(stream);
    ss_set_arrays a;
    if (int e = ss_set_sort(set, n_strings, n_suffixes, suffixes_out, &a, temp, temp_bytes, s)) return e;
    if (int e = ss_set_copy_out(a, n_strings, n_suffixes, string_ids_out, cum_lengths_out, s)) return e;
    return hipStreamSynchronize(s);
}

NVB_API uint64_t nvbio_hip_set_bwt_temp_bytes(uint64_t n_suffixes, uint32_t n_strings)
{
    if (!ss_set_counts_ok(n_suffixes, n_strings)) return 256u;
    return ss_align(n_suffixes * 4u) + nvbio_hip_set_suffix_sort_temp_bytes(n_suffixes, n_strings);       // the sorted slots, then the sorter's
}

NVB_API int nvbio_hip_set_bwt(const nvbio_hip_string_set* set, uint32_t n_strings, uint64_t n_suffixes, uint8_t* bwt_out,
                              uint32_t* dollar_rows_out, uint32_t* dollar_ids_out, uint32_t* suffixes_out, void* temp, uint64_t temp_bytes, void* stream)
{
    if (int e = ss_set_check(set, n_strings, n_suffixes)) return e;
    if (!bwt_out || !dollar_rows_out || !dollar_ids_out) return hipErrorInvalidValue;
    if (!temp || temp_bytes < nvbio_hip_set_bwt_temp_bytes(n_suffixes, n_strings)) return hipErrorInvalidValue;
    hipStream_t s = to_stream(stream);
    const uint64_t n = n_suffixes;
    uint32_t* sa = reinterpret_cast<uint32_t*>(temp);
    uint8_t* rest = reinterpret_cast<uint8_t*>(temp) + ss_align(n * 4u);
    ss_set_arrays a;
    if (int e = ss_set_sort(set, n_strings, n, sa, &a, rest, temp_bytes - ss_align(n * 4u), s)) return e;
    g_last_kernel = "sufsort_set_bwt_kernel";
    const uint32_t word_stores = (reinterpret_cast<uintptr_t>(bwt_out) & 3u) == 0u ? 1u : 0u;
    hipLaunchKernelGGL(sufsort_set_bwt_kernel, dim3(ss_blocks((n + 3u) / 4u)), dim3(256), 0, s, set->words, set->big_endian ? 1u : 0u, set->begin, a.cum,
                       a.string_ids, sa, n, bwt_out, suffixes_out, word_stores);
    if (hipError_t e = hipGetLastError()) return e;
    // the '$' rows: the row of every string's whole suffix, sorted, with the string.  The sorter's key arrays are free by now; the four
    // arrays of N words (16 N bytes) start in keysA (8 n bytes) and, when N > n / 2, run on into keysB: ss_carve lays keysA | keysB out
    // next to each other, and this relies on it
    uint32_t* d = reinterpret_cast<uint32_t*>(a.bufs.keysA);
    const uint64_t N = n_strings;
    hipLaunchKernelGGL(sufsort_set_dollars_kernel, dim3(ss_blocks(N)), dim3(256), 0, s, a.cum, a.rank, N, d, d + 2u * N);
    if (hipError_t e = hipGetLastError()) return e;
    rocprim::double_buffer<uint32_t> rows(d, d + N), ids(d + 2u * N, d + 3u * N);
    if (hipError_t e = rocprim::radix_sort_pairs(a.prim, a.prim_bytes, rows, ids, size_t(N), 0u, 64u - uint32_t(__builtin_clzll(n)), s)) return e;
    if (hipError_t e = hipMemcpyAsync(dollar_rows_out, rows.current(), N * 4u, hipMemcpyDeviceToDevice, s)) return e;
    if (hipError_t e = hipMemcpyAsync(dollar_ids_out, ids.current(), N * 4u, hipMemcpyDeviceToDevice, s)) return e;
    return hipStreamSynchronize(s);
}
