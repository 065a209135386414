// wavelet.hip -- the wavelet tree of a byte text (1 to 8 bits a symbol) and an FM-index over the wavelet tree of a BWT: the reference's
// nvbio/strings/wavelet_tree.h (setup, text, rank; wavelet_tree_inl.h:128-497) and fm_index<WaveletTree, ..>'s match and locate
// (nvbio/fmindex/fmindex_inl.h:36-99, 307-341, 471-501).  DESIGN.md 3.15.
//
// Layout, the reference's bit for bit.  n = size, S = symbol_size, K = 2^S, W = ceil(n S / 32).
//   bits[W]     a big-endian 1-bit stream: global bit g is bit 31 - g % 32 of word g / 32, zero padded.  Level l is bits [l n, (l + 1) n):
//               bit S - 1 - l of the symbols after a stable sort by their top l bits.
//   splits[K]   a heap of internal nodes: node j of level l has index 2^l - 1 + j and covers the symbols [j K / 2^l, (j + 1) K / 2^l);
//               splits[node] = the text symbols smaller than the node's middle symbol.  splits[K - 1] = 0.
//   occ[K + W]  occ[node] = the 1 bits of the stream before bit l n + (the text symbols smaller than the node's first symbol),
//               occ[K - 1] = 0; occ[K + w] = the 1 bits before word w.
//
// The node table needs no walk and no bits.  With C[s] = the text symbols smaller than s: splits[node] = C[middle], and the 1 bits of
// level l inside node (l, j) are the symbols of its upper half, C[end] - C[middle].  The nodes before (l, j) in heap order are the whole
// levels above and the nodes left of it on its own level -- exactly the bits before its first one -- so occ[node] is the exclusive sum
// of those counts over the heap index.
//
// A query is one lane walking S levels; a level costs two dependent 4-byte reads, occ[K + w] and bits[w], issued before either is
// used; splits[0 .. K - 1) and occ[0 .. K - 1) are staged into LDS once per block.  Positions are carried as exclusive ends r (the
// reference's i + 1), so the walk ends as soon as r is 0 -- an empty node is one case of that -- and the two ends of a range descend
// together, since they take the same path.
#include "common.h"
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
#include <algorithm>

namespace nvb {

static constexpr uint64_t WT_MAX_BITS = 0xFFFFFFFFull;      // n S: a global bit index is a uint32

struct WtTree { const uint32_t* bits; const uint32_t* splits; const uint32_t* occ; uint32_t S, n; };

struct WtFmi
{
    WtTree t;
    const uint32_t* L2;
    const uint32_t* ssa;
    uint32_t length, primary, sa_int;
};

struct WtStrings { const uint8_t* symbols; uint64_t n_symbols; const uint64_t* begin; const uint32_t* length; uint32_t fixed_length; };

// ---- setup

__global__ __launch_bounds__(256) void wavelet_hist_kernel(const uint8_t* __restrict__ symbols, const uint32_t mask, const uint64_t n, uint32_t* __restrict__ hist)
{
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0u;
    __syncthreads();
    for (uint64_t i = uint64_t(blockIdx.x) * 256u + threadIdx.x; i < n; i += uint64_t(gridDim.x) * 256u) atomicAdd(&h[symbols[i] & mask], 1u);
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}

// one block: splits[0 .. K) and occ[0 .. K) from the histogram (the closed form at the top of the file)
__global__ __launch_bounds__(256) void wavelet_nodes_kernel(const uint32_t* __restrict__ hist, const uint32_t S, uint32_t* __restrict__ splits, uint32_t* __restrict__ occ)
{
    __shared__ uint32_t C[257];
    __shared__ uint32_t ones[256];
    const uint32_t K = 1u << S, t = threadIdx.x;
    if (t == 0u)
    {
        uint32_t sum = 0u;
        for (uint32_t c = 0; c < K; ++c) { C[c] = sum; sum += hist[c]; }
        C[K] = sum;
    }
    __syncthreads();
    uint32_t split = 0u, one = 0u;
    if (t + 1u < K)
    {
        const uint32_t l = 31u - uint32_t(__clz(int(t + 1u))), j = t + 1u - (1u << l);
        const uint32_t first = (j * K) >> l, half = K >> (l + 1u);
        split = C[first + half];
        one   = C[first + 2u * half] - split;
    }
    ones[t] = one;
    __syncthreads();
    if (t == 0u)
    {
        uint32_t sum = 0u;
        for (uint32_t k = 0; k < K; ++k) { const uint32_t v = ones[k]; ones[k] = sum; sum += v; }
    }
    __syncthreads();
    if (t < K) { splits[t] = split; occ[t] = t + 1u < K ? ones[t] : 0u; }
}

// One level's bit plane: a lane takes one global bit from the word the level starts in, a wave's ballot is two finished words.  A level
// that starts inside a word ORs its first word into what the level before stored there (the launches of a setup are ordered by the
// stream, and one lane of one launch owns a word); every other word is stored whole, so the stream needs no clearing.
__global__ __launch_bounds__(256) void wavelet_plane_kernel(const uint8_t* __restrict__ syms, const uint32_t bit, const uint64_t n, const uint64_t off, uint32_t* __restrict__ bits)
{
    const uint64_t g = (off & ~31ull) + uint64_t(blockIdx.x) * 256u + threadIdx.x;
    const uint64_t end = off + n;
    uint32_t b = 0u;
    if (g >= off && g < end) b = (uint32_t(syms[g - off]) >> bit) & 1u;
    const uint64_t m = __ballot(b);
    const uint32_t lane = threadIdx.x & 63u;
    if ((lane & 31u) == 0u && g < end)
    {
        const uint32_t v = __brev(uint32_t(lane ? (m >> 32) : m));      // lane k of a half holds bit 31 - k of the word
        if (g < off) bits[g >> 5] |= v; else bits[g >> 5] = v;
    }
}

struct wt_popc { __host__ __device__ uint32_t operator()(const uint32_t w) const { return uint32_t(__builtin_popcount(w)); } };
typedef rocprim::transform_iterator<const uint32_t*, wt_popc, uint32_t> wt_popc_iterator;

static inline uint64_t wt_align(uint64_t x) { return (x + 255ull) & ~255ull; }
static inline uint32_t wt_blocks(uint64_t items, uint32_t per_block = 256u) { return uint32_t((items + per_block - 1u) / per_block); }

// what rocPRIM asks for the sorts and the scan of a setup, queried with the very calls the setup makes
static uint64_t wt_prim_bytes(uint64_t n, uint32_t S, uint64_t n_words)
{
    size_t sort = 0, scan = 0;
    for (uint32_t l = 1; l < S; ++l)
    {
        size_t one = 0;
        (void)rocprim::radix_sort_keys(nullptr, one, (const uint8_t*)nullptr, (uint8_t*)nullptr, size_t(n), S - l, S);
        sort = std::max(sort, one);
    }
    (void)rocprim::exclusive_scan(nullptr, scan, wt_popc_iterator((const uint32_t*)nullptr, wt_popc()), (uint32_t*)nullptr, 0u, size_t(n_words), rocprim::plus<uint32_t>());
    return wt_align(std::max<uint64_t>(sort, scan)) + 256u;
}

static inline bool wt_size_ok(uint64_t n, uint32_t S) { return S >= 1u && S <= 8u && n >= 1u && n * S <= WT_MAX_BITS; }

// ---- queries

#define WT_STAGE(t)                                                                                                     \
    __shared__ uint32_t s_split[256];                                                                                   \
    __shared__ uint32_t s_occ[256];                                                                                     \
    if (threadIdx.x < (1u << (t).S)) { s_split[threadIdx.x] = (t).splits[threadIdx.x]; s_occ[threadIdx.x] = (t).occ[threadIdx.x]; } \
    __syncthreads();

// rank of symbol c at the exclusive ends rx, ry (<= n) of one path: rx, ry become the counts of c in [0, rx), [0, ry)
__device__ __forceinline__ void wt_rank_pair(const WtTree& t, const uint32_t* __restrict__ occw, const uint32_t* s_split, const uint32_t* s_occ,
                                             const uint32_t c, uint32_t& rx, uint32_t& ry)
{
    uint32_t node = 0u, lo = 0u;
    for (uint32_t l = 0; l < t.S; ++l)
    {
        if ((rx | ry) == 0u) break;
        const uint32_t gx = l * t.n + lo + rx - 1u, gy = l * t.n + lo + ry - 1u;       // the last bit of each prefix (unused where r is 0)
        uint32_t cx = 0u, wx = 0u, cy = 0u, wy = 0u;
        if (rx) { cx = occw[gx >> 5]; wx = t.bits[gx >> 5]; }
        if (ry) { cy = occw[gy >> 5]; wy = t.bits[gy >> 5]; }
        const uint32_t b = (c >> (t.S - 1u - l)) & 1u, base = s_occ[node];
        if (rx) { const uint32_t ones = cx + uint32_t(__popc(wx >> (31u - (gx & 31u)))) - base; rx = b ? ones : rx - ones; }
        if (ry) { const uint32_t ones = cy + uint32_t(__popc(wy >> (31u - (gy & 31u)))) - base; ry = b ? ones : ry - ones; }
        if (b) lo = s_split[node];
        node = 2u * node + 1u + b;
    }
}

// the symbol at position i < n; r_out = the count of that symbol in [0, i)
__device__ __forceinline__ uint32_t wt_text_walk(const WtTree& t, const uint32_t* __restrict__ occw, const uint32_t* s_split, const uint32_t* s_occ,
                                                 const uint32_t i, uint32_t& r_out)
{
    uint32_t node = 0u, lo = 0u, r = i, c = 0u;
    for (uint32_t l = 0; l < t.S; ++l)
    {
        const uint32_t g = l * t.n + lo + r, m = g & 31u;
        const uint32_t cw = occw[g >> 5], wd = t.bits[g >> 5];
        const uint32_t b = (wd >> (31u - m)) & 1u;
        const uint32_t ones = cw + (m ? uint32_t(__popc(wd >> (32u - m))) : 0u) - s_occ[node];     // the 1 bits of the node before g
        r = b ? ones : r - ones;
        c = (c << 1) | b;
        if (b) lo = s_split[node];
        node = 2u * node + 1u + b;
    }
    r_out = r;
    return c;
}

// QPL independent queries a lane, all loads of a level issued together (as sufsort_key_kernel does)
template <uint32_t QPL>
__global__ __launch_bounds__(256) void wavelet_rank_kernel(const WtTree t, const uint32_t* __restrict__ positions, const uint8_t* __restrict__ symbols,
                                                           const uint64_t nq, uint32_t* __restrict__ out)
{
    WT_STAGE(t)
    const uint32_t K = 1u << t.S;
    const uint32_t* __restrict__ occw = t.occ + K;
    const uint64_t base = uint64_t(blockIdx.x) * (256u * QPL) + threadIdx.x;
    uint32_t r[QPL], c[QPL], node[QPL], lo[QPL];
    #pragma unroll
    for (uint32_t q = 0; q < QPL; ++q)
    {
        const uint64_t k = base + q * 256u;
        r[q] = c[q] = node[q] = lo[q] = 0u;
        if (k < nq)
        {
            const uint32_t e = positions[k] + 1u;                    // 0xFFFFFFFF wraps to 0: nothing before the text
            r[q] = e > t.n ? t.n : e;                                // the reference clamps a position to the end of its level
            c[q] = symbols[k] & (K - 1u);
        }
    }
    for (uint32_t l = 0; l < t.S; ++l)
    {
        uint32_t any = 0u;
        #pragma unroll
        for (uint32_t q = 0; q < QPL; ++q) any |= r[q];
        if (any == 0u) break;
        uint32_t g[QPL], cw[QPL], wd[QPL];
        #pragma unroll
        for (uint32_t q = 0; q < QPL; ++q)
        {
            g[q] = l * t.n + lo[q] + r[q] - 1u;
            cw[q] = wd[q] = 0u;
            if (r[q]) { cw[q] = occw[g[q] >> 5]; wd[q] = t.bits[g[q] >> 5]; }
        }
        #pragma unroll
        for (uint32_t q = 0; q < QPL; ++q)
        {
            const uint32_t b = (c[q] >> (t.S - 1u - l)) & 1u;
            if (r[q])
            {
                const uint32_t ones = cw[q] + uint32_t(__popc(wd[q] >> (31u - (g[q] & 31u)))) - s_occ[node[q]];
                r[q] = b ? ones : r[q] - ones;
            }
            if (b) lo[q] = s_split[node[q]];
            node[q] = (2u * node[q] + 1u + b) & 255u;                // past the last level the index is not used
        }
    }
    #pragma unroll
    for (uint32_t q = 0; q < QPL; ++q)
    {
        const uint64_t k = base + q * 256u;
        if (k < nq) out[k] = r[q];
    }
}

__global__ __launch_bounds__(256) void wavelet_rank_range_kernel(const WtTree t, const uint2* __restrict__ ranges, const uint8_t* __restrict__ symbols,
                                                                 const uint64_t nq, uint2* __restrict__ out)
{
    WT_STAGE(t)
    const uint64_t k = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    if (k >= nq) return;
    const uint32_t K = 1u << t.S;
    const uint2 range = ranges[k];
    uint32_t rx = range.x + 1u, ry = range.y + 1u;
    rx = rx > t.n ? t.n : rx;
    ry = ry > t.n ? t.n : ry;
    wt_rank_pair(t, t.occ + K, s_split, s_occ, symbols[k] & (K - 1u), rx, ry);
    out[k] = make_uint2(rx, ry);
}

template <uint32_t QPL>
__global__ __launch_bounds__(256) void wavelet_text_kernel(const WtTree t, const uint32_t* __restrict__ positions, const uint64_t nq, uint8_t* __restrict__ out)
{
    WT_STAGE(t)
    const uint32_t K = 1u << t.S;
    const uint32_t* __restrict__ occw = t.occ + K;
    const uint64_t base = uint64_t(blockIdx.x) * (256u * QPL) + threadIdx.x;
    uint32_t r[QPL], c[QPL], node[QPL], lo[QPL];
    bool live[QPL];
    #pragma unroll
    for (uint32_t q = 0; q < QPL; ++q)
    {
        const uint64_t k = base + q * 256u;
        r[q] = c[q] = node[q] = lo[q] = 0u;
        live[q] = false;
        if (k < nq)
        {
            const uint64_t p = positions ? uint64_t(positions[k]) : k;
            live[q] = p < t.n;                                       // a position past the end gives 0 without a read
            r[q] = live[q] ? uint32_t(p) : 0u;
        }
    }
    for (uint32_t l = 0; l < t.S; ++l)
    {
        uint32_t g[QPL], cw[QPL], wd[QPL];
        #pragma unroll
        for (uint32_t q = 0; q < QPL; ++q)
        {
            g[q] = l * t.n + lo[q] + r[q];
            cw[q] = wd[q] = 0u;
            if (live[q]) { cw[q] = occw[g[q] >> 5]; wd[q] = t.bits[g[q] >> 5]; }
        }
        #pragma unroll
        for (uint32_t q = 0; q < QPL; ++q)
        {
            const uint32_t m = g[q] & 31u;
            const uint32_t b = (wd[q] >> (31u - m)) & 1u;
            const uint32_t ones = cw[q] + (m ? uint32_t(__popc(wd[q] >> (32u - m))) : 0u) - s_occ[node[q]];
            if (live[q]) r[q] = b ? ones : r[q] - ones;
            c[q] = (c[q] << 1) | b;
            if (b) lo[q] = s_split[node[q]];
            node[q] = (2u * node[q] + 1u + b) & 255u;
        }
    }
    #pragma unroll
    for (uint32_t q = 0; q < QPL; ++q)
    {
        const uint64_t k = base + q * 256u;
        if (k < nq) out[k] = uint8_t(c[q]);
    }
}

// ---- the FM-index over the tree of a BWT

// L2[c] = the text symbols smaller than c: symbol c >= 1 is the middle of exactly one node, the one of level S - 1 - ctz(c)
__global__ __launch_bounds__(256) void wavelet_fm_L2_kernel(const WtTree t, uint32_t* __restrict__ L2)
{
    const uint32_t K = 1u << t.S;
    for (uint32_t c = threadIdx.x; c <= K; c += 256u)
    {
        uint32_t v = 0u;
        if (c == K) v = t.n;
        else if (c)
        {
            const uint32_t z = uint32_t(__ffs(int(c))) - 1u, l = t.S - 1u - z;
            v = t.splits[(1u << l) - 1u + (c >> (z + 1u))];
        }
        L2[c] = v;
    }
}

#define WT_STAGE_L2(f)                                                                                                  \
    __shared__ uint32_t s_L2[257];                                                                                      \
    for (uint32_t k_ = threadIdx.x; k_ <= (1u << (f).t.S); k_ += 256u) s_L2[k_] = (f).L2[k_];

// the exclusive end in the BWT (which has no '$') of the rows [0, k] of the matrix: fmindex_inl.h:36-57 with the tree's own clamp
__device__ __forceinline__ uint32_t wt_fm_end(const WtFmi& f, const uint32_t k) { return k == 0xFFFFFFFFu ? 0u : (k >= f.primary ? k : k + 1u); }

__global__ __launch_bounds__(256) void wavelet_fm_match_kernel(const WtFmi f, const WtStrings p, const uint64_t n, uint2* __restrict__ out)
{
    WT_STAGE_L2(f)
    WT_STAGE(f.t)
    const uint64_t id = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    if (id >= n) return;
    const uint32_t K = 1u << f.t.S;
    const uint64_t beg = p.begin[id];
    uint64_t len = p.length ? p.length[id] : p.fixed_length;
    if (beg >= p.n_symbols) len = 0u; else if (len > p.n_symbols - beg) len = p.n_symbols - beg;       // never past the symbols the caller gave
    uint32_t x = 0u, y = f.length;
    for (uint64_t i = len; i-- > 0u && x <= y;)
    {
        const uint32_t c = p.symbols[beg + i];
        if (c >= K) { x = 1u; y = 0u; break; }                       // no such symbol in the alphabet (the reference tests c > K)
        uint32_t rx = wt_fm_end(f, x - 1u), ry = wt_fm_end(f, y);
        wt_rank_pair(f.t, f.t.occ + K, s_split, s_occ, c, rx, ry);
        x = s_L2[c] + rx + 1u;
        y = s_L2[c] + ry;
    }
    out[id] = make_uint2(x, y);
}

__global__ __launch_bounds__(256) void wavelet_fm_locate_kernel(const WtFmi f, const uint32_t* __restrict__ rows, const uint64_t n, uint32_t* __restrict__ out)
{
    WT_STAGE_L2(f)
    WT_STAGE(f.t)
    const uint64_t id = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    if (id >= n) return;
    const uint32_t K = 1u << f.t.S;
    uint32_t j = rows[id], steps = 0u;
    // a row above the length is no row; the two tests inside the loop can fail only on arrays that are no index, and keep such a walk
    // inside them and finite
    while (j <= f.length && j % f.sa_int != 0u && steps <= f.length)
    {
        if (j == f.primary) j = 0u;
        else
        {
            uint32_t r;
            const uint32_t c = wt_text_walk(f.t, f.t.occ + K, s_split, s_occ, j < f.primary ? j : j - 1u, r);
            j = s_L2[c] + r + 1u;                                    // LF: r counts c before the row, the row itself is one more
        }
        ++steps;
    }
    out[id] = (j <= f.length && j % f.sa_int == 0u) ? f.ssa[j / f.sa_int] + steps : 0xFFFFFFFFu;
}

static int wt_check(const nvbio_hip_wavelet_tree* tree)
{
    if (!tree || !tree->bits || !tree->splits || !tree->occ) return hipErrorInvalidValue;
    return wt_size_ok(tree->size, tree->symbol_size) ? hipSuccess : hipErrorInvalidValue;
}
static WtTree wt_make(const nvbio_hip_wavelet_tree* tree)
{
    WtTree t;
    t.bits = tree->bits; t.splits = tree->splits; t.occ = tree->occ; t.S = tree->symbol_size; t.n = tree->size;
    return t;
}
static int wt_fm_check(const nvbio_hip_wavelet_fmindex* fmi)
{
    if (!fmi || !fmi->L2) return hipErrorInvalidValue;
    if (int e = wt_check(&fmi->bwt)) return e;
    if (fmi->length != fmi->bwt.size || fmi->primary == 0u || fmi->primary > fmi->length) return hipErrorInvalidValue;
    return hipSuccess;
}
static WtFmi wt_fm_make(const nvbio_hip_wavelet_fmindex* fmi)
{
    WtFmi f;
    f.t = wt_make(&fmi->bwt); f.L2 = fmi->L2; f.ssa = fmi->ssa; f.length = fmi->length; f.primary = fmi->primary; f.sa_int = fmi->sa_int;
    return f;
}

// queries a lane of the rank and text kernels: NVBIO_HIP_WAVELET_LANES = 1, 2 or 4 picks a form, anything else the kernel's default.
// Measured on 16 M shuffled queries of a 64 M-symbol text (profiles/wavelet/wavelet_time.txt): rank is fastest with 4 a lane at S = 8
// and at S = 5; text with 4 at S = 8 (4 % over 1) and with 1 at S = 5 (10 % over 4), so text keeps 1.
static uint32_t wt_lanes(const uint32_t by_default)
{
    const int sw = test_switch(SW_WAVELET_LANES);
    return (sw == 1 || sw == 2 || sw == 4) ? uint32_t(sw) : by_default;
}

} // namespace nvb

using namespace nvb;

NVB_API uint64_t nvbio_hip_wavelet_setup_temp_bytes(uint64_t n, uint32_t symbol_size)
{
    if (!wt_size_ok(n, symbol_size)) return 256u;
    // the histogram | the sorted symbols | rocPRIM's.  A setup asks again to check its temp_bytes: the last answer is kept, so a run of
    // setups of one shape pays rocPRIM's size queries once
    thread_local uint64_t last_n = 0, last_bytes = 0;
    thread_local uint32_t last_S = 0;
    if (n != last_n || symbol_size != last_S)
    {
        last_bytes = 1024u + wt_align(n) + wt_prim_bytes(n, symbol_size, (n * symbol_size + 31u) / 32u);
        last_n = n; last_S = symbol_size;
    }
    return last_bytes;
}

NVB_API int nvbio_hip_wavelet_setup(const uint8_t* symbols, uint32_t symbol_size, uint64_t n, uint32_t* bits_out, uint32_t* splits_out, uint32_t* occ_out,
                                    void* temp, uint64_t temp_bytes, void* stream)
{
    if (!symbols || !bits_out || !splits_out || !occ_out || !temp) return hipErrorInvalidValue;
    if (!wt_size_ok(n, symbol_size) || temp_bytes < nvbio_hip_wavelet_setup_temp_bytes(n, symbol_size)) return hipErrorInvalidValue;
    hipStream_t s = to_stream(stream);
    const uint32_t S = symbol_size, K = 1u << S;
    const uint64_t n_words = (n * S + 31u) / 32u;
    uint8_t* p = reinterpret_cast<uint8_t*>(temp);
    uint32_t* hist = reinterpret_cast<uint32_t*>(p);   p += 1024u;
    uint8_t* sorted = p;                               p += wt_align(n);
    void* prim = p;
    size_t prim_bytes = size_t(temp_bytes - uint64_t(p - reinterpret_cast<uint8_t*>(temp)));

    if (hipError_t e = hipMemsetAsync(hist, 0, 1024u, s)) return e;
    g_last_kernel = "wavelet_hist_kernel";
    hipLaunchKernelGGL(wavelet_hist_kernel, dim3(std::min<uint32_t>(wt_blocks(n), 2048u)), dim3(256), 0, s, symbols, K - 1u, n, hist);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(wavelet_nodes_kernel, dim3(1), dim3(256), 0, s, hist, S, splits_out, occ_out);
    if (hipError_t e = hipGetLastError()) return e;
    g_last_kernel = "wavelet_plane_kernel";
    for (uint32_t l = 0; l < S; ++l)
    {
        // level l: the text stably sorted by its top l bits.  Every level sorts the text itself, so one buffer serves them all (the
        // bits above S are outside the sorted range and outside the plane's bit: the tree is the masked text's)
        const uint8_t* level = symbols;
        if (l)
        {
            if (hipError_t e = rocprim::radix_sort_keys(prim, prim_bytes, symbols, sorted, size_t(n), S - l, S, s)) return e;
            level = sorted;
        }
        const uint64_t off = uint64_t(l) * n;
        hipLaunchKernelGGL(wavelet_plane_kernel, dim3(wt_blocks(off + n - (off & ~31ull))), dim3(256), 0, s, level, S - 1u - l, n, off, bits_out);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return rocprim::exclusive_scan(prim, prim_bytes, wt_popc_iterator(bits_out, wt_popc()), occ_out + K, 0u, size_t(n_words), rocprim::plus<uint32_t>(), s);
}

NVB_API int nvbio_hip_wavelet_text(const nvbio_hip_wavelet_tree* tree, const uint32_t* positions, uint64_t n_queries, uint8_t* out, void* stream)
{
    if (int e = wt_check(tree)) return e;
    if (n_queries > 0xFFFFFFFFull || (n_queries && !out)) return hipErrorInvalidValue;
    if (n_queries == 0u) return hipSuccess;
    const WtTree t = wt_make(tree);
    hipStream_t s = to_stream(stream);
    g_last_kernel = "wavelet_text_kernel";
    switch (wt_lanes(1u))
    {
        case 2u: hipLaunchKernelGGL(wavelet_text_kernel<2u>, dim3(wt_blocks(n_queries, 512u)),  dim3(256), 0, s, t, positions, n_queries, out); break;
        case 4u: hipLaunchKernelGGL(wavelet_text_kernel<4u>, dim3(wt_blocks(n_queries, 1024u)), dim3(256), 0, s, t, positions, n_queries, out); break;
        default: hipLaunchKernelGGL(wavelet_text_kernel<1u>, dim3(wt_blocks(n_queries, 256u)),  dim3(256), 0, s, t, positions, n_queries, out); break;
    }
    return hipGetLastError();
}

NVB_API int nvbio_hip_wavelet_rank(const nvbio_hip_wavelet_tree* tree, const uint32_t* positions, const uint8_t* symbols, uint64_t n_queries, uint32_t* out, void* stream)
{
    if (int e = wt_check(tree)) return e;
    if (n_queries > 0xFFFFFFFFull || (n_queries && (!positions || !symbols || !out))) return hipErrorInvalidValue;
    if (n_queries == 0u) return hipSuccess;
    const WtTree t = wt_make(tree);
    hipStream_t s = to_stream(stream);
    g_last_kernel = "wavelet_rank_kernel";
    switch (wt_lanes(4u))
    {
        case 1u: hipLaunchKernelGGL(wavelet_rank_kernel<1u>, dim3(wt_blocks(n_queries, 256u)),  dim3(256), 0, s, t, positions, symbols, n_queries, out); break;
        case 2u: hipLaunchKernelGGL(wavelet_rank_kernel<2u>, dim3(wt_blocks(n_queries, 512u)),  dim3(256), 0, s, t, positions, symbols, n_queries, out); break;
        default: hipLaunchKernelGGL(wavelet_rank_kernel<4u>, dim3(wt_blocks(n_queries, 1024u)), dim3(256), 0, s, t, positions, symbols, n_queries, out); break;
    }
    return hipGetLastError();
}

NVB_API int nvbio_hip_wavelet_rank_range(const nvbio_hip_wavelet_tree* tree, const uint32_t* ranges, const uint8_t* symbols, uint64_t n_queries, uint32_t* out, void* stream)
{
    if (int e = wt_check(tree)) return e;
    if (n_queries > 0xFFFFFFFFull || (n_queries && (!ranges || !symbols || !out))) return hipErrorInvalidValue;
    if (n_queries == 0u) return hipSuccess;
    g_last_kernel = "wavelet_rank_range_kernel";
    hipLaunchKernelGGL(wavelet_rank_range_kernel, dim3(wt_blocks(n_queries)), dim3(256), 0, to_stream(stream), wt_make(tree),
                       reinterpret_cast<const uint2*>(ranges), symbols, n_queries, reinterpret_cast<uint2*>(out));
    return hipGetLastError();
}

NVB_API int nvbio_hip_wavelet_fm_L2(const nvbio_hip_wavelet_tree* tree, uint32_t* L2_out, void* stream)
{
    if (int e = wt_check(tree)) return e;
    if (!L2_out) return hipErrorInvalidValue;
    g_last_kernel = "wavelet_fm_L2_kernel";
    hipLaunchKernelGGL(wavelet_fm_L2_kernel, dim3(1), dim3(256), 0, to_stream(stream), wt_make(tree), L2_out);
    return hipGetLastError();
}

NVB_API int nvbio_hip_wavelet_fm_match(const nvbio_hip_wavelet_fmindex* fmi, const nvbio_hip_byte_string_set* patterns, uint64_t n, uint32_t* ranges_out, void* stream)
{
    if (int e = wt_fm_check(fmi)) return e;
    if (!patterns || n > 0xFFFFFFFFull || (n && (!patterns->begin || !ranges_out))) return hipErrorInvalidValue;
    if (n && !patterns->symbols && patterns->n_symbols) return hipErrorInvalidValue;
    if (n == 0u) return hipSuccess;
    WtStrings p;
    p.symbols = patterns->symbols; p.n_symbols = patterns->symbols ? patterns->n_symbols : 0u; p.begin = patterns->begin; p.length = patterns->length;
    p.fixed_length = patterns->fixed_length;
    g_last_kernel = "wavelet_fm_match_kernel";
    hipLaunchKernelGGL(wavelet_fm_match_kernel, dim3(wt_blocks(n)), dim3(256), 0, to_stream(stream), wt_fm_make(fmi), p, n, reinterpret_cast<uint2*>(ranges_out));
    return hipGetLastError();
}

NVB_API int nvbio_hip_wavelet_fm_locate(const nvbio_hip_wavelet_fmindex* fmi, const uint32_t* rows, uint64_t n_rows, uint32_t* positions_out, void* stream)
{
    if (int e = wt_fm_check(fmi)) return e;
    if (!fmi->ssa || fmi->sa_int == 0u) return hipErrorInvalidValue;
    if (n_rows > 0xFFFFFFFFull || (n_rows && (!rows || !positions_out))) return hipErrorInvalidValue;
    if (n_rows == 0u) return hipSuccess;
    g_last_kernel = "wavelet_fm_locate_kernel";
    hipLaunchKernelGGL(wavelet_fm_locate_kernel, dim3(wt_blocks(n_rows)), dim3(256), 0, to_stream(stream), wt_fm_make(fmi), rows, n_rows, positions_out);
    return hipGetLastError();
}
