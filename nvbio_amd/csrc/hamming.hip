// hamming.hip -- ungapped ("Hamming") scoring for gfx950: HammingDistanceAligner<TYPE, scheme, PatternBlockingTag>
// (nvbio/alignment/hamming/hamming_inl.h:413-720; nvBowtie's --ungapped-mates, score_paired.cu:110-137).
//
//   H(i,j) = H(i-1,j-1) + (text[i] == pattern[j] ? match : mismatch[q_j]),  every border zero, LOCAL clamped at zero.
//
// A cell depends on its diagonal neighbour alone, so nothing passes between lanes.  One wave scores one job, in the reference's own
// block order (which keeps its early exit and the sink it freezes):
//
//   for each 16-column pattern block                    16 symbols and 16 penalties, wave-uniform, in scalar registers
//     for each pass of 64 text rows, LAST pass first      lane = the diagonal segment that enters the block at row i0
//       h = column[i0 - 1]                                 the reference's int16 boundary column, in LDS
//       16 cells straight down the diagonal               bfe, cmp, cndmask, add (+ max, shift-add, max for LOCAL)
//       column[i0 + 15] = int16(h)
//     exit test on the wave's maximum of the block's right edge
//
// Walking the passes downwards lets the column be updated in place: a pass reads entries [64p - 17, 64p + 47] and writes
// [64p, 64p + 63]; the pass below it reads nothing at or above 64p - 16, the pass above it wrote nothing below 64p + 64.
// Sixteen entries in front of the column stay zero: the left border for the segments that start above the text.
//
// LOCAL finds its cell with one packed maximum per cell, (h << 4 | k): the LAST of equal scores along a segment, which is the one
// BestSink keeps (it replaces on <=); segments are then compared by (score, block, row, column).  Passes next to the text's ends and
// the pattern's last, partial block take a checked form of the same 16 cells.
#include "common.h"
#include <algorithm>

namespace nvb {

struct HammingParams {
    StringSet       pat, txt;
    int32_t         match;
    const int32_t*  min_score;         // nullable: -(1 << 30) for every job
    uint32_t        n;
    int32_t*        out_score;
    uint32_t*       out_sink;
    uint8_t*        out_ok;            // nullable
    const uint8_t*  quals; uint64_t n_quals;      // nullptr: every mismatch costs mm_lut[0]
    uint32_t        m_pad;             // max_pattern_len rounded up to 16 (>= 16)
    uint32_t        txt_words;         // LDS words of the staged text window
    uint32_t        max_n;
    // job control, as FullParams has it (full_gotoh.hip)
    const uint32_t* n_dev; const uint32_t* job_index; const uint32_t* gate; uint32_t gate_limit, gate_above;
    int32_t         mm_lut[256];
};

// LDS of one job: penalties int32[m_pad] | pattern nibbles uint32[m_pad / 8] | text uint32[txt_words] | column int16[16 + 64 * passes]
__host__ __device__ inline uint32_t hamming_passes(uint32_t N)     { return (N + 15u + 63u) / 64u; }
// (the last pass's lanes start at rows up to 64 * passes - 16, at most 15 symbols into the window's first word: words 0 .. 4 * passes)
__host__ __device__ inline uint32_t hamming_txt_words(uint32_t N)  { return 4u * hamming_passes(N) + 2u; }
inline uint64_t hamming_lds_bytes(uint32_t m_pad, uint32_t maxN)
{
    return 4ull * m_pad + m_pad / 2u + 4ull * hamming_txt_words(maxN) + 2ull * (16u + 64u * hamming_passes(maxN));
}

__device__ __forceinline__ int32_t uniform(int32_t v) { return __builtin_amdgcn_readfirstlane(v); }

struct HamBest { int32_t score; uint32_t hi, lo; };       // hi = block, lo = (row + 1) << 5 | (column in block + 1): larger = reported later; lo == 0: nothing yet
__device__ __forceinline__ void ham_report(HamBest& b, const int32_t s, const uint32_t hi, const uint32_t lo)
{
    // BestSink::report replaces on <=: of equal scores the one later in the report order stays
    const bool later = hi > b.hi || (hi == b.hi && lo > b.lo);
    if (s > b.score || (s == b.score && later)) { b.score = s; b.hi = hi; b.lo = lo; }
}

// 16 cells down one diagonal segment.  sc[k]: the block's mismatch scores; pg: its symbols as nibbles; tg: the lane's 16 text symbols.
// CHECKED: rows outside [0, N) and columns past M are computed but not reported, and h is held at the zero border above the text.
template <int TYPE, bool CHECKED>
__device__ __forceinline__ void ham_segment(int32_t& h, int32_t& comb, int32_t& h_last, const uint32_t tg, const uint64_t pg, const int32_t (&sc)[16],
                                            const int32_t match, const int32_t i0, const uint32_t N, const uint32_t cols, const uint32_t k_last)
{
    #pragma unroll
    for (int k = 0; k < 16; ++k)
    {
        const uint32_t c = (tg >> (2 * k)) & 3u, q = uint32_t(pg >> (4 * k)) & 15u;
        h += (c == q) ? match : sc[k];
        if (TYPE == NVBIO_HIP_LOCAL) h = max(h, 0);
        if (CHECKED)
        {
            const int32_t row = i0 + k;
            if (row < 0) h = 0;
            const bool valid = uint32_t(row) < N && uint32_t(k) < cols;
            if (TYPE == NVBIO_HIP_LOCAL) comb = max(comb, valid ? int32_t((uint32_t(h) << 4) | uint32_t(k)) : -1);
            else if (uint32_t(k) == k_last) h_last = h;
        }
        else if (TYPE == NVBIO_HIP_LOCAL) comb = max(comb, int32_t((uint32_t(h) << 4) | uint32_t(k)));
    }
}

// BIG: a working set past the 64 KB a launch may ask for dynamically -- the instance declares the CU's whole LDS (one job per CU at a time)
constexpr uint32_t HAMMING_LDS_MAX = 160u * 1024u, HAMMING_LDS_DYNAMIC = 64u * 1024u;
template <int TYPE, bool BIG>
__global__ __launch_bounds__(64) void hamming_score_kernel(const HammingParams p)
{
    extern __shared__ uint32_t ham_dynamic[];
    uint32_t* ham_lds = ham_dynamic;
    if constexpr (BIG) { __shared__ uint32_t ham_static[HAMMING_LDS_MAX / 4u]; ham_lds = ham_static; }
    const uint32_t lane = threadIdx.x;
    if (p.gate != nullptr && ((*p.gate > p.gate_limit) != (p.gate_above != 0u))) return;
    const uint32_t entry = blockIdx.x;
    if (entry >= (p.n_dev ? min(*p.n_dev, p.n) : p.n)) return;
    const uint32_t job = p.job_index ? p.job_index[entry] : entry;

    // (lengths beyond the bounds the LDS was sized for are a caller's error: clamped, so that nothing is written past it)
    const uint32_t M = min(p.pat.length ? p.pat.length[job] : p.pat.fixed_length, p.m_pad);
    const uint32_t N = min(p.txt.length ? p.txt.length[job] : p.txt.fixed_length, p.max_n);
    const uint64_t pb = p.pat.begin[job], tb = p.txt.begin[job];

    int32_t*  pen  = reinterpret_cast<int32_t*>(ham_lds);
    uint32_t* psym = ham_lds + p.m_pad;
    uint32_t* txt  = psym + p.m_pad / 8u;
    int16_t*  col  = reinterpret_cast<int16_t*>(txt + p.txt_words);

    const uint32_t n_blocks = M > 16u ? (M + 15u) / 16u : 1u;
    const uint32_t passes   = hamming_passes(N);

    // stage the job: a score per pattern position, the pattern as nibbles, the text window in canonical order, the zero border
    for (uint32_t j = lane; j < 16u * n_blocks; j += 64u)
        pen[j] = (j < M) ? (p.quals ? p.mm_lut[p.quals[min(pb + j, p.n_quals - 1u)]] : p.mm_lut[0]) : 0;
    for (uint32_t b = lane; b < n_blocks; b += 64u)
    {
        const uint64_t g = fetch_pattern16(p.pat.s, pb + 16u * b);
        psym[2u * b] = uint32_t(g); psym[2u * b + 1u] = uint32_t(g >> 32);
    }
    const uint32_t t_off = uint32_t(tb) & 15u;
    for (uint32_t w = lane; w < hamming_txt_words(N); w += 64u)
    {
        const uint32_t x = ld_word_global(p.txt.s, (tb >> 4) + w);
        txt[w] = p.txt.s.big_endian ? rev2(x) : x;
    }
    if (lane < 16u) col[lane] = 0;
    __syncthreads();

    const int32_t min_score = p.min_score ? p.min_score[job] : -(1 << 30);     // no threshold: Field_traits<int32>::min(), as the host twin passes
    HamBest best = { -(1 << 30), 0u, 0u };
    bool exited = false;

    for (uint32_t b = 0; b < n_blocks; ++b)
    {
        const bool     last   = (b + 1u == n_blocks);
        const uint32_t cols   = min(16u, M - min(M, 16u * b));                  // columns of this block inside the pattern
        const uint32_t k_last = (M - 1u) & 15u;                                 // the pattern's last column inside its last block
        int32_t sc[16];
        #pragma unroll
        for (int k = 0; k < 16; ++k) sc[k] = uniform(pen[16u * b + k]);
        const uint64_t pg = (uint64_t(uint32_t(uniform(int32_t(psym[2u * b + 1u])))) << 32) | uint32_t(uniform(int32_t(psym[2u * b])));
        int32_t edge = int32_t(0x80000000u);

        for (uint32_t ps = passes; ps-- > 0u; )
        {
            const int32_t i0 = int32_t(64u * ps + lane) - 15;
            int32_t h = b ? int32_t(col[16 + i0 - 1]) : 0;
            // the lane's 16 text symbols, rows i0 .. i0 + 15 (rows above the text: whatever; their cells are held at zero)
            uint32_t tg;
            {
                const uint32_t sym = t_off + uint32_t(max(i0, 0)), w = sym >> 4;
                tg = funnel(txt[w], txt[w + 1u], (sym & 15u) << 1);
                if (i0 < 0) tg <<= 2u * uint32_t(-i0);
            }
            int32_t comb = -1, h_last = 0;
            const bool fast = ps >= 1u && 64u * ps + 63u < N && cols == 16u && (TYPE == NVBIO_HIP_LOCAL || !last);
            if (fast) ham_segment<TYPE, false>(h, comb, h_last, tg, pg, sc, p.match, i0, N, cols, k_last);
            else      ham_segment<TYPE, true >(h, comb, h_last, tg, pg, sc, p.match, i0, N, cols, k_last);
            col[16 + i0 + 15] = int16_t(h);
            if (!last && uint32_t(i0 + 15) < N) edge = max(edge, h);
            if (TYPE == NVBIO_HIP_LOCAL)
            {
                if (comb >= 0) { const uint32_t k = uint32_t(comb) & 15u; ham_report(best, comb >> 4, b, (uint32_t(i0 + int32_t(k) + 1) << 5) | (k + 1u)); }
            }
            else if (last)
            {
                const uint32_t row = uint32_t(i0 + int32_t(k_last));
                if (row < N && M != 0u && (TYPE == NVBIO_HIP_SEMI_GLOBAL || row + 1u == N)) ham_report(best, h_last, b, ((row + 1u) << 5) | (k_last + 1u));
            }
        }
        if (!last)
        {
            #pragma unroll
            for (int o = 32; o >= 1; o >>= 1) edge = max(edge, __shfl_xor(edge, o, 64));
            if (int64_t(edge) + int64_t(M - 16u * (b + 1u)) * int64_t(p.match) < int64_t(min_score)) { exited = true; break; }
        }
        __syncthreads();      // the next block reads the column this one wrote
    }

    // the wave's best: (score, block, row, column), the later report of equal scores
    #pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
    {
        const int32_t  s  = __shfl_xor(best.score, o, 64);
        const uint32_t hi = __shfl_xor(best.hi, o, 64), lo = __shfl_xor(best.lo, o, 64);
        ham_report(best, s, hi, lo);
    }
    if (lane == 0u)
    {
        uint32_t sx = 0xFFFFFFFFu, sy = 0xFFFFFFFFu;
        if (best.lo != 0u) { sx = best.lo >> 5; sy = 16u * best.hi + (best.lo & 31u); }
        else if (TYPE == NVBIO_HIP_GLOBAL && N == 0u && !exited) { best.score = 0; sx = 0u; sy = M; }     // the zero border
        p.out_score[job] = best.score; p.out_sink[2u * job] = sx; p.out_sink[2u * job + 1u] = sy;
        if (p.out_ok) p.out_ok[job] = exited ? 0 : 1;
    }
}

static int hamming_core(const int32_t match, const int32_t* lut, const int32_t flat_mismatch, const int32_t algorithm, const int32_t type,
                        const nvbio_hip_string_set* patterns, const uint8_t* quals, const uint64_t n_quals, const nvbio_hip_string_set* texts,
                        const uint32_t maxM, const uint32_t maxN, const int32_t* min_score, const uint32_t n,
                        const uint32_t* n_dev, const uint32_t* job_index, const uint32_t* gate, const uint32_t gate_limit, const int32_t wave_form,
                        int32_t* out_score, uint32_t* out_sink, uint8_t* out_ok, void* stream)
{
    if (!patterns || !texts || type < 0 || type > 2 || algorithm < 0 || algorithm > 1) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    if (!out_score || !out_sink) return hipErrorInvalidValue;
    if (algorithm != NVBIO_HIP_PATTERN_BLOCKING) return hipErrorNotSupported;
    if (!(patterns->bits == 2 || patterns->bits == 4 || patterns->bits == 8) || texts->bits != 2) return hipErrorNotSupported;
    if (maxM > 4096u) return hipErrorNotSupported;
    // LOCAL packs (h << 4 | k) into 31 bits: h stays below 2^15 + 16 * 2^20 inside a block
    auto big = [](int32_t v) { return v > (1 << 20) || v < -(1 << 20); };
    if (big(match)) return hipErrorNotSupported;
    if (lut) { for (int i = 0; i < 256; ++i) if (big(lut[i])) return hipErrorNotSupported; }
    else if (big(flat_mismatch)) return hipErrorNotSupported;

    HammingParams p;
    p.pat = make_string_set(patterns); p.txt = make_string_set(texts);
    p.match = match; p.min_score = min_score; p.n = n; p.out_score = out_score; p.out_sink = out_sink; p.out_ok = out_ok;
    p.quals = lut ? quals : nullptr; p.n_quals = lut ? n_quals : 0;
    p.m_pad = std::max(16u, 16u * ((maxM + 15u) / 16u));
    p.txt_words = hamming_txt_words(maxN); p.max_n = maxN;
    p.n_dev = wave_form ? n_dev : nullptr; p.job_index = wave_form ? job_index : nullptr;
    p.gate = gate; p.gate_limit = gate_limit; p.gate_above = wave_form ? 0u : 1u;
    for (int i = 0; i < 256; ++i) p.mm_lut[i] = lut ? lut[i] : flat_mismatch;

    const uint64_t lds = hamming_lds_bytes(p.m_pad, maxN);
    if (lds > HAMMING_LDS_MAX) return hipErrorNotSupported;
    const bool whole = lds > HAMMING_LDS_DYNAMIC;
    auto launch = [&](auto kernel) -> int {
        hipLaunchKernelGGL(kernel, dim3(n), dim3(64), whole ? size_t(0) : size_t(lds), to_stream(stream), p);
        return hipGetLastError();
    };
    g_last_kernel = "hamming_score_kernel";
    if (type == NVBIO_HIP_LOCAL)       return whole ? launch(hamming_score_kernel<NVBIO_HIP_LOCAL, true>)       : launch(hamming_score_kernel<NVBIO_HIP_LOCAL, false>);
    if (type == NVBIO_HIP_SEMI_GLOBAL) return whole ? launch(hamming_score_kernel<NVBIO_HIP_SEMI_GLOBAL, true>) : launch(hamming_score_kernel<NVBIO_HIP_SEMI_GLOBAL, false>);
    return whole ? launch(hamming_score_kernel<NVBIO_HIP_GLOBAL, true>) : launch(hamming_score_kernel<NVBIO_HIP_GLOBAL, false>);
}

} // namespace nvb

using namespace nvb;

NVB_API int nvbio_hip_hamming_score(
    const nvbio_hip_sw_scheme* scheme, int32_t algorithm, int32_t type,
    const nvbio_hip_string_set* patterns, const nvbio_hip_string_set* texts,
    uint32_t max_pattern_len, uint32_t max_text_len, const int32_t* min_score,
    uint32_t n, int32_t* out_score, uint32_t* out_sink, uint8_t* out_ok, void* stream)
{
    if (!scheme) return hipErrorInvalidValue;
    return hamming_core(scheme->match, nullptr, scheme->mismatch, algorithm, type, patterns, nullptr, 0, texts, max_pattern_len, max_text_len, min_score, n,
                        nullptr, nullptr, nullptr, 0u, 0, out_score, out_sink, out_ok, stream);
}

NVB_API int nvbio_hip_hamming_score_qual(
    const nvbio_hip_gotoh_qual_scheme* scheme, int32_t algorithm, int32_t type,
    const nvbio_hip_string_set* patterns, const uint8_t* quals, uint64_t n_quals, const nvbio_hip_string_set* texts,
    uint32_t max_pattern_len, uint32_t max_text_len, const int32_t* min_score,
    uint32_t n, int32_t* out_score, uint32_t* out_sink, uint8_t* out_ok, void* stream)
{
    if (!scheme) return hipErrorInvalidValue;
    if (n != 0 && (!quals || n_quals == 0)) return hipErrorInvalidValue;
    return hamming_core(scheme->match, scheme->mismatch, 0, algorithm, type, patterns, quals, n_quals, texts, max_pattern_len, max_text_len, min_score, n,
                        nullptr, nullptr, nullptr, 0u, 0, out_score, out_sink, out_ok, stream);
}

NVB_API int nvbio_hip_hamming_score_qual_jobs(
    const nvbio_hip_gotoh_qual_scheme* scheme, int32_t algorithm, int32_t type,
    const nvbio_hip_string_set* patterns, const uint8_t* quals, uint64_t n_quals, const nvbio_hip_string_set* texts,
    uint32_t max_pattern_len, uint32_t max_text_len, const int32_t* min_score,
    uint32_t n, const uint32_t* n_on_device, const uint32_t* job_index, const uint32_t* gate, uint32_t gate_limit, int32_t wave_form,
    int32_t* out_score, uint32_t* out_sink, uint8_t* out_ok, void* stream)
{
    if (!scheme) return hipErrorInvalidValue;
    if (n != 0 && (!quals || n_quals == 0)) return hipErrorInvalidValue;
    if (wave_form && (!n_on_device || !job_index)) return hipErrorInvalidValue;
    return hamming_core(scheme->match, scheme->mismatch, 0, algorithm, type, patterns, quals, n_quals, texts, max_pattern_len, max_text_len, min_score, n,
                        n_on_device, job_index, gate, gate_limit, wave_form, out_score, out_sink, out_ok, stream);
}
