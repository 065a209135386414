// pair_row_probe.hip -- where a row of banded_gotoh_pair_kernel<15, PM3> spends its cycles outside its cells, and what the same row costs
// with the column frame's cell (PD3).
//
// Launches the real kernel template (nvbio_amd/csrc/banded_gotoh_pair.h) in its forms and in knock-out variants of them on strings
// generated on the device in the headline's layout: 100-symbol reads, 4 bits big-endian, back to back; 150-symbol windows, 2 bits
// little-endian, back to back; scheme (2,-1,-2,-1).  Two warm-up launches, then ten timed ones with HIP events around each.
// A knock-out takes one part of the row away and keeps its inputs live (PairForm, PF_KO_*); what it prints is a time, never a result.
// The forms that do compute results print a checksum of scores and sinks, which must be the same for all of them.
// The last rows are the column frame's row with its sink folded once per two rows (PF_FOLD2), and that row with the cell's wave-uniform
// constants in scalar registers (const-s) and as literals with the pad (PF_CONST2, const-klit-pad), and on that row the two sub-* rows:
// the knock-out with a v_xor_b32 in each v_perm_b32's place (PF_KO_PERM, the ceiling of the lookup's class change) and the substitution
// words read from LDS (PF_SUBLDS, sub-lds); then two cells' words to a read (sub-xor8, its ceiling, and PF_SUBLDS2, sub-lds2, which the
// library launches) and the pad-* rows, s_nop pads at places that had none.  The forms that were measured beside them and are gone have
// their figures in profiles/banded_pair/README.md.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/pair_row_probe.hip -o tools/pair_row_probe
//   tools/pair_row_probe [jobs = 10000000] [timed launches = 10] [only the variants whose names begin with this]
// (fewer than about 10 M jobs are too few rounds of waves per SIMD for the cycles per row to mean much)
//
// Counters: run it under the profiler with one counter group and `10000000 1`; every variant is a kernel of its own name.
#include "../nvbio_amd/csrc/banded_gotoh_pair.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

namespace nvb {
// the library's launch bookkeeping, which the headers declare and this program does not use
thread_local const char* g_last_kernel = nullptr;
thread_local PairLaunch g_last_pair;
int test_switch(TestSwitch) { return 0; }
}
using namespace nvb;

constexpr uint32_t READ = 100, WINDOW = 150;

__device__ __forceinline__ uint32_t mix(uint64_t x)
{
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
    return uint32_t(x);
}
__device__ __forceinline__ uint32_t text_symbol(uint64_t job, uint32_t pos) { return mix(job * WINDOW + pos) & 3u; }

// word w of the text array: symbols 16 w ... 16 w + 15, little-endian
__global__ void make_text(uint32_t* words, uint64_t n_words, uint64_t n_symbols)
{
    const uint64_t w = blockIdx.x * uint64_t(blockDim.x) + threadIdx.x;
    if (w >= n_words) return;
    uint32_t v = 0;
    for (uint32_t k = 0; k < 16u; ++k)
    {
        const uint64_t g = 16u * w + k;
        if (g < n_symbols) v |= text_symbol(g / WINDOW, uint32_t(g % WINDOW)) << (2u * k);
    }
    words[w] = v;
}
// word w of the pattern array: symbols 8 w ... 8 w + 7, big-endian.  A read is its window from column 7 on, one symbol in 16 redrawn from 0 ... 4
__global__ void make_reads(uint32_t* words, uint64_t n_words, uint64_t n_symbols)
{
    const uint64_t w = blockIdx.x * uint64_t(blockDim.x) + threadIdx.x;
    if (w >= n_words) return;
    uint32_t v = 0;
    for (uint32_t k = 0; k < 8u; ++k)
    {
        const uint64_t g = 8u * w + k;
        if (g >= n_symbols) break;
        const uint32_t r = mix(g ^ 0x9e3779b97f4a7c15ull);
        const uint32_t s = (r & 15u) == 0u ? (r >> 4) % 5u : text_symbol(g / READ, uint32_t(g % READ) + 7u);
        v |= s << (28u - 4u * k);
    }
    words[w] = v;
}
__global__ void make_begins(uint64_t* pb, uint64_t* tb, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { pb[i] = uint64_t(i) * READ; tb[i] = uint64_t(i) * WINDOW; }
}

struct Variant { const char* name; const char* what; hipError_t (*launch)(const GotohParams&, hipStream_t); uint32_t rows; bool results; };

#define FORM(f) launch_band_pair<15, PM3, (f)>
#define COLF(f) launch_band_pair<15, PD3, (f)>
constexpr int STREAMED = PF_STREAM | PF_PBE;               // the streamed form of these strings: 4-bit big-endian reads, little-endian windows
constexpr int SUBLDS = STREAMED | PF_FOLD2 | PF_CONST2 | PF_GE1 | PF_SUBLDS;   // sub-lds's form
static const Variant VARIANTS[] = {
    { "K0",        "nothing: generic fetches (the form before the streamed one)",      FORM(PF_SINK_VCC), READ, true },
    { "K1",        "the sink fold",                                                    FORM(PF_KO_SINK), READ, false },
    { "K2",        "the LDS table reads",                                              FORM(PF_KO_TABLE), READ, false },
    { "K3",        "the block loop's fetches",                                         FORM(PF_KO_FETCH), READ, false },
    { "K0/96",     "nothing, 96 rows (K4's and K5's yardstick)",                       FORM(PF_SINK_VCC), 96, true },
    { "K4",        "the per-row bound test, 96 rows",                                  FORM(PF_KO_BOUND), 96, false },
    { "K5",        "K1 to K4 together, 96 rows: cells only",                           FORM(PF_KO_SINK | PF_KO_TABLE | PF_KO_FETCH | PF_KO_BOUND), 96, false },
    { "sink-key",  "generic fetches, sink: one 32-bit key per job, plain maximum",     FORM(PF_SINK_KEY), READ, true },
    { "stream",    "streamed words (what the library launches for these strings)",     FORM(STREAMED), READ, true },
    { "stream-key","streamed words, key sink",                                         FORM(STREAMED | PF_SINK_KEY), READ, true },
    { "stream-K2", "streamed words without the LDS table reads",                       FORM(STREAMED | PF_KO_TABLE), READ, false },
    { "stream/96", "streamed words, 96 rows (stream-K4's yardstick)",                  FORM(STREAMED), 96, true },
    { "stream-K4", "streamed words without the per-row bound test, 96 rows",           FORM(STREAMED | PF_KO_BOUND), 96, false },
    // the column frame's cell in the same forms: the whole kernel beside K0 and stream, the cells alone beside K5
    { "col-K0",    "column frame, nothing: generic fetches",                           COLF(PF_SINK_VCC), READ, true },
    { "col-K0/96", "column frame, nothing, 96 rows (col-K5's yardstick)",              COLF(PF_SINK_VCC), 96, true },
    { "col-K5",    "column frame, K1 to K4 together, 96 rows: cells only",             COLF(PF_KO_SINK | PF_KO_TABLE | PF_KO_FETCH | PF_KO_BOUND), 96, false },
    { "col-stream","column frame, streamed words (what the library launches)",         COLF(STREAMED), READ, true },
    { "col-stream/96", "column frame, streamed words, 96 rows",                        COLF(STREAMED), 96, true },
    // the row around the column frame's cells: the pair fold, which the library takes; its checksum must be col-stream's
    { "col-fold2",  "col-stream, the sink folded once per two rows (the library's row)",   COLF(STREAMED | PF_FOLD2), READ, true },
    { "col-stream'", "col-stream once more (the run's drift)",                         COLF(STREAMED), READ, true },
    // where the cell's wave-uniform constants live, on the library's row; their checksums must be col-fold2's
    { "const-s",    "col-fold2 once more: D and K_j in scalar registers",              COLF(STREAMED | PF_FOLD2), READ, true },
    { "const-klit-pad", "col-fold2, K_j and 2 G literals, s_nop pads (the library's launch)", COLF(STREAMED | PF_FOLD2 | PF_CONST2 | PF_GE1), READ, true },
    { "const-s'",   "const-s once more (the run's drift)",                             COLF(STREAMED | PF_FOLD2), READ, true },
    // where the substitution words come from, on const-klit-pad's row: the ceiling of the lookup's class change (a knock-out), and the
    // words read from LDS, one ds_read_b32 per cell, whose checksum must be const-klit-pad's
    { "sub-xor",    "const-klit-pad, a v_xor_b32 for each v_perm_b32, table reads kept", COLF(STREAMED | PF_FOLD2 | PF_CONST2 | PF_GE1 | PF_KO_PERM), READ, false },
    { "sub-lds",    "const-klit-pad, substitution words from LDS (PF_SUBLDS)",         COLF(STREAMED | PF_FOLD2 | PF_CONST2 | PF_GE1 | PF_SUBLDS), READ, true },
    { "sub-perm'",  "const-klit-pad once more (the run's drift)",                      COLF(STREAMED | PF_FOLD2 | PF_CONST2 | PF_GE1), READ, true },
    // two cells per read, on sub-lds's row: the ceiling (a knock-out: eight address xors and eight reads of two adjacent words of
    // sub-lds's table, so seven cells of a row take a wrong word), the form itself (PF_SUBLDS2, ds_read_b64 from a table of 1 024 pairs),
    // whose checksum must be sub-lds's, and sub-lds once more
    { "sub-xor8",   "sub-lds, 8 address xors and 8 two-word reads per row",            COLF(SUBLDS | PF_KO_XOR8), READ, false },
    { "sub-lds2",   "sub-lds, two cells per read (PF_SUBLDS2, the library's launch)",  COLF(SUBLDS | PF_SUBLDS2), READ, true },
    { "sub-lds2-a2","sub-lds2, the reads two pairs ahead of the cells (one VGPR spilled)", COLF(SUBLDS | PF_SUBLDS2 | PF_AHEAD2), READ, true },
    { "sub-lds'",   "sub-lds once more (the run's drift)",                             COLF(SUBLDS), READ, true },
    // pads that were never tried, on both LDS rows: one s_nop behind each run of address xors (padx); PF_CONST2's pad behind the
    // groups of simple ops in col0 and tail2 as well (pade)
    { "pad-lds-x",  "sub-lds, an s_nop behind each run of address xors",               COLF(SUBLDS | PF_PAD_XOR), READ, true },
    { "pad-lds-e",  "sub-lds, s_nop pads in col0 and tail2",                           COLF(SUBLDS | PF_PAD_EDGE), READ, true },
    { "pad-lds2-x", "sub-lds2, an s_nop behind each run of address xors",              COLF(SUBLDS | PF_SUBLDS2 | PF_PAD_XOR), READ, true },
    { "pad-lds2-e", "sub-lds2, s_nop pads in col0 and tail2",                          COLF(SUBLDS | PF_SUBLDS2 | PF_PAD_EDGE), READ, true },
    { "pad-lds2-xe","sub-lds2, both pads",                                             COLF(SUBLDS | PF_SUBLDS2 | PF_PAD_XOR | PF_PAD_EDGE), READ, true },
    { "sub-lds2'",  "sub-lds2 once more (the run's drift)",                            COLF(SUBLDS | PF_SUBLDS2), READ, true },
};

int main(int argc, char** argv)
{
    const uint32_t n = argc > 1 ? uint32_t(strtoul(argv[1], nullptr, 10)) : 10000000u;
    const int timed = argc > 2 ? atoi(argv[2]) : 10;
    const char* only = argc > 3 ? argv[3] : "";
    if (n == 0 || n > 20000000u || timed < 1 || timed > 100) { printf("usage: pair_row_probe [jobs <= 20000000] [timed launches <= 100] [name prefix]\n"); return 2; }
    const uint64_t psym = uint64_t(n) * READ, tsym = uint64_t(n) * WINDOW, pw = (psym + 7u) / 8u + 4u, tw = (tsym + 15u) / 16u + 4u;
    uint32_t *pwords, *twords, *sink; int32_t* score; uint64_t *pbegin, *tbegin;
    CHECK(hipMalloc(&pwords, pw * 4u)); CHECK(hipMalloc(&twords, tw * 4u));
    CHECK(hipMalloc(&pbegin, uint64_t(n) * 8u)); CHECK(hipMalloc(&tbegin, uint64_t(n) * 8u));
    CHECK(hipMalloc(&score, uint64_t(n) * 4u)); CHECK(hipMalloc(&sink, uint64_t(n) * 8u));
    hipLaunchKernelGGL(make_text, dim3(uint32_t((tw + 255u) / 256u)), dim3(256), 0, 0, twords, tw, tsym);
    hipLaunchKernelGGL(make_reads, dim3(uint32_t((pw + 255u) / 256u)), dim3(256), 0, 0, pwords, pw, psym);
    hipLaunchKernelGGL(make_begins, dim3((n + 255u) / 256u), dim3(256), 0, 0, pbegin, tbegin, n);
    CHECK(hipGetLastError()); CHECK(hipDeviceSynchronize());

    GotohParams p = {};
    p.pat.s.words = pwords; p.pat.s.n_words = pw; p.pat.s.bits = 4; p.pat.s.big_endian = 1; p.pat.begin = pbegin;
    p.txt.s.words = twords; p.txt.s.n_words = tw; p.txt.s.bits = 2; p.txt.s.big_endian = 0; p.txt.begin = tbegin; p.txt.fixed_length = WINDOW;
    p.match = 2; p.mismatch = -1; p.gap_open = -2; p.gap_ext = -1; p.txt_gap_open = -2; p.txt_gap_ext = -1;
    p.n = n; p.out_score = score; p.out_sink = sink;

    const double waves = double((n / 2u + (n & 1u) + 63u) / 64u), simd_hz = 2.4e9 * 1024.0;
    std::vector<int32_t> hs(n); std::vector<uint32_t> hk(2u * size_t(n));
    hipEvent_t e0, e1; CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    printf("%u jobs, %u-symbol reads, %u-symbol windows, band 15, LOCAL (2,-1,-2,-1); %d timed launches after 2 warm-ups\n", n, READ, WINDOW, timed);
    printf("%-14s %-68s %4s  %-26s %12s %12s  %s\n", "variant", "what is removed / which form", "rows", "ms min / median / max", "cyc/row(min)", "cyc/row(med)", "checksum");
    for (const Variant& v : VARIANTS)
    {
        if (strncmp(v.name, only, strlen(only)) != 0) continue;
        p.pat.fixed_length = v.rows;
        std::vector<float> ms;
        for (int it = 0; it < 2 + timed; ++it)
        {
            CHECK(hipEventRecord(e0, 0));
            CHECK(v.launch(p, 0));
            CHECK(hipEventRecord(e1, 0));
            CHECK(hipEventSynchronize(e1));
            float t; CHECK(hipEventElapsedTime(&t, e0, e1));
            if (it >= 2) ms.push_back(t);
        }
        std::sort(ms.begin(), ms.end());
        const float med = ms[ms.size() / 2];
        char sum[32] = "-";
        if (v.results)
        {
            CHECK(hipMemcpy(hs.data(), score, size_t(n) * 4u, hipMemcpyDeviceToHost)); CHECK(hipMemcpy(hk.data(), sink, size_t(n) * 8u, hipMemcpyDeviceToHost));
            uint64_t c = 0;
            for (size_t i = 0; i < n; ++i) c = (c ^ uint32_t(hs[i])) * 0x100000001b3ull + hk[2 * i] * 31u + hk[2 * i + 1];
            snprintf(sum, sizeof sum, "%016llx", (unsigned long long)c);
        }
        char t3[64]; snprintf(t3, sizeof t3, "%.4f / %.4f / %.4f", ms.front(), med, ms.back());
        printf("%-14s %-68s %4u  %-26s %12.1f %12.1f  %s\n", v.name, v.what, v.rows, t3, ms.front() * 1e-3 * simd_hz / (waves * v.rows), med * 1e-3 * simd_hz / (waves * v.rows), sum);
        fflush(stdout);
    }
    return 0;
}
