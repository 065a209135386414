// tools/wavelet_twins_check.cpp -- a stand-alone program over the byte-alphabet host twins (nvbio_hip_*_bytes_host, nvbio_hip_wavelet_*_host)
// on small texts of every symbol size, for a host sanitizer build: text() must give back the BWT, locate() the suffix array, and patterns
// that run past their set's symbols must be clipped.  It needs no GPU.  From the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fopenmp -Xarch_host -fsanitize=address,undefined \
//         nvbio_amd/csrc/host_twins.hip tools/wavelet_twins_check.cpp -o wavelet_twins_check
//   ASAN_OPTIONS=detect_leaks=0 ./wavelet_twins_check        (the OpenMP runtime keeps one allocation of its own until exit)
#include "../include/nvbio_hip.h"
#include <vector>
#include <cstdio>
#include <cstdlib>
int main()
{
    int bad = 0;
    for (unsigned S = 1; S <= 8; ++S)
        for (unsigned n : { 1u, 2u, 31u, 32u, 33u, 97u, 1000u })
        {
            std::vector<uint8_t> text(n);
            srand(S * 1000 + n);
            for (auto& c : text) c = uint8_t(rand());
            const unsigned K = 1u << S, W = (n * S + 31) / 32;
            std::vector<uint32_t> sa(n + 1), ssa(n + 1), bits(W), splits(K), occ(K + W), L2(K + 1);
            std::vector<uint8_t> bwt(n), out8(n + 3);
            uint32_t primary = 0;
            bad |= nvbio_hip_suffix_sort_bytes_host(text.data(), S, n, sa.data(), 2);
            bad |= nvbio_hip_bwt_bytes_host(text.data(), S, n, 4, bwt.data(), &primary, ssa.data(), nullptr, 2);
            bad |= nvbio_hip_wavelet_setup_host(bwt.data(), S, n, bits.data(), splits.data(), occ.data(), 2);
            nvbio_hip_wavelet_tree t = { bits.data(), splits.data(), occ.data(), S, n };
            std::vector<uint32_t> pos(n + 3), r(n + 3), rr(2 * ((n + 3) / 2));
            for (unsigned i = 0; i < n + 3; ++i) pos[i] = i < n + 2 ? i : 0xFFFFFFFFu;
            std::vector<uint8_t> sym(n + 3);
            for (auto& c : sym) c = uint8_t(rand());
            bad |= nvbio_hip_wavelet_text_host(&t, pos.data(), n + 3, out8.data(), 2);
            bad |= nvbio_hip_wavelet_text_host(&t, nullptr, n, out8.data(), 2);
            bad |= nvbio_hip_wavelet_rank_host(&t, pos.data(), sym.data(), n + 3, r.data(), 2);
            bad |= nvbio_hip_wavelet_rank_range_host(&t, pos.data(), sym.data(), (n + 3) / 2, rr.data(), 2);
            bad |= nvbio_hip_wavelet_fm_L2_host(&t, L2.data(), 2);
            nvbio_hip_wavelet_fmindex f = { t, L2.data(), ssa.data(), n, primary, 4, 0 };
            std::vector<uint64_t> begin(n); std::vector<uint32_t> len(n);
            for (unsigned i = 0; i < n; ++i) { begin[i] = i; len[i] = n - i + (i % 3); }       // some run past the end: clipped
            nvbio_hip_byte_string_set ps = { text.data(), n, begin.data(), len.data(), 0, 0 };
            std::vector<uint32_t> ranges(2 * n), where(n + 3);
            bad |= nvbio_hip_wavelet_fm_match_host(&f, &ps, n, ranges.data(), 2);
            bad |= nvbio_hip_wavelet_fm_locate_host(&f, pos.data(), n + 3, where.data(), 2);
            for (unsigned i = 0; i <= n; ++i) if (i && where[i] != sa[i]) { printf("locate S=%u n=%u row %u\n", S, n, i); bad = 1; }
            for (unsigned i = 0; i < n; ++i) if (out8[i] != bwt[i]) { printf("text S=%u n=%u\n", S, n); bad = 1; }
        }
    printf(bad ? "FAILED\n" : "ok\n");
    return bad;
}
