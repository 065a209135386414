// valu_probe.hip -- per-opcode VALU issue-rate probe for gfx950 (wave64 instructions per cycle per SIMD).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

#define OPS_LIST \
  X(add_u32,      "v_add_u32 %0, %0, %1") \
  X(max_i32,      "v_max_i32 %0, %0, %1") \
  X(min_i32,      "v_min_i32 %0, %0, %1") \
  X(max3_i32,     "v_max3_i32 %0, %0, %1, %1") \
  X(cndmask_vcc,  "v_cndmask_b32 %0, %0, %1, vcc") \
  X(cndmask_sgpr, "v_cndmask_b32_e64 %0, %0, %1, s[10:11]") \
  X(cmp_eq_u32,   "v_cmp_eq_u32 vcc, %0, %1") \
  X(cmp_eq_u16,   "v_cmp_eq_u16 vcc, %0, %1") \
  X(cmp_sgpr,     "v_cmp_eq_u32_e64 s[10:11], %0, %1") \
  X(cmp_cnd_pair, "v_cmp_eq_u32 vcc, %0, %1\n v_cndmask_b32 %0, %0, %1, vcc") \
  X(cmpx_pair,    "v_cmp_eq_u32_e64 s[10:11], %0, %1\n v_cndmask_b32_e64 %0, %0, %1, s[10:11]") \
  X(or_b32,       "v_or_b32 %0, %0, %1") \
  X(lshlrev_b32,  "v_lshlrev_b32 %0, 1, %0") \
  X(lshrrev_b32,  "v_lshrrev_b32 %0, 1, %0") \
  X(ashrrev_i32,  "v_ashrrev_i32 %0, 1, %0") \
  X(add_u16,      "v_add_u16 %0, %0, %1") \
  X(sub_u16,      "v_sub_u16 %0, %0, %1") \
  X(max_i16,      "v_max_i16 %0, %0, %1") \
  X(min_i16,      "v_min_i16 %0, %0, %1") \
  X(max_u16,      "v_max_u16 %0, %0, %1") \
  X(min_u16,      "v_min_u16 %0, %0, %1") \
  X(lshlrev_b16,  "v_lshlrev_b16 %0, 1, %0") \
  X(mul_lo_u16,   "v_mul_lo_u16 %0, %0, %1") \
  X(max_f32,      "v_max_f32 %0, %0, %1") \
  X(add_f32,      "v_add_f32 %0, %0, %1") \
  X(max_f16,      "v_max_f16 %0, %0, %1") \
  X(add_f16,      "v_add_f16 %0, %0, %1") \
  X(and_or_b32,   "v_and_or_b32 %0, %0, %1, %1") \
  X(lshl_add_u32, "v_lshl_add_u32 %0, %0, 5, %1") \
  X(bfi_b32,      "v_bfi_b32 %0, %0, %1, %1") \
  X(med3_i32,     "v_med3_i32 %0, %0, %1, %1") \
  X(add_co_u32,   "v_add_co_u32 %0, vcc, %0, %1") \
  X(subrev_u32,   "v_subrev_u32 %0, %0, %1") \
  X(mad_u16,      "v_mad_u16 %0, %0, %1, %1") \
  X(sub_u16_clamp,"v_sub_u16_e64 %0, %0, %1 clamp") \
  X(max_i16_sdwa, "v_max_i16_sdwa %0, %0, %1 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1 src1_sel:WORD_1") \
  X(add_u16_sdwa, "v_add_u16_sdwa %0, %0, %1 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1 src1_sel:WORD_1") \
  X(pk_max_i16,   "v_pk_max_i16 %0, %0, %1") \
  X(perm_b32,     "v_perm_b32 %0, %0, %1, %1") \
  X(bfe_u32,      "v_bfe_u32 %0, %0, %1, 8") \
  X(bfe_i32,      "v_bfe_i32 %0, %0, %1, 8") \
  X(xor_b32,      "v_xor_b32 %0, %0, %1") \
  X(and_b32,      "v_and_b32 %0, %0, %1") \
  X(alignbit_b32, "v_alignbit_b32 %0, %0, %1, %1") \
  X(alignbyte_b32,"v_alignbyte_b32 %0, %0, %1, %1") \
  X(lshrrev_b16,  "v_lshrrev_b16 %0, %1, %0") \
  X(lshrrev_b32v, "v_lshrrev_b32 %0, %1, %0") \
  X(perm_add_pair,"v_perm_b32 %0, %0, %1, %1\n v_add_u16 %0, %0, %1") \
  X(cmp_cnd_add,  "v_cmp_eq_u32 vcc, %0, %1\n v_cndmask_b32 %0, %0, %1, vcc\n v_add_u16 %0, %0, %1") \
  X(mov_dpp,      "v_mov_b32_dpp %0, %1 wave_shr:1 row_mask:0xf bank_mask:0xf") \
  X(xor_subclamp, "v_xor_b32 %0, %0, %1\n v_sub_u16_e64 %0, %1, %0 clamp") \
  X(cnd_dpp_vcc,  "v_cndmask_b32_dpp %0, %0, %1, vcc wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0") \
  X(smov_cnd_dpp, "s_mov_b64 vcc, s[10:11]\n v_cndmask_b32_dpp %0, %0, %1, vcc wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0") \
  X(smov_3cnd_dpp,"s_mov_b64 vcc, s[10:11]\n v_cndmask_b32_dpp %0, %0, %1, vcc wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n v_cndmask_b32_dpp %0, %0, %1, vcc wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n v_cndmask_b32_dpp %0, %0, %1, vcc wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0") \
  X(dpp_cnd_sgpr, "v_mov_b32_dpp %0, %1 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n v_cndmask_b32_e64 %0, %0, %1, s[10:11]") \
  X(add_u16_dpp,  "v_add_u16_dpp %0, %1, %0 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0") \
  X(max_i16_dpp,  "v_max_i16_dpp %0, %1, %0 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0") \
  X(mad_u32_u24,  "v_mad_u32_u24 %0, %0, %1, %1") \
  X(s_nop_add,    "s_nop 0\n v_add_u16 %0, %0, %1") \
  X(add_u16_sgpr, "v_add_u16 %0, s10, %0") \
  X(smov_add,     "s_mov_b64 vcc, s[10:11]\n v_add_u16 %0, %0, %1") \
  X(max_i16_inl0, "v_max_i16 %0, 0, %0") \
  X(add_u16_inl7, "v_add_u16 %0, 7, %0") \
  X(max_i16_sgpr, "v_max_i16 %0, s10, %0") \
  X(perm_sgpr,    "v_perm_b32 %0, %0, %1, s10") \
  X(mov_dpp_rshl, "v_mov_b32_dpp %0, %1 row_shl:3 row_mask:0xf bank_mask:0xf bound_ctrl:0") \
  X(and_lit,      "v_and_b32 %0, 0x30000, %0") \
  X(mul_u32_u24,  "v_mul_u32_u24 %0, %0, %1") \
  X(lshl_or,      "v_lshl_or_b32 %0, %0, 3, %1") \
  X(add_lshl,     "v_add_lshl_u32 %0, %0, %1, 1") \
  X(add3,         "v_add3_u32 %0, %0, %1, %1") \
  X(add_i16_clamp,"v_add_i16 %0, %0, %1 clamp") \
  X(sub_i16_clamp,"v_sub_i16 %0, %0, %1 clamp") \
  X(add_u16_clamp,"v_add_u16_e64 %0, %0, %1 clamp") \
  X(add_i16,      "v_add_i16 %0, %0, %1") \
  X(max_i16_e64,  "v_max_i16_e64 %0, %0, %1") \
  X(mov_b32,      "v_mov_b32 %0, %1") \
  X(swap_b32,     "v_swap_b32 %0, %1") \
  X(pk_max_u16,   "v_pk_max_u16 %0, %0, %1") \
  X(pk_max_f16,   "v_pk_max_f16 %0, %0, %1") \
  X(pk_maximum3_f16, "v_pk_maximum3_f16 %0, %0, %1, %1") \
  X(pk_minimum3_f16, "v_pk_minimum3_f16 %0, %0, %1, %1") \
  X(add_u32_lit,  "v_add_u32 %0, 0x000d000d, %0") \
  X(pk_add_u16,   "v_pk_add_u16 %0, %0, %1") \
  X(max3_then_u16,"v_pk_maximum3_f16 %0, %0, %1, %1\n v_pk_max_u16 %0, %0, %1") \
  X(max3_then_sub,"v_pk_maximum3_f16 %0, %0, %1, %1\n v_sub_u32 %0, %0, %1") \
  X(u16_then_sub, "v_pk_max_u16 %0, %0, %1\n v_sub_u32 %0, %0, %1")

#define X(name, str) \
__global__ void __launch_bounds__(256) k_##name(uint32_t* out, int iters) { \
    uint32_t a0 = threadIdx.x, a1 = a0 + 1, a2 = a0 + 2, a3 = a0 + 3, a4 = a0 + 4, a5 = a0 + 5, a6 = a0 + 6, a7 = a0 + 7; \
    uint32_t b = blockIdx.x | 1; \
    for (int i = 0; i < iters; ++i) { \
        _Pragma("unroll") for (int u = 0; u < 8; ++u) { \
            asm volatile(str : "+v"(a0) : "v"(b) : "vcc"); asm volatile(str : "+v"(a1) : "v"(b) : "vcc"); \
            asm volatile(str : "+v"(a2) : "v"(b) : "vcc"); asm volatile(str : "+v"(a3) : "v"(b) : "vcc"); \
            asm volatile(str : "+v"(a4) : "v"(b) : "vcc"); asm volatile(str : "+v"(a5) : "v"(b) : "vcc"); \
            asm volatile(str : "+v"(a6) : "v"(b) : "vcc"); asm volatile(str : "+v"(a7) : "v"(b) : "vcc"); } } \
    out[blockIdx.x * 256 + threadIdx.x] = a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ a6 ^ a7; }
OPS_LIST
#undef X

// ---- a simple op's price under the pair row's conditions (`valu_probe mix`; profiles/banded_pair/valu_probe_mix.txt)
//
// cellmix_*: the fifteen instructions of PD3::cell2 (nvbio_amd/csrc/banded_gotoh_pair.h), same opcodes, order and dependences, on resident
// registers: four cells' F' / S' sets one after the other, E' and the row key chained through them as in a row.  The table words are
// zero (every substitution byte 0) and Z = 0x2000, D = 0x40, K = 0x4c / 0x2d per half, so every half settles between Z - D and Z + K,
// inside the f16-ordered range.  _s: D, K_0, K_1, Z_0, Z_1 in scalar registers; _v: D, K_0, K_1 in vector registers; _lit: as literals.
// ratio_k: one v_pk_maximum3_f16 and k dependent v_add_u32 (of a register holding 0) on vector registers.
// Occupancy: blocks of 256 lanes (one wave per SIMD), one round of 256 * W blocks, W held by the launch's dynamic LDS.
// Phase: de-phased, a wave first runs (11 * its slot on the SIMD) mod 15 of the body's instructions (mod k + 1 for ratio_k), so that
// the waves of a SIMD stand at different places of the body.
#define CM_I0  "v_perm_b32 %[d0], %[thi], %[tlo], %[g0]\n\t"
#define CM_I1  "v_perm_b32 %[d1], %[thi], %[tlo], %[g1]\n\t"
#define CM_I2  "v_pk_maximum3_f16 %[f0], %[f1], %[s1], %[z0]\n\t"
#define CM_I3  "v_pk_maximum3_f16 %[f1], %[f2], %[s2], %[z1]\n\t"
#define CM_I4  "v_add_u32 %[d0], %[s0], %[d0]\n\t"
#define CM_I5  "v_add_u32 %[d1], %[s1], %[d1]\n\t"
#define CM_I6  "v_pk_maximum3_f16 %[h], %[f0], %[d0], %[ei]\n\t"
#define CM_I7  "v_subrev_u32 %[s0], %[dd], %[h]\n\t"
#define CM_I8  "v_add_u32 %[d0], %[k0], %[h]\n\t"
#define CM_I9  "v_pk_max_u16 %[e], %[ei], %[s0]\n\t"
#define CM_I10 "v_pk_maximum3_f16 %[h], %[f1], %[d1], %[e]\n\t"
#define CM_I11 "v_subrev_u32 %[s1], %[dd], %[h]\n\t"
#define CM_I12 "v_add_u32 %[d1], %[k1], %[h]\n\t"
#define CM_I13 "v_pk_max_u16 %[e], %[e], %[s1]\n\t"
#define CM_I14 "v_pk_maximum3_f16 %[rk], %[rk], %[d0], %[d1]"
#define CM_BODY CM_I0 CM_I1 CM_I2 CM_I3 CM_I4 CM_I5 CM_I6 CM_I7 CM_I8 CM_I9 CM_I10 CM_I11 CM_I12 CM_I13 CM_I14
#define CM_OPS(F0, F1, S0, S1, EI, E, CD, CK) \
    : [f0] "+v"(F0), [f1] "+v"(F1), [s0] "+v"(S0), [s1] "+v"(S1), [ei] "+v"(EI), [e] "+v"(E), [rk] "+v"(rk), [d0] "+v"(d0), [d1] "+v"(d1), [h] "+v"(h) \
    : [f2] "v"(f2), [s2] "v"(s2), [g0] "v"(g0), [g1] "v"(g1), [tlo] "v"(tlo), [thi] "v"(thi), [z0] "s"(Z0), [z1] "s"(Z1), [dd] CD, [k0] CK##0, [k1] CK##1
#define CM_LIT_D 0x00400040
#define CM_LIT_K0 0x004c004c
#define CM_LIT_K1 0x002d002d
#define CM_KERNEL(name, CD, CK, PIN, BODY) \
__global__ void __launch_bounds__(256) k_cellmix_##name(uint32_t* out, int iters, int dephase, uint32_t D, uint32_t K0, uint32_t K1, uint32_t Z0, uint32_t Z1) { \
    const uint32_t lo = 0x04000400u + (threadIdx.x & 1u) * 0x00010001u, s_ = Z0 - D; \
    uint32_t fa0 = lo, fa1 = lo, fb0 = lo, fb1 = lo, fc0 = lo, fc1 = lo, fd0 = lo, fd1 = lo, sa0 = s_, sa1 = s_, sb0 = s_, sb1 = s_, sc0 = s_, sc1 = s_, sd0 = s_, sd1 = s_; \
    uint32_t f2 = lo, s2 = s_, g0 = 0x0C040C00u | (threadIdx.x & 3u), g1 = 0x0C040C00u | ((threadIdx.x >> 2) & 3u), tlo = 0u, thi = 0u; \
    uint32_t ea = 0x10001000u, eb = 0x10001000u, rk = lo, d0 = lo, d1 = lo, h = lo; \
    asm volatile("" : "+v"(f2), "+v"(s2), "+v"(g0), "+v"(g1), "+v"(tlo), "+v"(thi)); \
    PIN \
    const int skew = dephase ? int((__builtin_amdgcn_s_getreg(4 | (3 << 11)) * 11u) % 15u) : 0;      /* HW_ID bits 0-3: the wave's slot on its SIMD */ \
    if (skew > 0)  asm volatile(CM_I0  CM_OPS(fa0, fa1, sa0, sa1, ea, eb, CD, CK)); \
    if (skew > 1)  asm volatile(CM_I1  CM_OPS(fa0, fa1, sa0, sa1, ea, eb, CD, CK)); \
    if (skew > 2)  asm volatile(CM_I2  CM_OPS(fa0, fa1, sa0, sa1, ea, eb, CD, CK)); \
    if (skew > 3)  asm volatile(CM_I3  CM_OPS(fa0, fa1, sa0, sa1, ea, eb, CD, CK)); \
    if (skew > 4)  asm volatile(CM_I4  CM_OPS(fa0, fa1, sa0, sa1, ea, eb, CD, CK)); \
    if (skew > 5)  asm volatile(CM_I5  CM_OPS(fa0, fa1, sa0, sa1, ea, eb, CD, CK)); \
    if (skew > 6)  asm volatile(CM_I6  CM_OPS(fa0, fa1, sa0, sa1, ea, eb, CD, CK)); \
    if (skew > 7)  asm volatile(CM_I7  CM_OPS(fa0, fa1, sa0, sa1, ea, eb, CD, CK)); \
    if (skew > 8)  asm volatile(CM_I8  CM_OPS(fa0, fa1, sa0, sa1, ea, eb, CD, CK)); \
    if (skew > 9)  asm volatile(CM_I9  CM_OPS(fa0, fa1, sa0, sa1, ea, eb, CD, CK)); \
    if (skew > 10) asm volatile(CM_I10 CM_OPS(fa0, fa1, sa0, sa1, ea, eb, CD, CK)); \
    if (skew > 11) asm volatile(CM_I11 CM_OPS(fa0, fa1, sa0, sa1, ea, eb, CD, CK)); \
    if (skew > 12) asm volatile(CM_I12 CM_OPS(fa0, fa1, sa0, sa1, ea, eb, CD, CK)); \
    if (skew > 13) asm volatile(CM_I13 CM_OPS(fa0, fa1, sa0, sa1, ea, eb, CD, CK)); \
    for (int i = 0; i < iters; ++i) { \
        asm volatile(BODY CM_OPS(fa0, fa1, sa0, sa1, ea, eb, CD, CK)); \
        asm volatile(BODY CM_OPS(fb0, fb1, sb0, sb1, eb, ea, CD, CK)); \
        asm volatile(BODY CM_OPS(fc0, fc1, sc0, sc1, ea, eb, CD, CK)); \
        asm volatile(BODY CM_OPS(fd0, fd1, sd0, sd1, eb, ea, CD, CK)); } \
    out[blockIdx.x * 256 + threadIdx.x] = fa0 ^ fa1 ^ fb0 ^ fb1 ^ fc0 ^ fc1 ^ fd0 ^ fd1 ^ sa0 ^ sa1 ^ sb0 ^ sb1 ^ sc0 ^ sc1 ^ sd0 ^ sd1 ^ ea ^ eb ^ rk ^ d0 ^ d1 ^ h; }
#define CM_Ks0 "s"(K0)
#define CM_Ks1 "s"(K1)
#define CM_Kv0 "v"(K0)
#define CM_Kv1 "v"(K1)
#define CM_Kn0 "n"(CM_LIT_K0)
#define CM_Kn1 "n"(CM_LIT_K1)
CM_KERNEL(s,   "s"(D), CM_Ks, , CM_BODY)
CM_KERNEL(v,   "v"(D), CM_Kv, asm volatile("" : "+v"(D), "+v"(K0), "+v"(K1));, CM_BODY)
CM_KERNEL(lit, "n"(CM_LIT_D), CM_Kn, , CM_BODY)
// cellmix_s with s_nop 0 at chosen places of the body (a scalar instruction between two vector instructions of one wave):
// pad_a: behind each group of simple ops (I5, I8, I12); pad_b: between the two simple ops of each group (I4, I7, I11); pad_c: behind
// every simple op; pad_d: behind every instruction; pad_e: one, in the middle (I8); pad_f: behind every slow op
#define CM_N "s_nop 0\n\t"
#define CM_BODY_A CM_I0 CM_I1 CM_I2 CM_I3 CM_I4 CM_I5 CM_N CM_I6 CM_I7 CM_I8 CM_N CM_I9 CM_I10 CM_I11 CM_I12 CM_N CM_I13 CM_I14
#define CM_BODY_B CM_I0 CM_I1 CM_I2 CM_I3 CM_I4 CM_N CM_I5 CM_I6 CM_I7 CM_N CM_I8 CM_I9 CM_I10 CM_I11 CM_N CM_I12 CM_I13 CM_I14
#define CM_BODY_C CM_I0 CM_I1 CM_I2 CM_I3 CM_I4 CM_N CM_I5 CM_N CM_I6 CM_I7 CM_N CM_I8 CM_N CM_I9 CM_I10 CM_I11 CM_N CM_I12 CM_N CM_I13 CM_I14
#define CM_BODY_D CM_I0 CM_N CM_I1 CM_N CM_I2 CM_N CM_I3 CM_N CM_I4 CM_N CM_I5 CM_N CM_I6 CM_N CM_I7 CM_N CM_I8 CM_N CM_I9 CM_N CM_I10 CM_N CM_I11 CM_N CM_I12 CM_N CM_I13 CM_N CM_I14
#define CM_BODY_E CM_I0 CM_I1 CM_I2 CM_I3 CM_I4 CM_I5 CM_I6 CM_I7 CM_I8 CM_N CM_I9 CM_I10 CM_I11 CM_I12 CM_I13 CM_I14
#define CM_BODY_F CM_I0 CM_N CM_I1 CM_N CM_I2 CM_N CM_I3 CM_N CM_I4 CM_I5 CM_I6 CM_N CM_I7 CM_I8 CM_I9 CM_N CM_I10 CM_N CM_I11 CM_I12 CM_I13 CM_N CM_I14
CM_KERNEL(pad_a, "s"(D), CM_Ks, , CM_BODY_A)
CM_KERNEL(pad_b, "s"(D), CM_Ks, , CM_BODY_B)
CM_KERNEL(pad_c, "s"(D), CM_Ks, , CM_BODY_C)
CM_KERNEL(pad_d, "s"(D), CM_Ks, , CM_BODY_D)
CM_KERNEL(pad_e, "s"(D), CM_Ks, , CM_BODY_E)
CM_KERNEL(pad_f, "s"(D), CM_Ks, , CM_BODY_F)
// the same pads on cellmix_v and cellmix_lit
CM_KERNEL(v_pad_a, "v"(D), CM_Kv, asm volatile("" : "+v"(D), "+v"(K0), "+v"(K1));, CM_BODY_A)
CM_KERNEL(v_pad_c, "v"(D), CM_Kv, asm volatile("" : "+v"(D), "+v"(K0), "+v"(K1));, CM_BODY_C)
CM_KERNEL(v_pad_e, "v"(D), CM_Kv, asm volatile("" : "+v"(D), "+v"(K0), "+v"(K1));, CM_BODY_E)
CM_KERNEL(v_pad_f, "v"(D), CM_Kv, asm volatile("" : "+v"(D), "+v"(K0), "+v"(K1));, CM_BODY_F)
CM_KERNEL(lit_pad_a, "n"(CM_LIT_D), CM_Kn, , CM_BODY_A)
CM_KERNEL(lit_pad_c, "n"(CM_LIT_D), CM_Kn, , CM_BODY_C)
CM_KERNEL(lit_pad_f, "n"(CM_LIT_D), CM_Kn, , CM_BODY_F)

#define RT_ADD "v_add_u32 %0, %0, %2\n\t"
#define RT_ADDS_0 ""
#define RT_ADDS_1 RT_ADD
#define RT_ADDS_2 RT_ADD RT_ADD
#define RT_ADDS_4 RT_ADDS_2 RT_ADDS_2
#define RT_ADDS_8 RT_ADDS_4 RT_ADDS_4
#define RT_KERNEL(k) \
__global__ void __launch_bounds__(256) k_ratio_##k(uint32_t* out, int iters, int dephase) { \
    uint32_t a = 0x20002000u + (threadIdx.x & 1u) * 0x00010001u, b = 0x10001000u, c = 0u; \
    asm volatile("" : "+v"(b), "+v"(c)); \
    const int skew = dephase ? int(((__builtin_amdgcn_s_getreg(4 | (3 << 11)) * 11u) % 15u) % (k + 1)) : 0; \
    if (skew > 0) asm volatile("v_pk_maximum3_f16 %0, %0, %1, %1" : "+v"(a) : "v"(b), "v"(c)); \
    for (int j = 1; j < skew; ++j) asm volatile("v_add_u32 %0, %0, %2" : "+v"(a) : "v"(b), "v"(c)); \
    for (int i = 0; i < iters; ++i) { \
        _Pragma("unroll") for (int u = 0; u < 8; ++u) asm volatile("v_pk_maximum3_f16 %0, %0, %1, %1\n\t" RT_ADDS_##k : "+v"(a) : "v"(b), "v"(c)); } \
    out[blockIdx.x * 256 + threadIdx.x] = a; }
RT_KERNEL(0) RT_KERNEL(1) RT_KERNEL(2) RT_KERNEL(4) RT_KERNEL(8)

// nop_*: ratio_2's body eight times in ONE asm statement, bare (the compiler puts nothing between the bodies) and with an s_nop 0 behind
// each, which is what the compiler puts between two asm statements when it has no scalar instruction for the wait state it keeps there
#define NP_BODY(pad) "v_pk_maximum3_f16 %0, %0, %1, %1\n\t" RT_ADDS_2 pad
#define NP_KERNEL(name, pad) \
__global__ void __launch_bounds__(256) k_nop_##name(uint32_t* out, int iters, int) { \
    uint32_t a = 0x20002000u + (threadIdx.x & 1u) * 0x00010001u, b = 0x10001000u, c = 0u; \
    asm volatile("" : "+v"(b), "+v"(c)); \
    for (int i = 0; i < iters; ++i) \
        asm volatile(NP_BODY(pad) NP_BODY(pad) NP_BODY(pad) NP_BODY(pad) NP_BODY(pad) NP_BODY(pad) NP_BODY(pad) NP_BODY(pad) : "+v"(a) : "v"(b), "v"(c)); \
    out[blockIdx.x * 256 + threadIdx.x] = a; }
NP_KERNEL(bare, "") NP_KERNEL(padded, "s_nop 0\n\t")

// bank_*: does the price of an instruction depend on which registers its vector sources are?  Eight independent chains on v40, v44, ...
// v68 (register number = 0 mod 4) as destination and first source; the other sources are v72 / v76 (0 mod 4 as well) or v73 / v74 /
// v77 (1, 2, 1 mod 4).  Physical registers are named in the asm; the values do not matter to the timing and nothing is addressed by them.
#define BK_CLOB "v40", "v44", "v48", "v52", "v56", "v60", "v64", "v68", "v72", "v73", "v74", "v76", "v77"
#define BK_8(I) I("v40") I("v44") I("v48") I("v52") I("v56") I("v60") I("v64") I("v68")
#define BK_KERNEL(name, I) \
__global__ void __launch_bounds__(256) k_bank_##name(uint32_t* out, int iters, int) { \
    asm volatile("v_mov_b32 v40, 0x20002000\n v_mov_b32 v44, 0x20012001\n v_mov_b32 v48, 0x20022002\n v_mov_b32 v52, 0x20032003\n" \
                 "v_mov_b32 v56, 0x20042004\n v_mov_b32 v60, 0x20052005\n v_mov_b32 v64, 0x20062006\n v_mov_b32 v68, 0x20072007\n" \
                 "v_mov_b32 v72, 0x10001000\n v_mov_b32 v73, 0x10011001\n v_mov_b32 v74, 0x10021002\n v_mov_b32 v76, 0x10031003\n v_mov_b32 v77, 0x10041004" ::: BK_CLOB); \
    for (int i = 0; i < iters; ++i) asm volatile(BK_8(I) BK_8(I) BK_8(I) BK_8(I) BK_8(I) BK_8(I) BK_8(I) BK_8(I) ::: BK_CLOB); \
    uint32_t r; asm volatile("v_xor_b32 %0, v40, v68" : "=v"(r) :: BK_CLOB); \
    out[blockIdx.x * 256 + threadIdx.x] = r; }
#define BK_ADD_SAME(c)   "v_add_u32 " c ", " c ", v72\n\t"
#define BK_ADD_DIFF(c)   "v_add_u32 " c ", " c ", v73\n\t"
#define BK_ADD_SGPR(c)   "v_add_u32 " c ", s10, " c "\n\t"
#define BK_MAX3_SAME(c)  "v_pk_maximum3_f16 " c ", " c ", v72, v76\n\t"
#define BK_MAX3_DIFF(c)  "v_pk_maximum3_f16 " c ", " c ", v73, v74\n\t"
#define BK_MAX3_TWO(c)   "v_pk_maximum3_f16 " c ", " c ", v73, v77\n\t"
#define BK_MAX3_SGPR(c)  "v_pk_maximum3_f16 " c ", " c ", v73, s10\n\t"
#define BK_MAX3_SGPR0(c) "v_pk_maximum3_f16 " c ", " c ", v72, s10\n\t"
#define BK_PKMAX_SAME(c) "v_pk_max_u16 " c ", " c ", v72\n\t"
#define BK_PKMAX_DIFF(c) "v_pk_max_u16 " c ", " c ", v73\n\t"
#define BK_PERM_SAME(c)  "v_perm_b32 " c ", " c ", v72, v76\n\t"
#define BK_PERM_DIFF(c)  "v_perm_b32 " c ", " c ", v73, v74\n\t"
BK_KERNEL(add_same, BK_ADD_SAME) BK_KERNEL(add_diff, BK_ADD_DIFF) BK_KERNEL(add_sgpr, BK_ADD_SGPR)
BK_KERNEL(max3_same, BK_MAX3_SAME) BK_KERNEL(max3_diff, BK_MAX3_DIFF) BK_KERNEL(max3_two, BK_MAX3_TWO) BK_KERNEL(max3_sgpr, BK_MAX3_SGPR) BK_KERNEL(max3_sgpr0, BK_MAX3_SGPR0)
BK_KERNEL(pkmax_same, BK_PKMAX_SAME) BK_KERNEL(pkmax_diff, BK_PKMAX_DIFF) BK_KERNEL(perm_same, BK_PERM_SAME) BK_KERNEL(perm_diff, BK_PERM_DIFF)

static int run_mix()
{
    const int cus = 256, iters = 4000;
    const int waves[4] = { 8, 5, 4, 3 };
    const size_t lds[4] = { 0, 32768, 40960, 49152 };        // 160 KiB of LDS per CU: as many blocks as fit
    uint32_t* out; CHECK(hipMalloc(&out, size_t(cus) * 8 * 256 * 4));
    hipEvent_t e0, e1; CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    const uint32_t D = CM_LIT_D, K0 = CM_LIT_K0, K1 = CM_LIT_K1, Z0 = 0x20002000u, Z1 = 0x20002000u;
    printf("cellmix: PD3::cell2's 15 instructions (9 slow: 2 v_perm_b32, 5 v_pk_maximum3_f16, 2 v_pk_max_u16; 6 simple: 4 v_add_u32, 2 v_subrev_u32), %d x 4 bodies per wave\n", iters);
    printf("cyc/body: SIMD-cycles per wave-body at 2.4 GHz, 1024 SIMDs.  simple@4.3: (cyc/body - 9 x 4.3) / 6\n");
    printf("%-12s %5s %6s %9s %6s %9s %10s %10s\n", "variant", "waves", "blk/CU", "phase", "skew", "ms", "cyc/body", "simple@4.3");
#define MIX(name) \
    for (int w = 0; w < 4; ++w) for (int ph = 0; ph < 2; ++ph) { \
        int occ = 0; CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_cellmix_##name, 256, lds[w])); \
        const int blocks = cus * waves[w]; \
        k_cellmix_##name<<<blocks, 256, lds[w]>>>(out, 10, ph, D, K0, K1, Z0, Z1); CHECK(hipDeviceSynchronize()); \
        float best = 1e30f; \
        for (int r = 0; r < 3; ++r) { \
            CHECK(hipEventRecord(e0)); k_cellmix_##name<<<blocks, 256, lds[w]>>>(out, iters, ph, D, K0, K1, Z0, Z1); CHECK(hipEventRecord(e1)); CHECK(hipEventSynchronize(e1)); \
            float ms; CHECK(hipEventElapsedTime(&ms, e0, e1)); if (ms < best) best = ms; } \
        const double bodies = double(blocks) * 4 * iters * 4, cyc = 1024.0 * 2.4e9 * best * 1e-3 / bodies; \
        printf("%-12s %5d %6d %9s %6s %9.3f %10.2f %10.2f\n", "cellmix_" #name, waves[w], occ, ph ? "de-phased" : "in-phase", ph ? "0-14" : "0", best, cyc, (cyc - 9 * 4.3) / 6); fflush(stdout); }
    MIX(s) MIX(v) MIX(lit)
    MIX(pad_a) MIX(pad_b) MIX(pad_c) MIX(pad_d) MIX(pad_e) MIX(pad_f)
    MIX(v_pad_a) MIX(v_pad_c) MIX(v_pad_e) MIX(v_pad_f) MIX(lit_pad_a) MIX(lit_pad_c) MIX(lit_pad_f)
#undef MIX
    printf("\nratio_k: one v_pk_maximum3_f16 and k dependent v_add_u32 on vector registers, 5 waves per SIMD, %d x 8 bodies per wave\n", iters);
    printf("%-12s %5s %6s %9s %9s %10s\n", "variant", "waves", "blk/CU", "phase", "ms", "cyc/body");
#define RATIO(k) \
    for (int ph = 0; ph < 2; ++ph) { \
        int occ = 0; CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_ratio_##k, 256, lds[1])); \
        const int blocks = cus * 5; \
        k_ratio_##k<<<blocks, 256, lds[1]>>>(out, 10, ph); CHECK(hipDeviceSynchronize()); \
        float best = 1e30f; \
        for (int r = 0; r < 3; ++r) { \
            CHECK(hipEventRecord(e0)); k_ratio_##k<<<blocks, 256, lds[1]>>>(out, iters, ph); CHECK(hipEventRecord(e1)); CHECK(hipEventSynchronize(e1)); \
            float ms; CHECK(hipEventElapsedTime(&ms, e0, e1)); if (ms < best) best = ms; } \
        const double bodies = double(blocks) * 4 * iters * 8; \
        printf("%-12s %5d %6d %9s %9.3f %10.2f\n", "ratio_" #k, 5, occ, ph ? "de-phased" : "in-phase", best, 1024.0 * 2.4e9 * best * 1e-3 / bodies); fflush(stdout); }
    RATIO(0) RATIO(1) RATIO(2) RATIO(4) RATIO(8)
#undef RATIO
    printf("\nnop_*: ratio_2's body, eight to one asm statement: bare, and with one s_nop 0 behind each body; 5 waves per SIMD\n");
    printf("%-12s %5s %6s %9s %9s %10s\n", "variant", "waves", "blk/CU", "", "ms", "cyc/body");
#define NOPROW(name) { \
        int occ = 0; CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_nop_##name, 256, lds[1])); \
        const int blocks = cus * 5; \
        k_nop_##name<<<blocks, 256, lds[1]>>>(out, 10, 0); CHECK(hipDeviceSynchronize()); \
        float best = 1e30f; \
        for (int r = 0; r < 3; ++r) { \
            CHECK(hipEventRecord(e0)); k_nop_##name<<<blocks, 256, lds[1]>>>(out, iters, 0); CHECK(hipEventRecord(e1)); CHECK(hipEventSynchronize(e1)); \
            float ms; CHECK(hipEventElapsedTime(&ms, e0, e1)); if (ms < best) best = ms; } \
        const double bodies = double(blocks) * 4 * iters * 8; \
        printf("%-12s %5d %6d %9s %9.3f %10.2f\n", "nop_" #name, 5, occ, "", best, 1024.0 * 2.4e9 * best * 1e-3 / bodies); fflush(stdout); }
    NOPROW(bare) NOPROW(padded)
#undef NOPROW
    printf("\nbank_*: eight independent chains, destination and first source 0 mod 4; same: the other vector sources 0 mod 4 too; diff: 1 and 2 mod 4; two: both 1 mod 4; sgpr: one scalar source\n");
    printf("%-16s %5s %6s %9s %10s\n", "variant", "waves", "blk/CU", "ms", "cyc/instr");
#define BANKROW(name) for (int w = 0; w < 2; ++w) { \
        int occ = 0; CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_bank_##name, 256, lds[w])); \
        const int blocks = cus * waves[w]; \
        k_bank_##name<<<blocks, 256, lds[w]>>>(out, 10, 0); CHECK(hipDeviceSynchronize()); \
        float best = 1e30f; \
        for (int r = 0; r < 3; ++r) { \
            CHECK(hipEventRecord(e0)); k_bank_##name<<<blocks, 256, lds[w]>>>(out, iters, 0); CHECK(hipEventRecord(e1)); CHECK(hipEventSynchronize(e1)); \
            float ms; CHECK(hipEventElapsedTime(&ms, e0, e1)); if (ms < best) best = ms; } \
        const double n = double(blocks) * 4 * iters * 64; \
        printf("%-16s %5d %6d %9.3f %10.2f\n", "bank_" #name, waves[w], occ, best, 1024.0 * 2.4e9 * best * 1e-3 / n); fflush(stdout); }
    BANKROW(add_same) BANKROW(add_diff) BANKROW(add_sgpr) BANKROW(max3_same) BANKROW(max3_diff) BANKROW(max3_two) BANKROW(max3_sgpr) BANKROW(max3_sgpr0)
    BANKROW(pkmax_same) BANKROW(pkmax_diff) BANKROW(perm_same) BANKROW(perm_diff)
#undef BANKROW
    return 0;
}

int main(int argc, char** argv)
{
    if (argc > 1 && argv[1][0] == 'm') return run_mix();
    const int blocks = 256 * 8, iters = 2000;            // 8 blocks of 4 waves per CU = 8 waves/SIMD
    uint32_t* out; CHECK(hipMalloc(&out, size_t(blocks) * 256 * 4));
    hipEvent_t e0, e1; CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    printf("%-14s %9s %12s %16s\n", "op", "ms", "Twave-op/s", "cyc/instr/SIMD@2.4");
#define X(name, str) { \
    k_##name<<<blocks, 256>>>(out, 10); CHECK(hipDeviceSynchronize()); \
    CHECK(hipEventRecord(e0)); k_##name<<<blocks, 256>>>(out, iters); CHECK(hipEventRecord(e1)); CHECK(hipEventSynchronize(e1)); \
    float ms; CHECK(hipEventElapsedTime(&ms, e0, e1)); \
    const double winstr = double(blocks) * 4 * iters * 64; \
    printf("%-14s %9.3f %12.4f %16.2f\n", #name, ms, winstr / ms / 1e9, 1024.0 * 2.4e9 / (winstr / (ms * 1e-3))); }
    OPS_LIST
#undef X
    return 0;
}
