// seam_split.h -- the three-plane truncation split of an fp32 value into bf16 pieces, shared by the kernels that run the fp32
// product on the bf16 matrix pipe (conv_igemm_sx in seam_conv.hip, conv1x1_sxpc in seam_pwsx.hip, conv3x3_wino24sx through
// seam_wino24_common.h).  The arithmetic is described at conv_igemm_sx.
#pragma once
#include <hip/hip_runtime.h>
#include "seam_device.h"

// top 16 bits of x as a float.  The opaque asm keeps each value its own register: without it hipcc (7.x) folds the four
// masked words of a vector into ONE operand of its v_pk_add_f32 (op_sel_hi:[1,0]) and every element loses the top piece of
// element 0 instead of its own -- found by the identity test, visible in the ISA.
__device__ __forceinline__ float top16(float x) {
    unsigned t = __builtin_bit_cast(unsigned, x) & 0xffff0000u;
    asm volatile("" : "+v"(t));
    return __builtin_bit_cast(float, t);
}

// four fp32 values -> their three bf16 pieces, 8 bytes per plane (element e of the vector in bf16 slot e).  As hipcc compiles it:
// 22 VALU instructions per f32x4, the second-level subtractions paired into two v_pk_add_f32 by the SLP pass.  The form of the
// kernels whose MFMA waves cut their own operands (conv_igemm_sx, conv3x3_wino24sx).
__device__ __forceinline__ void split3_bf16(const f32x4 v, u32x2& p0, u32x2& p1, u32x2& p2) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const float a0 = top16(v[2 * p]), b0 = top16(v[2 * p + 1]);
        const float ra = v[2 * p] - a0, rb = v[2 * p + 1] - b0;          // exact: <= 16 significand bits left
        const float a1 = top16(ra), b1 = top16(rb);
        const float sa = ra - a1, sb = rb - b1;                          // exact: <= 8 bits left, a bf16 as it stands
        p0[p] = (__builtin_bit_cast(unsigned, a0) >> 16) | __builtin_bit_cast(unsigned, b0);
        p1[p] = (__builtin_bit_cast(unsigned, a1) >> 16) | __builtin_bit_cast(unsigned, b1);
        p2[p] = (__builtin_bit_cast(unsigned, sa) >> 16) | (__builtin_bit_cast(unsigned, sb) & 0xffff0000u);
    }
}

// a - b as ONE v_sub_f32: written as asm so that the SLP pass cannot pair two of them into a v_pk_add_f32
__device__ __forceinline__ float sub1(float a, float b) {
    float d;
    asm("v_sub_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
    return d;
}

// the upper halves of two words as one: hi's in bits 31..16, lo's in bits 15..0 (one v_perm_b32: no mask, no shift)
__device__ __forceinline__ unsigned pack_hi16(float lo, float hi) {
    return __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, hi), __builtin_bit_cast(unsigned, lo), 0x07060302u);
}

// The same cut, the same bits, for the producer waves of conv1x1_sxpc and its kin, which share their SIMDs with the consumers'
// MFMAs: no packed fp32 instruction (two masks and two v_sub_f32 per level and pair, one v_perm_b32 per plane -- 22 VALU
// instructions per f32x4 again).  There a v_pk_add_f32 costs several plain subtractions: conv1x1_sxpc 295 -> 253 us on
// 40 x 50^2 x 1024 -> 256 without the two the compiler forms above (the last table of profiles/w24sx_l2_layer_ab.txt; 283 -> 250
// in the table with the roles of the libraries swapped); with all four subtractions packed by hand (18 instructions) it stays at
// the parent's time.  In the MFMA waves' own loops this form is level or slower, so they keep split3_bf16.
__device__ __forceinline__ void split3_bf16_single(const f32x4 v, u32x2& p0, u32x2& p1, u32x2& p2) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const float a = v[2 * p], b = v[2 * p + 1];
        const float ra = sub1(a, top16(a)), rb = sub1(b, top16(b));       // exact: <= 16 significand bits left
        const float sa = sub1(ra, top16(ra)), sb = sub1(rb, top16(rb));   // exact: <= 8 bits left, a bf16 as it stands
        p0[p] = pack_hi16(a, b);                                          // the truncation IS the top piece
        p1[p] = pack_hi16(ra, rb);
        p2[p] = pack_hi16(sa, sb);
    }
}
