// seam_split.h -- the three-plane truncation split of an fp32 value into bf16 pieces, shared by the kernels that run the fp32
// product on the bf16 matrix pipe (conv_igemm_sx in seam_conv.hip, conv1x1_sxpc in seam_pwsx.hip).  The arithmetic is described at
// conv_igemm_sx.
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

// four fp32 values -> their three bf16 pieces, 8 bytes per plane (element e of the vector in bf16 slot e)
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
