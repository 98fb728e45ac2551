// Device helpers shared by the training kernels (seam_roi_train.hip, seam_rpn_train.hip): fixed-order block sums, the
// order-preserving float key of the samplers, and torchvision's box_iou element in its fp32 expression order.
#pragma once
#include <hip/hip_runtime.h>
#include "seam_device.h"

namespace seam_train {

// fixed-order sum over a 256-thread block (4 waves).  Deliberately not seam_device.h's block_sum: this one associates
// (r0 + r1) + (r2 + r3) and ends in a barrier (`red` is free again on return); merging the two would change last bits.
__device__ __forceinline__ float block_sum256(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float r = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return r;
}

// float -> unsigned with the same order (negative keys below positive ones)
__device__ __forceinline__ unsigned ord_key(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// torchvision box_iou(gt, proposals) element, in its expression order and without FMA contraction
__device__ __forceinline__ float iou_gt_prop(float4 g, float area_g, float4 p, float area_p) {
#pragma clang fp contract(off)
    const float iw = fmaxf(fminf(g.z, p.z) - fmaxf(g.x, p.x), 0.f);
    const float ih = fmaxf(fminf(g.w, p.w) - fmaxf(g.y, p.y), 0.f);
    const float inter = iw * ih;
    return inter / ((area_g + area_p) - inter);
}

__device__ __forceinline__ float box_area(float4 b) {
#pragma clang fp contract(off)
    return (b.z - b.x) * (b.w - b.y);
}

}  // namespace seam_train
