// Device helpers shared by a forward kernel and its adjoint (seam_roialign.hip, seam_elementwise.hip, seam_conv.hip, seam_pw.hip,
// seam_pwh.hip, seam_fpn_train.hip) or by two kernels that must give the same bits (seam_input.hip): a gradient must go to the level /
// pixel the forward read, so both sides call ONE function.
#pragma once
#include <hip/hip_runtime.h>

namespace seam_fpn {

// LevelMapper: floor(4 + log2(sqrt(area)/224) + 1e-6), clamped to [k_min, k_min+3], every step an fp32 operation rounded
// correctly (the host's torch.log2 and the oracle): log2 in fp64, rounded once -- the fast log2f is an ulp off at some
// sizes within a few ulps of 112 / 224 / 448 * 2^-1e-6 and moved those boxes one level down
__device__ __forceinline__ int map_level(float x1, float y1, float x2, float y2, int k_min) {
    const float s = sqrtf((x2 - x1) * (y2 - y1));
    float l = floorf(4.f + (float)log2((double)(s / 224.f)) + 1e-6f);
    l = fminf(fmaxf(l, (float)k_min), (float)(k_min + 3));
    return (int)l - k_min;
}

// ATen upsample_nearest: source index of destination index `dst`, scale = (float)in / (float)out
__device__ __forceinline__ int nearest_src(int dst, float scale, int in_size) {
    return min((int)floorf((float)dst * scale), in_size - 1);
}

// One axis of the transform's bilinear resize: the two source taps and the weight of the second for destination index `dst`.  The
// preprocess kernels of seam_elementwise.hip and the batched uint8 one of seam_input.hip must give the same bits, so both call this.
__device__ __forceinline__ void bilinear_axis(int dst, int in, int out, int& i0, int& i1, float& l1) {
    // ATen upsample_bilinear2d, align_corners=False, scale = in/out (recompute_scale_factor=True)
    const float scale = (float)in / (float)out;
    float src = scale * ((float)dst + 0.5f) - 0.5f;
    if (src < 0.f) src = 0.f;
    int i = (int)src;
    if (i > in - 1) i = in - 1;
    i0 = i;
    i1 = (i < in - 1) ? i + 1 : i;
    float l = src - (float)i;
    l1 = fminf(fmaxf(l, 0.f), 1.f);
}

}  // namespace seam_fpn
