// seam_paste.h -- the one definition of a pasted mask pixel (paste_masks_in_image [TV]), shared by the paste kernel and the
// mask-intersection kernel of seam_detect.hip and by the RLE encoder of seam_rle.hip.
//
// Mask prob [K,1,28,28] zero-padded to 30x30, box expanded by 30/28 and truncated to int, bilinear (align_corners=False)
// resize of the padded map to the integer box size, pasted into [K,1,H,W] (zeros elsewhere).  The paste kernel writes the
// value, the mask-intersection kernel and the encoder threshold it, and all must agree to the bit.  So contraction is off in
// both functions and every fused multiply-add is spelled out (they are the ones the compiler used to pick for the plain
// expressions, which keeps seam_paste_masks_f32's results what they were): no caller can round differently.
#pragma once
#include <hip/hip_runtime.h>

namespace {

struct PasteBox {
    int x0, y0, x1, y1, bw, bh;     // the integer box (inclusive corners) and its size
    float sx, sy;                   // 30 / size: padded-map cells per pixel
};

__device__ __forceinline__ PasteBox paste_box(float4 bx) {
#pragma clang fp contract(off)
    PasteBox b;
    const float scale = 30.f / 28.f;
    const float wh = (bx.z - bx.x) * 0.5f * scale, hh = (bx.w - bx.y) * 0.5f * scale;
    const float xs = bx.z + bx.x, ys = bx.w + bx.y;
    b.x0 = (int)__builtin_fmaf(xs, 0.5f, -wh); b.y0 = (int)__builtin_fmaf(ys, 0.5f, -hh);    // trunc toward 0 (int64 cast)
    b.x1 = (int)__builtin_fmaf(xs, 0.5f, wh); b.y1 = (int)__builtin_fmaf(ys, 0.5f, hh);
    b.bw = max(b.x1 - b.x0 + 1, 1); b.bh = max(b.y1 - b.y0 + 1, 1);
    b.sx = 30.f / (float)b.bw; b.sy = 30.f / (float)b.bh;
    return b;
}

// value of pixel (y, x) of the pasted mask; m = the detection's 28x28 map (global or LDS)
__device__ __forceinline__ float paste_value(const float* m, const PasteBox& b, int y, int x) {
#pragma clang fp contract(off)
    const int ry = y - b.y0, rx = x - b.x0;
    if (!(ry >= 0 && ry < b.bh && rx >= 0 && rx < b.bw && y <= b.y1 && x <= b.x1)) return 0.f;
    float fy = __builtin_fmaf(b.sy, (float)ry + 0.5f, -0.5f), fx = __builtin_fmaf(b.sx, (float)rx + 0.5f, -0.5f);
    if (fy < 0.f) fy = 0.f;
    if (fx < 0.f) fx = 0.f;
    int iy = min((int)fy, 29), ix = min((int)fx, 29);
    const int iy1 = iy < 29 ? iy + 1 : iy, ix1 = ix < 29 ? ix + 1 : ix;
    const float ly = fminf(fmaxf(fy - (float)iy, 0.f), 1.f), lx = fminf(fmaxf(fx - (float)ix, 0.f), 1.f);
    auto at = [&](int yy, int xx) -> float {      // 30x30 zero-padded view of the 28x28 map
        return (yy >= 1 && yy <= 28 && xx >= 1 && xx <= 28) ? m[(yy - 1) * 28 + (xx - 1)] : 0.f;
    };
    const float top = __builtin_fmaf(1.f - lx, at(iy, ix), lx * at(iy, ix1));
    const float bot = __builtin_fmaf(1.f - lx, at(iy1, ix), lx * at(iy1, ix1));
    return __builtin_fmaf(1.f - ly, top, ly * bot);
}

}  // namespace
