// seam_input.hip -- the input stage of a training step (ref train_matchrcnn.py + stuffs/engine.py:38-39) for a batch that crossed
// the bus as image bytes and annotation integers:
//   preprocess_u8_batch  N uint8 HWC images of different sizes in one flat buffer -> ToTensor (/255) + horizontal flip + normalise
//                        + bilinear resize + pad + layout (NHWC4 or the space-to-depth frame of the stem) in ONE launch.
//   masks, resized       the polygon bitmaps / RLE run tables of seam_masks_common.h expanded straight at the size the transform
//                        resizes the image to, flipped where the image is: the original-size uint8 stack is never written.
// The image arithmetic is that of preprocess_kernel / preprocess_s2d_kernel (seam_elementwise.hip) on byte / 255.f, expression for
// expression, so that a batch prepared here and one that went through the host's to_tensor + flip + the fp32 kernels are the same
// bits (tests/test_gpu_input_batch.py); a flipped image reads source column in_w - 1 - x for the taps of flipped column x.
// Pixels are 3 bytes: an image's offset and an odd row length are not dword-aligned, so every load is a byte load; stores are
// 16-byte vectors.
#include <hip/hip_runtime.h>
#include "seam_device.h"
#include <stdint.h>

#include "seam_fpn_common.h"
#include "seam_masks_common.h"

namespace {

using seam_fpn::bilinear_axis;

struct ImageDims { int in_h, in_w, out_h, out_w, flip; };

// colour c of output pixel (y, x) of an image, y < out_h and x < out_w
__device__ __forceinline__ void pixel(const uint8_t* __restrict__ img, const ImageDims& d, int y, int x, float v[3]) {
    const float mean[3] = {0.485f, 0.456f, 0.406f};
    const float stdv[3] = {0.229f, 0.224f, 0.225f};
    const int in_w = d.in_w;
    if (d.out_h == d.in_h && d.out_w == in_w) {
        const uint8_t* p = img + ((size_t)y * in_w + (d.flip ? in_w - 1 - x : x)) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float t = (float)p[c] / 255.f;
            v[c] = (t - mean[c]) / stdv[c];
        }
        return;
    }
    int y0, y1, x0, x1;
    float ly, lx;
    bilinear_axis(y, d.in_h, d.out_h, y0, y1, ly);
    bilinear_axis(x, in_w, d.out_w, x0, x1, lx);
    const float hy = 1.f - ly, hx = 1.f - lx;
    if (d.flip) { x0 = in_w - 1 - x0; x1 = in_w - 1 - x1; }
    const uint8_t* p00 = img + ((size_t)y0 * in_w + x0) * 3;
    const uint8_t* p01 = img + ((size_t)y0 * in_w + x1) * 3;
    const uint8_t* p10 = img + ((size_t)y1 * in_w + x0) * 3;
    const uint8_t* p11 = img + ((size_t)y1 * in_w + x1) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float t00 = (float)p00[c] / 255.f, t01 = (float)p01[c] / 255.f;
        const float t10 = (float)p10[c] / 255.f, t11 = (float)p11[c] / 255.f;
        const float v00 = (t00 - mean[c]) / stdv[c];
        const float v01 = (t01 - mean[c]) / stdv[c];
        const float v10 = (t10 - mean[c]) / stdv[c];
        const float v11 = (t11 - mean[c]) / stdv[c];
        v[c] = hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11);
    }
}

// grid (x blocks, rows, images).  S2D: a thread writes one cell = pixels (2Y..2Y+1, 2X..2X+1), channel (dy*2 + dx)*3 + c, 48 bytes;
// else one NHWC4 pixel, 16 bytes.  An image whose table entry does not fit the buffer or the frame is written as zeros.
template <bool S2D>
__global__ void preprocess_u8_batch_kernel(const uint8_t* __restrict__ imgs, int64_t imgs_bytes, const int64_t* __restrict__ img_off,
                                           const int* __restrict__ img_dims, float* __restrict__ out, int Hp, int Wp) {
    const int X = blockIdx.x * blockDim.x + threadIdx.x;
    const int Y = blockIdx.y;
    const int n = blockIdx.z;
    const int Wc = S2D ? Wp >> 1 : Wp, Hc = S2D ? Hp >> 1 : Hp;
    if (X >= Wc) return;
    const int* t = img_dims + 5 * n;
    ImageDims d = {t[0], t[1], t[2], t[3], t[4]};
    const int64_t off = img_off[n];
    const bool ok = d.in_h > 0 && d.in_w > 0 && d.out_h > 0 && d.out_w > 0 && d.out_h <= Hp && d.out_w <= Wp && off >= 0 &&
                    off + (int64_t)d.in_h * d.in_w * 3 <= imgs_bytes;
    if (!ok) d.out_h = d.out_w = 0;
    const uint8_t* img = imgs + off;
    if constexpr (S2D) {
        float o[12];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int y = 2 * Y + (q >> 1), x = 2 * X + (q & 1);
            float v[3] = {0.f, 0.f, 0.f};
            if (y < d.out_h && x < d.out_w) pixel(img, d, y, x, v);
#pragma unroll
            for (int c = 0; c < 3; ++c) o[q * 3 + c] = v[c];
        }
        float* dst = out + (((size_t)n * Hc + Y) * Wc + X) * 12;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            f32x4 v4 = {o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]};
            *reinterpret_cast<f32x4*>(dst + 4 * q) = v4;
        }
    } else {
        float v[3] = {0.f, 0.f, 0.f};
        if (Y < d.out_h && X < d.out_w) pixel(img, d, Y, X, v);
        f32x4 v4 = {v[0], v[1], v[2], 0.f};
        *reinterpret_cast<f32x4*>(out + (((size_t)n * Hc + Y) * Wc + X) * 4) = v4;
    }
}

// ---------------------------------------------------------------------------------------------------- masks at the resized size
// obj_out int32 [n][3] = (out_h, out_w, flip): output pixel (r, c) of object o is source pixel (sy(r), flip ? w-1-sx(c) : sx(c)),
// sy / sx = ATen's nearest rule (seam_fpn::nearest_src) with scale = (float)in / (float)out -- resize_masks_nearest on the host.
struct ResizeMap {
    int h, w, oh, ow, flip;
    float ys, xs;
    __device__ __forceinline__ int row(int r) const { return seam_fpn::nearest_src(r, ys, h); }
    __device__ __forceinline__ int col(int c) const {
        const int s = seam_fpn::nearest_src(c, xs, w);
        return flip ? w - 1 - s : s;
    }
};

__device__ __forceinline__ bool resize_map(const int* __restrict__ obj_hw, const int* __restrict__ obj_out,
                                           const int64_t* __restrict__ obj_out_off, int64_t out_bytes, int o, ResizeMap& m) {
    m.h = obj_hw[2 * o]; m.w = obj_hw[2 * o + 1];
    m.oh = obj_out[3 * o]; m.ow = obj_out[3 * o + 1]; m.flip = obj_out[3 * o + 2];
    if (m.h <= 0 || m.w <= 0 || m.h > MAX_SIDE || m.w > MAX_SIDE) return false;        // the bound of seam_poly_masks_ws_bytes
    if (m.oh <= 0 || m.ow <= 0 || m.oh > MAX_SIDE || m.ow > MAX_SIDE) return false;
    const int64_t off = obj_out_off[o];
    if (off < 0 || off + (int64_t)m.oh * m.ow > out_bytes) return false;        // never write past the output
    m.ys = (float)m.h / (float)m.oh;
    m.xs = (float)m.w / (float)m.ow;
    return true;
}

__global__ void poly_expand_resized_kernel(const int* __restrict__ part_obj, const int64_t* __restrict__ part_ws_off,
                                           const int* __restrict__ obj_hw, const int* __restrict__ obj_out,
                                           const int64_t* __restrict__ obj_out_off, const uint32_t* __restrict__ ws, int64_t ws_words,
                                           uint8_t* __restrict__ out, int64_t out_bytes, int P, int n) {
    for (int o = blockIdx.y; o < n; o += gridDim.y) {
        ResizeMap m;
        if (!resize_map(obj_hw, obj_out, obj_out_off, out_bytes, o, m)) continue;
        const int p0 = first_ge(part_obj, P, o);
        int p1 = first_ge(part_obj, P, o + 1);
        const int bands = (m.h + 32) >> 5;
        while (p1 > p0 && part_ws_off[p1 - 1] + (int64_t)bands * m.w > ws_words) --p1;  // never read past the workspace
        write_object(out + obj_out_off[o], m.oh, m.ow, [&](int r, int c, int cnt) -> uint64_t {
            const int sr = m.row(r);
            uint64_t pack = 0;
            for (int k = 0; k < cnt; ++k) {
                const int sc = m.col(c + k);
                uint32_t wd = 0;
                for (int p = p0; p < p1; ++p) wd |= ws[part_ws_off[p] + (int64_t)(sr >> 5) * m.w + sc];
                pack |= (uint64_t)((wd >> (sr & 31)) & 1u) << (8 * k);
            }
            return pack;
        });
    }
}

__global__ void rle_expand_resized_kernel(const int* __restrict__ run_start, const int* __restrict__ obj_run_off,
                                          const int* __restrict__ obj_hw, const int* __restrict__ obj_out,
                                          const int64_t* __restrict__ obj_out_off, uint8_t* __restrict__ out, int64_t out_bytes, int n) {
    for (int o = blockIdx.y; o < n; o += gridDim.y) {
        ResizeMap m;
        if (!resize_map(obj_hw, obj_out, obj_out_off, out_bytes, o, m)) continue;
        const int r0 = obj_run_off[o], r1 = obj_run_off[o + 1];
        write_object(out + obj_out_off[o], m.oh, m.ow, [&](int r, int c, int cnt) -> uint64_t {
            uint64_t pack = 0;
            if (r1 <= r0) return pack;
            const int sr = m.row(r);
            for (int k = 0; k < cnt; ++k)
                pack |= (uint64_t)((last_le(run_start, r0, r1, (int64_t)m.col(c + k) * m.h + sr) - r0) & 1) << (8 * k);
            return pack;
        });
    }
}

}  // namespace

extern "C" {

int seam_preprocess_u8_batch_f32(const uint8_t* imgs, int64_t imgs_bytes, const int64_t* img_off, const int* img_dims, float* out,
                                 int n, int Hp, int Wp, int s2d, void* stream) {
    if (n < 1 || n > 65535 || Hp < 1 || Wp < 1 || Hp > 65535 || imgs_bytes < 0) return (int)hipErrorInvalidValue;
    if (s2d && ((Hp | Wp) & 1)) return (int)hipErrorInvalidValue;
    if (!imgs || !img_off || !img_dims || !out) return (int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    if (s2d) {
        const dim3 grid((unsigned)((Wp / 2 + 127) / 128), (unsigned)(Hp / 2), (unsigned)n);
        hipLaunchKernelGGL(preprocess_u8_batch_kernel<true>, grid, dim3(128), 0, s, imgs, imgs_bytes, img_off, img_dims, out, Hp, Wp);
    } else {
        const dim3 grid((unsigned)((Wp + 255) / 256), (unsigned)Hp, (unsigned)n);
        hipLaunchKernelGGL(preprocess_u8_batch_kernel<false>, grid, dim3(256), 0, s, imgs, imgs_bytes, img_off, img_dims, out, Hp, Wp);
    }
    return (int)hipGetLastError();
}

int seam_poly_masks_resized_u8(const int* pts, const int* part_off, const int* part_obj, const int* edge_pt_off,
                               const int64_t* part_ws_off, const int* obj_hw, const int* obj_out, const int64_t* obj_out_off,
                               uint8_t* out, int64_t out_bytes, void* ws, int64_t ws_bytes, int P, int V, int T, int n, void* stream) {
    if (P < 0 || V < 0 || T < 0 || n < 0 || out_bytes < 0 || ws_bytes < 0 || (ws_bytes & 3)) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    if (!obj_hw || !obj_out || !obj_out_off || !out) return (int)hipErrorInvalidValue;
    if (const int bad = poly_args_invalid(pts, part_off, part_obj, edge_pt_off, part_ws_off, ws, ws_bytes, P, V, T)) return bad;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t rc = poly_fill(pts, part_off, part_obj, edge_pt_off, part_ws_off, obj_hw, ws, ws_bytes, P, V, T, s);
    if (rc != hipSuccess) return (int)rc;
    hipLaunchKernelGGL(poly_expand_resized_kernel, object_grid(n), dim3(256), 0, s, part_obj, part_ws_off, obj_hw, obj_out, obj_out_off,
                       (const uint32_t*)ws, ws_bytes >> 2, out, out_bytes, P, n);
    return (int)hipGetLastError();
}

int seam_rle_masks_resized_u8(const int* run_start, const int* obj_run_off, const int* obj_hw, const int* obj_out,
                              const int64_t* obj_out_off, uint8_t* out, int64_t out_bytes, int n, void* stream) {
    if (n < 0 || out_bytes < 0) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    if (!run_start || !obj_run_off || !obj_hw || !obj_out || !obj_out_off || !out) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(rle_expand_resized_kernel, object_grid(n), dim3(256), 0, (hipStream_t)stream, run_start, obj_run_off, obj_hw,
                       obj_out, obj_out_off, out, out_bytes, n);
    return (int)hipGetLastError();
}

}  // extern "C"
