// seam_masks.hip -- ground-truth masks on the device: COCO-style `segmentation` entries (polygon lists, RLE counts) rasterised
// into the uint8 [n,H,W] stacks that the mask loss and the segm AP read (ref datasets/DF2Dataset.py:152-155 builds them on the CPU
// with pycocotools' annToMask and copies n*H*W bytes per image).  The arithmetic restates maskApi.c's rleFrPoly / rleMerge /
// rleDecode operation for operation: vertices upsampled by 5 (on the host), every integer point of every edge in float64 with the
// multiply and the add kept apart, a crossing wherever the upsampled x changes onto a pixel centre, then a parity fill.
//
// Polygons, three kernels over a whole batch of objects (images of different sizes in one call):
//   toggle  one thread per emitted boundary point: finds its edge by binary search in the cumulative point table, recomputes the
//           point and its predecessor in closed form from the edge's integer ends, and flips bit y of column x of its part's
//           bitmap with an integer atomicXor (order-independent: two launches give the same bits; no float atomic anywhere).
//   scan    prefix-XOR down every column, inside each 32-bit word and carried across words: toggles become the packed mask.
//           Every image column carries an even number of crossings (tests/test_mask_refs_host.py pins that), so filling each
//           column on its own equals maskApi.c's fill of the sorted column-major positions.
//   expand  OR over the object's parts, one byte per pixel, row-major: a wave per row, 8 bytes per lane per store.
// A part's bitmap is [ceil((h+1)/32)][w] words (bit r&31 of word [r>>5][c]): rows 0..h, row h taking the crossings clamped to h;
// words of one row band lie along c, so the scan's and the expand's lanes read consecutive words.
// RLE: one kernel; a pixel binary-searches its column-major index in the object's run starts, its value is the run index & 1.
// toggle, scan and the row writer live in seam_masks_common.h (seam_input.hip expands the same bitmaps at another size).
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma STDC FP_CONTRACT OFF

#include "seam_masks_common.h"      // searches, toggle + scan (poly_fill), write_object: shared with seam_input.hip

namespace {

__global__ void poly_expand_kernel(const int* __restrict__ part_obj, const int64_t* __restrict__ part_ws_off,
                                   const int* __restrict__ obj_hw, const int64_t* __restrict__ obj_out_off,
                                   const uint32_t* __restrict__ ws, int64_t ws_words, uint8_t* __restrict__ out, int P, int n) {
    for (int o = blockIdx.y; o < n; o += gridDim.y) {
        const int h = obj_hw[2 * o], w = obj_hw[2 * o + 1];
        const int p0 = first_ge(part_obj, P, o);
        int p1 = first_ge(part_obj, P, o + 1);
        const int bands = (h + 32) >> 5;
        while (p1 > p0 && part_ws_off[p1 - 1] + (int64_t)bands * w > ws_words) --p1;    // never read past the workspace
        write_object(out + obj_out_off[o], h, w, [&](int r, int c, int m) -> uint64_t {
            uint32_t wd[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int p = p0; p < p1; ++p) {
                const uint32_t* src = ws + part_ws_off[p] + (int64_t)(r >> 5) * w + c;
                if (m == 8) {                                    // the 8 columns' words: 32 contiguous bytes, dword-aligned
                    uint32_t t[8];
                    __builtin_memcpy(t, src, 32);
                    for (int k = 0; k < 8; ++k) wd[k] |= t[k];
                } else {
                    for (int k = 0; k < m; ++k) wd[k] |= src[k];
                }
            }
            uint64_t pack = 0;
            for (int k = 0; k < 8; ++k) pack |= (uint64_t)((wd[k] >> (r & 31)) & 1u) << (8 * k);
            return pack;
        });
    }
}

__global__ void rle_expand_kernel(const int* __restrict__ run_start, const int* __restrict__ obj_run_off,
                                  const int* __restrict__ obj_hw, const int64_t* __restrict__ obj_out_off,
                                  uint8_t* __restrict__ out, int n) {
    for (int o = blockIdx.y; o < n; o += gridDim.y) {
        const int h = obj_hw[2 * o], w = obj_hw[2 * o + 1];
        const int r0 = obj_run_off[o], r1 = obj_run_off[o + 1];
        write_object(out + obj_out_off[o], h, w, [&](int r, int c, int m) -> uint64_t {
            uint64_t pack = 0;
            if (r1 <= r0) return pack;
            for (int k = 0; k < m; ++k)
                pack |= (uint64_t)((last_le(run_start, r0, r1, (int64_t)(c + k) * h + r) - r0) & 1) << (8 * k);
            return pack;
        });
    }
}

}  // namespace

extern "C" {

// words * 4 of one part's bitmap on an h x w image
int64_t seam_poly_masks_ws_bytes(int h, int w) {
    if (h <= 0 || w <= 0 || h > MAX_SIDE || w > MAX_SIDE) return 0;
    return (int64_t)((h + 32) >> 5) * w * 4;
}

int seam_poly_masks_u8(const int* pts, const int* part_off, const int* part_obj, const int* edge_pt_off,
                       const int64_t* part_ws_off, const int* obj_hw, const int64_t* obj_out_off, uint8_t* out, void* ws,
                       int64_t ws_bytes, int P, int V, int T, int n, void* stream) {
    if (P < 0 || V < 0 || T < 0 || n < 0 || ws_bytes < 0 || (ws_bytes & 3)) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    if (!obj_hw || !obj_out_off || !out) return (int)hipErrorInvalidValue;
    if (const int bad = poly_args_invalid(pts, part_off, part_obj, edge_pt_off, part_ws_off, ws, ws_bytes, P, V, T)) return bad;
    hipStream_t s = (hipStream_t)stream;
    const int64_t ws_words = ws_bytes >> 2;
    const hipError_t rc = poly_fill(pts, part_off, part_obj, edge_pt_off, part_ws_off, obj_hw, ws, ws_bytes, P, V, T, s);
    if (rc != hipSuccess) return (int)rc;
    hipLaunchKernelGGL(poly_expand_kernel, object_grid(n), dim3(256), 0, s, part_obj, part_ws_off, obj_hw, obj_out_off,
                       (const uint32_t*)ws, ws_words, out, P, n);
    return (int)hipGetLastError();
}

int seam_rle_masks_u8(const int* run_start, const int* obj_run_off, const int* obj_hw, const int64_t* obj_out_off, uint8_t* out,
                      int n, void* stream) {
    if (n < 0) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    if (!run_start || !obj_run_off || !obj_hw || !obj_out_off || !out) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(rle_expand_kernel, object_grid(n), dim3(256), 0, (hipStream_t)stream, run_start, obj_run_off, obj_hw,
                       obj_out_off, out, n);
    return (int)hipGetLastError();
}

}  // extern "C"
