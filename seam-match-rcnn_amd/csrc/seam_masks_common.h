// seam_masks_common.h -- the stages of the ground-truth mask rasteriser that every expand form shares: the table searches, the
// polygon toggle + scan kernels that turn a batch of polygon parts into packed bitmaps (poly_fill launches them), and write_object,
// the row writer of an object's bytes.  seam_masks.hip expands the bitmaps and the RLE run tables at the image's own size,
// seam_input.hip at the size the model's transform resizes the image to (flipped where the sampler flipped it); both read the ONE
// definition of the bitmap here, so a mask and its resized form cannot disagree about a boundary pixel.
//
// The float64 arithmetic restates maskApi.c's rleFrPoly with the multiply and the add kept apart: contraction is off inside the
// functions that hold it (a file that includes this header keeps its own contraction mode everywhere else).
#pragma once
#include <hip/hip_runtime.h>
#include "seam_launch.h"
#include <stdint.h>

namespace {

constexpr int MAX_SIDE = 16384;

// largest i in [lo, hi) with tab[i] <= key; tab is non-decreasing and tab[lo] <= key
__device__ __forceinline__ int last_le(const int* __restrict__ tab, int lo, int hi, int64_t key) {
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (tab[mid] <= key) lo = mid; else hi = mid;
    }
    return lo;
}

// first i in [0, n] with tab[i] >= key (n if none)
__device__ __forceinline__ int first_ge(const int* __restrict__ tab, int n, int key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (tab[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

struct Pt { int u, v; };

// point `idx` (0 .. max(dx,dy)) of the edge (xs,ys) -> (xe,ye), counted from the edge's start (rleFrPoly's second loop).
// s*t is rounded to double before the add: a fused multiply-add rounds the half cases (s = 1/6, t = 3) the other way.  Plain
// operators with contraction off give that; HIP's __dmul_rn / __dadd_rn do NOT (they are inline `a * b` / `a + b` compiled
// under the header's contraction mode, and hipcc fuses them into v_fma_f64).
__device__ __forceinline__ Pt edge_point(int xs, int ys, int xe, int ye, int idx) {
#pragma clang fp contract(off)
    const int64_t dx = llabs((int64_t)xe - xs), dy = llabs((int64_t)ye - ys);
    const bool wide = dx >= dy;
    const bool flip = wide ? xs > xe : ys > ye;
    if (flip) {
        int t = xs; xs = xe; xe = t;
        t = ys; ys = ye; ye = t;
    }
    const int64_t len = wide ? dx : dy;
    Pt p;
    if (len == 0) {                       // zero-length edge: 0/0 in C; its v is never read (both neighbours share its u)
        p.u = xs; p.v = ys;
        return p;
    }
    const int64_t t = flip ? len - idx : idx;
    if (wide) {
        const double s = (double)((int64_t)ye - ys) / (double)dx;
        const double st = s * (double)t;
        p.u = (int)(t + xs);
        p.v = (int)((double)ys + st + 0.5);
    } else {
        const double s = (double)((int64_t)xe - xs) / (double)dy;
        const double st = s * (double)t;
        p.v = (int)(t + ys);
        p.u = (int)((double)xs + st + 0.5);
    }
    return p;
}

// point `idx` of ring edge e of the part whose vertices are [v0, v1): vertex e -> vertex e+1, the last edge back to v0
__device__ __forceinline__ Pt ring_point(const int* __restrict__ pts, int v0, int v1, int e, int idx) {
    const int e1 = e + 1 < v1 ? e + 1 : v0;
    return edge_point(pts[2 * e], pts[2 * e + 1], pts[2 * e1], pts[2 * e1 + 1], idx);
}

__global__ void poly_toggle_kernel(const int* __restrict__ pts, const int* __restrict__ part_off, const int* __restrict__ part_obj,
                                   const int* __restrict__ edge_pt_off, const int64_t* __restrict__ part_ws_off,
                                   const int* __restrict__ obj_hw, uint32_t* __restrict__ ws, int64_t ws_words, int P, int V, int T) {
#pragma clang fp contract(off)
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < T; g += (int64_t)gridDim.x * blockDim.x) {
        const int e = last_le(edge_pt_off, 0, V, g);
        const int p = last_le(part_off, 0, P, e);
        const int v0 = part_off[p], v1 = part_off[p + 1];
        const int first = edge_pt_off[e];
        if (e == v0 && g == first) continue;                         // the ring's first point has no predecessor
        const Pt b = ring_point(pts, v0, v1, e, (int)(g - first));
        const Pt a = g > first ? ring_point(pts, v0, v1, e, (int)(g - first) - 1)
                               : ring_point(pts, v0, v1, e - 1, first - 1 - edge_pt_off[e - 1]);
        if (a.u == b.u) continue;
        const int o = part_obj[p];
        const int h = obj_hw[2 * o], w = obj_hw[2 * o + 1];
        double xd = (double)(b.u < a.u ? b.u : b.u - 1);
        xd = (xd + 0.5) / 5.0 - 0.5;
        if (floor(xd) != xd || xd < 0.0 || xd > (double)(w - 1)) continue;
        double yd = (double)(b.v < a.v ? b.v : a.v);
        yd = (yd + 0.5) / 5.0 - 0.5;
        if (yd < 0.0) yd = 0.0; else if (yd > (double)h) yd = (double)h;
        const int x = (int)xd, y = (int)ceil(yd);
        const int64_t word = part_ws_off[p] + (int64_t)(y >> 5) * w + x;
        if (word < ws_words) atomicXor(ws + word, 1u << (y & 31));
    }
}

__global__ void poly_scan_kernel(const int* __restrict__ part_obj, const int64_t* __restrict__ part_ws_off,
                                 const int* __restrict__ obj_hw, uint32_t* __restrict__ ws, int64_t ws_words, int P) {
    for (int p = blockIdx.y; p < P; p += gridDim.y) {
        const int o = part_obj[p];
        const int h = obj_hw[2 * o], w = obj_hw[2 * o + 1];
        const int bands = (h + 32) >> 5;                             // ceil((h + 1) / 32)
        const int64_t base = part_ws_off[p];
        if (base + (int64_t)bands * w > ws_words) continue;
        for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < w; c += gridDim.x * blockDim.x) {
            uint32_t carry = 0;
            for (int k = 0; k < bands; ++k) {
                uint32_t x = ws[base + (int64_t)k * w + c];
                x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8; x ^= x << 16;
                x ^= carry;
                ws[base + (int64_t)k * w + c] = x;
                carry = 0u - (x >> 31);
            }
        }
    }
}

// Writes an object's [h,w] bytes row by row: a wave takes one row per pass and its lanes consecutive 8-byte-aligned chunks of the
// row's address range, stored whole; the chunks cut by the row's first and last byte are stored byte by byte, so any output
// offset and any w work.  row(r, c, n) returns the bytes of pixels (r, c .. c+n-1), n <= 8, pixel c + k in byte k.
template <class Row>
__device__ __forceinline__ void write_object(uint8_t* __restrict__ dst, int h, int w, Row row) {
    const int lane = threadIdx.x & 63, rows_per_pass = blockDim.x >> 6;
    for (int r = blockIdx.x * rows_per_pass + (threadIdx.x >> 6); r < h; r += gridDim.x * rows_per_pass) {
        uint8_t* rp = dst + (int64_t)r * w;
        const int head = (int)((uintptr_t)rp & 7);
        const int chunks = (w + head + 7) >> 3;
        for (int q = lane; q < chunks; q += 64) {
            const int i0 = q * 8 - head;
            const int lo = i0 < 0 ? 0 : i0, hi = i0 + 8 < w ? i0 + 8 : w;
            const uint64_t pack = row(r, lo, hi - lo);
            if (hi - lo == 8) {
                *reinterpret_cast<uint64_t*>(rp + lo) = pack;
            } else {
                for (int k = 0; k < hi - lo; ++k) rp[lo + k] = (uint8_t)(pack >> (8 * k));
            }
        }
    }
}

inline dim3 object_grid(int n) { return dim3(64, (unsigned)(n < 65535 ? n : 65535)); }

// The argument rules the two polygon entry points share (0: go on; anything else: the code to return)
inline int poly_args_invalid(const int* pts, const int* part_off, const int* part_obj, const int* edge_pt_off,
                             const int64_t* part_ws_off, const void* ws, int64_t ws_bytes, int P, int V, int T) {
    if (P > 0 && (!part_off || !part_obj || !part_ws_off || !ws || ws_bytes == 0)) return (int)hipErrorInvalidValue;
    if (T > 0 && (P == 0 || V == 0 || T < V || !pts || !edge_pt_off)) return (int)hipErrorInvalidValue;
    return 0;
}

// clear + toggle + scan: afterwards bit r&31 of word [r>>5][c] of part p's bitmap (at ws + part_ws_off[p]) is pixel (r, c)
inline hipError_t poly_fill(const int* pts, const int* part_off, const int* part_obj, const int* edge_pt_off,
                            const int64_t* part_ws_off, const int* obj_hw, void* ws, int64_t ws_bytes, int P, int V, int T,
                            hipStream_t s) {
    if (P <= 0) return hipSuccess;
    const int64_t ws_words = ws_bytes >> 2;
    hipError_t rc = hipMemsetAsync(ws, 0, (size_t)ws_bytes, s);
    if (rc != hipSuccess) return rc;
    if (T > 0) {
        const unsigned grid = seam_launch::grid256(T);
        hipLaunchKernelGGL(poly_toggle_kernel, dim3(grid), dim3(256), 0, s, pts, part_off, part_obj, edge_pt_off, part_ws_off,
                           obj_hw, (uint32_t*)ws, ws_words, P, V, T);
    }
    hipLaunchKernelGGL(poly_scan_kernel, dim3(8, (unsigned)(P < 65535 ? P : 65535)), dim3(256), 0, s, part_obj, part_ws_off,
                       obj_hw, (uint32_t*)ws, ws_words, P);
    return hipSuccess;
}

}  // namespace
