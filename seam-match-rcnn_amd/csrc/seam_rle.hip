// seam_rle.hip -- masks to COCO run-length encoding on the device (maskApi.c's rleEncode): the opposite direction of
// seam_masks.hip.  The RLE of a mask is the ascending list of column-major positions p = x*h + y at which the value changes,
// v(p) != v(p-1) with v(-1) = 0; the pixel before (0, x) is (h-1, x-1), so a run continues from the bottom of one column into
// the top of the next.  counts = diff([0, positions..., h*w]) is made on the host from a few hundred integers per object.
//
// An object's workspace is the rasteriser's bitmap layout, [ceil(h/32)][w] 32-bit words (bit r&31 of word [r>>5][c]): words of
// one row band lie along c, so a wave's lanes read consecutive bytes of a row-major mask and consecutive words of the bitmap.
//   values     one thread per (band, column) word: reads its 32 bytes (dense masks) or evaluates paste_value > 0.5 for its
//              rows inside the clipped integer box (detections; the 28x28 map sits in LDS) and stores the packed value bits.
//              Every pixel is read or evaluated exactly once.
//   count      transitions of a word = v ^ (v << 1 | carry), the carry being the top bit of the band above or, for band 0, the
//              last row's bit of the previous column: two word reads, no pixel is touched again.  Stores the popcount in
//              column-major order of the cells (column, then band), the order the positions come out in.
//   (scan)     an inclusive prefix sum over the whole batch's count table -- the caller's; it is also the CSR of the objects.
//   positions  the same transition word again; its set bits go to positions[scan - popcount ...], every slot written once at
//              a computed offset.  No atomics anywhere: two launches give identical bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "seam_paste.h"

namespace {

constexpr int MAX_SIDE = 16384;        // as seam_masks.hip

inline int64_t cells_of(int h, int w) { return (int64_t)((h + 31) >> 5) * w; }
inline bool side_ok(int h, int w) { return h >= 1 && w >= 1 && h <= MAX_SIDE && w <= MAX_SIDE && (int64_t)h * w < (int64_t(1) << 31); }

// Where the objects' shapes come from: tables (dense masks, any mix of sizes) or one shape for all (detections of an image).
struct Objs {
    const int* hw;                 // [n,2] or NULL
    const int64_t* cell_off;       // [n] first word of each object, with hw
    int h, w;                      // without hw
};

struct Obj { int h, w, bands; int64_t base; bool ok; };

__device__ __forceinline__ Obj obj_get(const Objs& t, int o, int64_t ws_words) {
    Obj r;
    if (t.hw) { r.h = t.hw[2 * o]; r.w = t.hw[2 * o + 1]; r.base = t.cell_off[o]; }
    else { r.h = t.h; r.w = t.w; r.base = (int64_t)o * (((t.h + 31) >> 5) * (int64_t)t.w); }
    r.ok = r.h >= 1 && r.w >= 1 && r.h <= MAX_SIDE && r.w <= MAX_SIDE;
    r.bands = r.ok ? (r.h + 31) >> 5 : 0;
    r.ok = r.ok && r.base >= 0 && r.base + (int64_t)r.bands * r.w <= ws_words;      // never touch words outside the workspace
    return r;
}

__global__ __launch_bounds__(256) void rle_values_u8_kernel(const uint8_t* __restrict__ masks, int64_t mask_bytes,
                                                            const int64_t* __restrict__ obj_off, Objs t,
                                                            uint32_t* __restrict__ ws, int64_t ws_words, int n) {
    for (int o = blockIdx.y; o < n; o += gridDim.y) {
        const Obj b = obj_get(t, o, ws_words);
        const int64_t off = obj_off[o];
        if (!b.ok || off < 0 || off + (int64_t)b.h * b.w > mask_bytes) continue;
        const uint8_t* m = masks + off;
        const int cells = b.bands * b.w;                              // <= 512 * 16384
        for (int i = blockIdx.x * 256 + threadIdx.x; i < cells; i += gridDim.x * 256) {
            const int k = i / b.w, c = i - k * b.w;
            const int r0 = k << 5, nr = min(32, b.h - r0);
            const uint8_t* p = m + (int64_t)r0 * b.w + c;
            uint32_t v = 0;
            if (nr == 32) {
#pragma unroll
                for (int r = 0; r < 32; ++r) v |= (uint32_t)(p[(int64_t)r * b.w] != 0) << r;
            } else {
                for (int r = 0; r < nr; ++r) v |= (uint32_t)(p[(int64_t)r * b.w] != 0) << r;
            }
            ws[b.base + i] = v;
        }
    }
}

// The workspace was cleared: only the words that the clipped integer box touches are written.
__global__ __launch_bounds__(256) void rle_values_paste_kernel(const float* __restrict__ probs, const float* __restrict__ boxes,
                                                               int D, int H, int W, uint32_t* __restrict__ ws, int64_t ws_words) {
    __shared__ float sm[784];
    const int64_t cells = (int64_t)((H + 31) >> 5) * W;
    for (int d = blockIdx.y; d < D; d += gridDim.y) {
        const PasteBox b = paste_box(reinterpret_cast<const float4*>(boxes)[d]);
        const int xlo = max(b.x0, 0), xhi = min(b.x1, W - 1), ylo = max(b.y0, 0), yhi = min(b.y1, H - 1);
        if (xlo > xhi || ylo > yhi) continue;                         // block-uniform: nothing of the box inside the image
        const int k0 = ylo >> 5, ncol = xhi - xlo + 1, total = ((yhi >> 5) - k0 + 1) * ncol;
        if ((int)(blockIdx.x * 256) >= total || ((int64_t)d + 1) * cells > ws_words) continue;
        __syncthreads();                                              // the previous detection's readers are done with sm
        for (int i = threadIdx.x; i < 784; i += 256) sm[i] = probs[(size_t)d * 784 + i];
        __syncthreads();
        for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
            const int kk = i / ncol;
            const int k = k0 + kk, x = xlo + (i - kk * ncol);
            const int ya = max(ylo, k << 5), yb = min(yhi, (k << 5) + 31);
            uint32_t v = 0;
            for (int y = ya; y <= yb; ++y) v |= (uint32_t)(paste_value(sm, b, y, x) > 0.5f) << (y & 31);
            ws[(int64_t)d * cells + (int64_t)k * W + x] = v;
        }
    }
}

// transition bits of word (band k, column c) of an object whose value words start at wsb
__device__ __forceinline__ uint32_t transitions(const uint32_t* __restrict__ wsb, const Obj& b, int k, int c) {
    const uint32_t v = wsb[k * b.w + c];
    uint32_t carry = 0;
    if (k > 0) carry = wsb[(k - 1) * b.w + c] >> 31;
    else if (c > 0) carry = (wsb[(b.bands - 1) * b.w + c - 1] >> ((b.h - 1) & 31)) & 1u;
    uint32_t t = v ^ ((v << 1) | carry);
    const int nr = b.h - (k << 5);
    if (nr < 32) t &= (1u << nr) - 1u;                                // rows past h do not exist
    return t;
}

__global__ __launch_bounds__(256) void rle_count_kernel(Objs t, const uint32_t* __restrict__ ws, int64_t ws_words,
                                                        int* __restrict__ counts, int n) {
    for (int o = blockIdx.y; o < n; o += gridDim.y) {
        const Obj b = obj_get(t, o, ws_words);
        if (!b.ok) continue;
        const int cells = b.bands * b.w;
        for (int i = blockIdx.x * 256 + threadIdx.x; i < cells; i += gridDim.x * 256) {
            const int k = i / b.w, c = i - k * b.w;
            counts[b.base + (int64_t)c * b.bands + k] = __popc(transitions(ws + b.base, b, k, c));
        }
    }
}

__global__ __launch_bounds__(256) void rle_positions_kernel(Objs t, const uint32_t* __restrict__ ws, int64_t ws_words,
                                                            const int64_t* __restrict__ scan, int* __restrict__ positions,
                                                            int64_t capacity, int n) {
    for (int o = blockIdx.y; o < n; o += gridDim.y) {
        const Obj b = obj_get(t, o, ws_words);
        if (!b.ok) continue;
        const int cells = b.bands * b.w;
        for (int i = blockIdx.x * 256 + threadIdx.x; i < cells; i += gridDim.x * 256) {
            const int k = i / b.w, c = i - k * b.w;
            uint32_t tr = transitions(ws + b.base, b, k, c);
            if (!tr) continue;
            const int64_t end = scan[b.base + (int64_t)c * b.bands + k];
            int64_t q = end - __popc(tr);
            if (q < 0 || end > capacity) continue;                    // a scan that is not this table's: write nothing
            const int p0 = c * b.h + (k << 5);
            while (tr) {
                positions[q++] = p0 + __ffs((int)tr) - 1;
                tr &= tr - 1u;
            }
        }
    }
}

inline dim3 cell_grid(int64_t max_cells, int n) {
    return dim3((unsigned)std::min<int64_t>((max_cells + 255) / 256, 256), (unsigned)std::min(n, 65535));
}

// host table of shapes -> total and largest cell count; false when a shape is refused
inline bool scan_shapes(const int* hw, int n, int64_t* total, int64_t* largest) {
    *total = 0; *largest = 0;
    for (int o = 0; o < n; ++o) {
        if (!side_ok(hw[2 * o], hw[2 * o + 1])) return false;
        const int64_t c = cells_of(hw[2 * o], hw[2 * o + 1]);
        *total += c;
        *largest = std::max(*largest, c);
    }
    return true;
}

}  // namespace

extern "C" {

int64_t seam_rle_encode_ws_bytes(int h, int w) {
    return side_ok(h, w) ? cells_of(h, w) * 4 : 0;
}

int seam_rle_encode_masks_u8(const uint8_t* masks, int64_t mask_bytes, const int* obj_hw_host, const int* obj_hw,
                             const int64_t* obj_off, const int64_t* obj_cell_off, void* ws, int64_t ws_bytes, int* counts, int n,
                             void* stream) {
    if (n < 0 || mask_bytes < 0 || ws_bytes < 0 || (ws_bytes & 3)) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    if (!masks || !obj_hw_host || !obj_hw || !obj_off || !obj_cell_off || !ws || !counts) return (int)hipErrorInvalidValue;
    int64_t total, largest;
    if (!scan_shapes(obj_hw_host, n, &total, &largest) || total * 4 > ws_bytes) return (int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    hipError_t rc = hipMemsetAsync(ws, 0, (size_t)ws_bytes, s);
    if (rc == hipSuccess) rc = hipMemsetAsync(counts, 0, (size_t)ws_bytes, s);
    if (rc != hipSuccess) return (int)rc;
    const Objs t{obj_hw, obj_cell_off, 0, 0};
    const int64_t ws_words = ws_bytes >> 2;
    hipLaunchKernelGGL(rle_values_u8_kernel, cell_grid(largest, n), dim3(256), 0, s, masks, mask_bytes, obj_off, t, (uint32_t*)ws,
                       ws_words, n);
    hipLaunchKernelGGL(rle_count_kernel, cell_grid(largest, n), dim3(256), 0, s, t, (const uint32_t*)ws, ws_words, counts, n);
    return (int)hipGetLastError();
}

int seam_rle_encode_paste_f32(const float* probs, const float* boxes, int D, int H, int W, void* ws, int64_t ws_bytes,
                              int* counts, void* stream) {
    if (D < 0 || ws_bytes < 0 || (ws_bytes & 3)) return (int)hipErrorInvalidValue;
    if (D == 0) return 0;
    if (!probs || !boxes || !ws || !counts || !side_ok(H, W) || ((uintptr_t)boxes & 15)) return (int)hipErrorInvalidValue;
    const int64_t cells = cells_of(H, W);
    if (cells * D * 4 > ws_bytes) return (int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    hipError_t rc = hipMemsetAsync(ws, 0, (size_t)ws_bytes, s);
    if (rc == hipSuccess) rc = hipMemsetAsync(counts, 0, (size_t)ws_bytes, s);
    if (rc != hipSuccess) return (int)rc;
    const Objs t{nullptr, nullptr, H, W};
    const int64_t ws_words = ws_bytes >> 2;
    hipLaunchKernelGGL(rle_values_paste_kernel, cell_grid(cells, D), dim3(256), 0, s, probs, boxes, D, H, W, (uint32_t*)ws,
                       ws_words);
    hipLaunchKernelGGL(rle_count_kernel, cell_grid(cells, D), dim3(256), 0, s, t, (const uint32_t*)ws, ws_words, counts, D);
    return (int)hipGetLastError();
}

int seam_rle_positions_masks(const int* obj_hw_host, const int* obj_hw, const int64_t* obj_cell_off, const void* ws,
                             int64_t ws_bytes, const int64_t* scan, int* positions, int64_t capacity, int n, void* stream) {
    if (n < 0 || ws_bytes < 0 || (ws_bytes & 3) || capacity < 0) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    if (!obj_hw_host || !obj_hw || !obj_cell_off || !ws || !scan || (capacity > 0 && !positions)) return (int)hipErrorInvalidValue;
    int64_t total, largest;
    if (!scan_shapes(obj_hw_host, n, &total, &largest) || total * 4 > ws_bytes) return (int)hipErrorInvalidValue;
    if (capacity == 0) return 0;
    const Objs t{obj_hw, obj_cell_off, 0, 0};
    hipLaunchKernelGGL(rle_positions_kernel, cell_grid(largest, n), dim3(256), 0, (hipStream_t)stream, t, (const uint32_t*)ws,
                       ws_bytes >> 2, scan, positions, capacity, n);
    return (int)hipGetLastError();
}

int seam_rle_positions_paste(int D, int H, int W, const void* ws, int64_t ws_bytes, const int64_t* scan, int* positions,
                             int64_t capacity, void* stream) {
    if (D < 0 || ws_bytes < 0 || (ws_bytes & 3) || capacity < 0) return (int)hipErrorInvalidValue;
    if (D == 0) return 0;
    if (!ws || !scan || (capacity > 0 && !positions) || !side_ok(H, W)) return (int)hipErrorInvalidValue;
    const int64_t cells = cells_of(H, W);
    if (cells * D * 4 > ws_bytes) return (int)hipErrorInvalidValue;
    if (capacity == 0) return 0;
    const Objs t{nullptr, nullptr, H, W};
    hipLaunchKernelGGL(rle_positions_kernel, cell_grid(cells, D), dim3(256), 0, (hipStream_t)stream, t, (const uint32_t*)ws,
                       ws_bytes >> 2, scan, positions, capacity, D);
    return (int)hipGetLastError();
}

}  // extern "C"
