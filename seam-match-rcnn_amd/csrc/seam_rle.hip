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

// ---- the bitmap as the common form of every RLE operation: runs -> bits, bits (op) bits, popcount(bits & bits) ----------------
// last i in [lo, hi) with tab[i] <= key (lo when none is), as seam_masks.hip's
__device__ __forceinline__ int last_run_le(const int* __restrict__ tab, int lo, int hi, int key) {
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (tab[mid] <= key) lo = mid; else hi = mid;
    }
    return lo;
}

// One thread per (band, column) word: binary search for the run that holds the word's first position p = c*h + 32*band, then a
// walk over the runs that start inside its rows.  A zero-length run repeats a start and sets nothing.
__global__ __launch_bounds__(256) void rle_values_runs_kernel(const int* __restrict__ run_start, const int* __restrict__ obj_run_off,
                                                              Objs t, uint32_t* __restrict__ ws, int64_t ws_words, int n_runs,
                                                              int n) {
    for (int o = blockIdx.y; o < n; o += gridDim.y) {
        const Obj b = obj_get(t, o, ws_words);
        if (!b.ok) continue;
        const int r0 = max(obj_run_off[o], 0), r1 = min(obj_run_off[o + 1], n_runs);     // never read outside the run table
        const int cells = b.bands * b.w;
        for (int i = blockIdx.x * 256 + threadIdx.x; i < cells; i += gridDim.x * 256) {
            const int k = i / b.w, c = i - k * b.w;
            const int nr = min(32, b.h - (k << 5));
            const int p = c * b.h + (k << 5), end = p + nr;            // < 2^31: h*w is
            uint32_t v = 0;
            if (r1 > r0) {
                int j = last_run_le(run_start, r0, r1, p), pos = p;
                while (pos < end) {
                    const int e = j + 1 < r1 ? min(max(run_start[j + 1], pos), end) : end;
                    if ((j - r0) & 1) {
                        const uint32_t upto = e - p == 32 ? ~0u : (1u << (e - p)) - 1u;
                        v |= upto & ~((1u << (pos - p)) - 1u);
                    }
                    pos = e;
                    ++j;
                }
            }
            ws[b.base + i] = v;
        }
    }
}

// dst object g <- OR (AND with `intersect`) over the source objects group_obj[group_off[g] .. group_off[g+1]); a source that is
// not a valid object of g's shape is left out, a group without a valid source gives zeros.
__global__ __launch_bounds__(256) void rle_bits_combine_kernel(const int* __restrict__ group_off, const int* __restrict__ group_obj,
                                                               int n_entries, Objs st, const uint32_t* __restrict__ src,
                                                               int64_t src_words, int n_src, Objs dt, uint32_t* __restrict__ dst,
                                                               int64_t dst_words, int n_dst, int intersect) {
    for (int g = blockIdx.y; g < n_dst; g += gridDim.y) {
        const Obj b = obj_get(dt, g, dst_words);
        if (!b.ok) continue;
        const int e0 = max(group_off[g], 0), e1 = min(group_off[g + 1], n_entries);
        const int cells = b.bands * b.w;
        for (int i = blockIdx.x * 256 + threadIdx.x; i < cells; i += gridDim.x * 256) {
            uint32_t acc = 0;
            bool any = false;
            for (int e = e0; e < e1; ++e) {
                const int s = group_obj[e];
                if (s < 0 || s >= n_src) continue;
                const Obj a = obj_get(st, s, src_words);
                if (!a.ok || a.h != b.h || a.w != b.w) continue;
                const uint32_t v = src[a.base + i];
                acc = !any ? v : (intersect ? acc & v : acc | v);
                any = true;
            }
            const int nr = b.h - ((i / b.w) << 5);
            if (nr < 32) acc &= (1u << nr) - 1u;                      // rows past h stay zero whatever the sources hold
            dst[b.base + i] = acc;
        }
    }
}

// One block per pair (a, b): out[p] = sum over the cells of popcount(a & b), rows past h masked off; pairs == NULL: pair p is
// (p, p), the object's own popcount.  A pair that names no two valid objects of one shape gives -1.  Integer sums: the lanes'
// partial sums meet in a fixed tree, and any order gives the same number.
__global__ __launch_bounds__(256) void rle_bits_inter_kernel(const int* __restrict__ pairs, Objs t, const uint32_t* __restrict__ ws,
                                                             int64_t ws_words, int n, int64_t* __restrict__ out, int P) {
    __shared__ int part[4];
    for (int p = blockIdx.x; p < P; p += gridDim.x) {
        const int ia = pairs ? pairs[2 * p] : p, ib = pairs ? pairs[2 * p + 1] : p;
        bool ok = ia >= 0 && ia < n && ib >= 0 && ib < n;              // block-uniform
        Obj a{}, b{};
        if (ok) {
            a = obj_get(t, ia, ws_words);
            b = obj_get(t, ib, ws_words);
            ok = a.ok && b.ok && a.h == b.h && a.w == b.w;
        }
        if (!ok) {
            if (threadIdx.x == 0) out[p] = -1;
            continue;
        }
        const int cells = a.bands * a.w, full = (a.h & 31) ? (a.bands - 1) * a.w : cells;
        const uint32_t tail = (1u << (a.h & 31)) - 1u;
        const uint32_t* __restrict__ wa = ws + a.base;
        const uint32_t* __restrict__ wb = ws + b.base;
        int sum = 0;                                                   // <= h*w < 2^31
        for (int i = threadIdx.x; i < cells; i += 256) {
            const uint32_t v = wa[i] & wb[i];
            sum += __popc(i < full ? v : v & tail);
        }
        for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d, 64);
        __syncthreads();                                              // the previous pair's reader is done with part
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sum;
        __syncthreads();
        if (threadIdx.x == 0) out[p] = (int64_t)part[0] + part[1] + part[2] + part[3];
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

inline int bits_inter_launch(const int* pairs, int P, const int* obj_hw_host, const int* obj_hw, const int64_t* obj_cell_off,
                      const void* ws, int64_t ws_bytes, int n, int64_t* out, void* stream) {
    int64_t total, largest;
    if (!scan_shapes(obj_hw_host, n, &total, &largest) || total * 4 > ws_bytes) return (int)hipErrorInvalidValue;
    const Objs t{obj_hw, obj_cell_off, 0, 0};
    hipLaunchKernelGGL(rle_bits_inter_kernel, dim3((unsigned)std::min(P, 65535)), dim3(256), 0, (hipStream_t)stream, pairs, t,
                       (const uint32_t*)ws, ws_bytes >> 2, n, out, P);
    return (int)hipGetLastError();
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

int seam_rle_bits_from_runs(const int* run_start, const int* obj_run_off, int n_runs, const int* obj_hw_host, const int* obj_hw,
                            const int64_t* obj_cell_off, void* ws, int64_t ws_bytes, int n, void* stream) {
    if (n < 0 || n_runs < 0 || ws_bytes < 0 || (ws_bytes & 3)) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    if (!run_start || !obj_run_off || !obj_hw_host || !obj_hw || !obj_cell_off || !ws) return (int)hipErrorInvalidValue;
    int64_t total, largest;
    if (!scan_shapes(obj_hw_host, n, &total, &largest) || total * 4 > ws_bytes) return (int)hipErrorInvalidValue;
    const Objs t{obj_hw, obj_cell_off, 0, 0};
    hipLaunchKernelGGL(rle_values_runs_kernel, cell_grid(largest, n), dim3(256), 0, (hipStream_t)stream, run_start, obj_run_off, t,
                       (uint32_t*)ws, ws_bytes >> 2, n_runs, n);
    return (int)hipGetLastError();
}

int seam_rle_bits_combine(const int* group_off, const int* group_obj, int n_entries, const int* src_hw, const int64_t* src_cell_off,
                          const void* src, int64_t src_bytes, int n_src, const int* dst_hw_host, const int* dst_hw,
                          const int64_t* dst_cell_off, void* dst, int64_t dst_bytes, int n_dst, int intersect, void* stream) {
    if (n_dst < 0 || n_src < 0 || n_entries < 0 || src_bytes < 0 || dst_bytes < 0 || ((src_bytes | dst_bytes) & 3))
        return (int)hipErrorInvalidValue;
    if (n_dst == 0) return 0;
    if (!group_off || !dst_hw_host || !dst_hw || !dst_cell_off || !dst) return (int)hipErrorInvalidValue;
    if (n_entries > 0 && (!group_obj || !src_hw || !src_cell_off || !src || n_src == 0)) return (int)hipErrorInvalidValue;
    int64_t total, largest;
    if (!scan_shapes(dst_hw_host, n_dst, &total, &largest) || total * 4 > dst_bytes) return (int)hipErrorInvalidValue;
    const Objs st{src_hw, src_cell_off, 0, 0}, dt{dst_hw, dst_cell_off, 0, 0};
    hipLaunchKernelGGL(rle_bits_combine_kernel, cell_grid(largest, n_dst), dim3(256), 0, (hipStream_t)stream, group_off, group_obj,
                       n_entries, st, (const uint32_t*)src, src_bytes >> 2, n_src, dt, (uint32_t*)dst, dst_bytes >> 2, n_dst,
                       intersect);
    return (int)hipGetLastError();
}

int seam_rle_count_bits(const int* obj_hw_host, const int* obj_hw, const int64_t* obj_cell_off, const void* ws, int64_t ws_bytes,
                        int* counts, int n, void* stream) {
    if (n < 0 || ws_bytes < 0 || (ws_bytes & 3)) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    if (!obj_hw_host || !obj_hw || !obj_cell_off || !ws || !counts) return (int)hipErrorInvalidValue;
    int64_t total, largest;
    if (!scan_shapes(obj_hw_host, n, &total, &largest) || total * 4 > ws_bytes) return (int)hipErrorInvalidValue;
    const Objs t{obj_hw, obj_cell_off, 0, 0};
    hipLaunchKernelGGL(rle_count_kernel, cell_grid(largest, n), dim3(256), 0, (hipStream_t)stream, t, (const uint32_t*)ws,
                       ws_bytes >> 2, counts, n);
    return (int)hipGetLastError();
}

int seam_rle_bits_inter(const int* pairs, int P, const int* obj_hw_host, const int* obj_hw, const int64_t* obj_cell_off,
                        const void* ws, int64_t ws_bytes, int n, int64_t* inter, void* stream) {
    if (P < 0 || n < 0 || ws_bytes < 0 || (ws_bytes & 3)) return (int)hipErrorInvalidValue;
    if (P == 0) return 0;
    if (n == 0 || !pairs || !obj_hw_host || !obj_hw || !obj_cell_off || !ws || !inter) return (int)hipErrorInvalidValue;
    return bits_inter_launch(pairs, P, obj_hw_host, obj_hw, obj_cell_off, ws, ws_bytes, n, inter, stream);
}

int seam_rle_bits_area(const int* obj_hw_host, const int* obj_hw, const int64_t* obj_cell_off, const void* ws, int64_t ws_bytes,
                       int n, int64_t* area, void* stream) {
    if (n < 0 || ws_bytes < 0 || (ws_bytes & 3)) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    if (!obj_hw_host || !obj_hw || !obj_cell_off || !ws || !area) return (int)hipErrorInvalidValue;
    return bits_inter_launch(nullptr, n, obj_hw_host, obj_hw, obj_cell_off, ws, ws_bytes, n, area, stream);
}

}  // extern "C"
