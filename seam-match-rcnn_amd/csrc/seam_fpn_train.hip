// seam_fpn_train.hip -- the adjoints the FPN needs to learn from the heads' losses (gfx950, fp32, NHWC):
//
//   seam_roi_align_bwd_f32        adjoint of seam_roi_align_f32 (MultiScaleRoIAlign, roi_align(aligned=False))
//   seam_rpn_scatter_patches_f32  adjoint of seam_rpn_gather_patches_f32 (the RPN conv's 3x3 windows at the sampled pixels)
//   seam_upsample_add_bwd_f32     adjoint of the nearest top-down merge (seam_upsample_add_f32 / seam_conv2d_upres_f32)
//   seam_subsample_add_bwd_f32    adjoint of LastLevelMaxPool (max_pool2d k=1, s=2), added in place
//
// No float atomics anywhere: every output element is summed by ONE thread in a fixed order (gather form), so a launch is
// bit-identical to the next, and every kernel writes its whole output (zeros where nothing arrives).
//
// RoIAlign adjoint.  The bilinear weight of a sample is a product of a row factor and a column factor, and so are the clamps
// and the validity test, so for one ROI
//     dX[y,x,:] = sum_ph sum_pw Wy[y,ph] * Wx[x,pw] * dout[ph,pw,:] / sr^2
// with Wy[y,ph] = the summed row weights of bin row ph's samples on feature row y.  Three launches:
//   prepare  one thread per ROI: image, level (the forward's LevelMapper, seam_fpn_common.h), scaled origin and bin size, and a
//            conservative pixel bounding box; a ROI that can reach nothing (bad image index, every sample outside) gets key -1
//   lists    one workgroup per (image, level): the ROIs of that bucket in ascending ROI index (ordered ballot compaction)
//   tiles    one workgroup per 8x8-pixel tile of one image and level and per 256-channel chunk: it walks the bucket's list in
//            order, rejects a ROI by its bounding box with wave-uniform work, builds the two <= 8 x P weight tables in LDS,
//            and accumulates in registers (a wave owns 16 pixels; the 64 lanes are the channels, 16 bytes each); one store.
// A tile only ever writes its own pixels, so no ROI -- whatever its coordinates -- can cause an access outside the maps.
//
// The sample positions are formed WITHOUT fused multiply-adds (torchvision's own operation sequence, and the oracle's); the
// forward kernel lets the compiler fuse `y1 + ph * bh`, which can move a position by an ulp.  The level is the forward's.
#include <hip/hip_runtime.h>
#include "seam_device.h"
#include <stdint.h>
#include "seam_fpn_common.h"

namespace {

constexpr int RB_TILE = 8;          // tile side, feature pixels
constexpr int RB_PMAX = 32;         // largest pooled size
constexpr int RB_CCHUNK = 256;      // channels per workgroup: 64 lanes x 4
constexpr int RB_PIX = RB_TILE * RB_TILE / 4;   // pixels per wave

struct RoiBwdArgs {
    float* dmap[4];
    int h[4], w[4];
    float scale[4];
    int tile0[5];                   // first tile of each level in the grid; [4] = total
    int tw[4], tpi[4];              // tiles per tile row / per image
    int C, k_min, N, K, P, sr;
    const float* rois;
    const int* levels;
    const float* dout;
    int* key;                       // [K] image * 4 + level, -1: contributes nothing
    float4* geo;                    // [K] (x1, y1, bin w, bin h) on the level's grid
    int4* box;                      // [K] (xlo, xhi, ylo, yhi) pixels the ROI may touch (conservative)
    int* list;                      // [K] ROI indices grouped by bucket, ascending inside a bucket
    int2* bucket;                   // [N*4] (offset into list, count)
};

// position of sample i of bin p along one axis: torchvision's sequence of fp32 operations, none fused
__device__ __forceinline__ float sample_pos(float start, float bin, int p, int i, int sr) {
#pragma clang fp contract(off)
    const float a = start + (float)p * bin;
    const float b = ((float)i + 0.5f) * bin / (float)sr;
    return a + b;
}

__global__ __launch_bounds__(256) void roi_bwd_prepare_kernel(const RoiBwdArgs a) {
#pragma clang fp contract(off)
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= a.K) return;
    const float* r = a.rois + (size_t)k * 5;
    const float b = r[0];
    const float bx1 = r[1], by1 = r[2], bx2 = r[3], by2 = r[4];
    bool ok = b >= 0.f && b < (float)a.N;                        // false for NaN
    const int img = ok ? (int)b : 0;
    const int lvl = a.levels ? a.levels[k] : seam_fpn::map_level(bx1, by1, bx2, by2, a.k_min);
    ok = ok && lvl >= 0 && lvl < 4;
    const int H = lvl == 0 ? a.h[0] : lvl == 1 ? a.h[1] : lvl == 2 ? a.h[2] : a.h[3];
    const int W = lvl == 0 ? a.w[0] : lvl == 1 ? a.w[1] : lvl == 2 ? a.w[2] : a.w[3];
    const float sc = lvl == 0 ? a.scale[0] : lvl == 1 ? a.scale[1] : lvl == 2 ? a.scale[2] : a.scale[3];
    const float x1 = bx1 * sc, y1 = by1 * sc, x2 = bx2 * sc, y2 = by2 * sc;
    const float rw = fmaxf(x2 - x1, 1.f), rh = fmaxf(y2 - y1, 1.f);
    const float bw = rw / (float)a.P, bh = rh / (float)a.P;
    // first and last sample of each axis; valid samples lie in [-1, size] and touch floor(max(pos, 0)) and the pixel after it
    const float xf = sample_pos(x1, bw, 0, 0, a.sr), xl = sample_pos(x1, bw, a.P - 1, a.sr - 1, a.sr);
    const float yf = sample_pos(y1, bh, 0, 0, a.sr), yl = sample_pos(y1, bh, a.P - 1, a.sr - 1, a.sr);
    ok = ok && xf <= (float)W + 1.f && xl >= -2.f && yf <= (float)H + 1.f && yl >= -2.f;      // false for NaN
    int4 box = make_int4(1, 0, 1, 0);
    if (ok) {
        box.x = max((int)fminf(fmaxf(xf, 0.f), (float)W) - 1, 0);
        box.y = min((int)fminf(fmaxf(xl, 0.f), (float)W) + 2, W - 1);
        box.z = max((int)fminf(fmaxf(yf, 0.f), (float)H) - 1, 0);
        box.w = min((int)fminf(fmaxf(yl, 0.f), (float)H) + 2, H - 1);
    }
    a.key[k] = ok ? img * 4 + lvl : -1;
    a.geo[k] = make_float4(x1, y1, bw, bh);
    a.box[k] = box;
}

__global__ __launch_bounds__(256) void roi_bwd_lists_kernel(const RoiBwdArgs a) {
    __shared__ int s_cnt[2][4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int less = 0, eq = 0;
    for (int k = tid; k < a.K; k += 256) {
        const int key = a.key[k];
        less += (key >= 0 && key < b) ? 1 : 0;
        eq += key == b ? 1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) {
        less += __shfl_xor(less, o, 64);
        eq += __shfl_xor(eq, o, 64);
    }
    if (lane == 0) { s_cnt[0][wave] = less; s_cnt[1][wave] = eq; }
    __syncthreads();
    const int off = s_cnt[0][0] + s_cnt[0][1] + s_cnt[0][2] + s_cnt[0][3];
    const int cnt = s_cnt[1][0] + s_cnt[1][1] + s_cnt[1][2] + s_cnt[1][3];
    __syncthreads();
    if (tid == 0) a.bucket[b] = make_int2(off, cnt);
    int base = 0;
    for (int k0 = 0; k0 < a.K; k0 += 256) {                     // ordered compaction, 256 ROIs per step
        const int k = k0 + tid;
        const bool mine = k < a.K && a.key[k] == b;
        const unsigned long long m = __ballot(mine);
        if (lane == 0) s_cnt[0][wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < 4; ++w) {
            before += w < wave ? s_cnt[0][w] : 0;
            total += s_cnt[0][w];
        }
        if (mine) a.list[off + base + before + __popcll(m & ((1ull << lane) - 1ull))] = k;
        base += total;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void roi_bwd_tile_kernel(const RoiBwdArgs a) {
    __shared__ float s_tab[2][RB_TILE][RB_PMAX];                // [0]: Wy[row][ph], [1]: Wx[col][pw]
    __shared__ int s_rng[2][RB_TILE][2];                        // bins with a non-zero weight: [lo, hi)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x;
    const int lvl = tile < a.tile0[1] ? 0 : tile < a.tile0[2] ? 1 : tile < a.tile0[3] ? 2 : 3;
    const int H = lvl == 0 ? a.h[0] : lvl == 1 ? a.h[1] : lvl == 2 ? a.h[2] : a.h[3];
    const int W = lvl == 0 ? a.w[0] : lvl == 1 ? a.w[1] : lvl == 2 ? a.w[2] : a.w[3];
    const int t0 = lvl == 0 ? a.tile0[0] : lvl == 1 ? a.tile0[1] : lvl == 2 ? a.tile0[2] : a.tile0[3];
    const int tw = lvl == 0 ? a.tw[0] : lvl == 1 ? a.tw[1] : lvl == 2 ? a.tw[2] : a.tw[3];
    const int tpi = lvl == 0 ? a.tpi[0] : lvl == 1 ? a.tpi[1] : lvl == 2 ? a.tpi[2] : a.tpi[3];
    float* dmap = lvl == 0 ? a.dmap[0] : lvl == 1 ? a.dmap[1] : lvl == 2 ? a.dmap[2] : a.dmap[3];
    const int t = tile - t0;
    const int img = t / tpi, tt = t - img * tpi;
    const int ty0 = (tt / tw) * RB_TILE, tx0 = (tt % tw) * RB_TILE;
    const int c0 = blockIdx.y * RB_CCHUNK + lane * 4;
    const bool cact = c0 < a.C;
    const int P = a.P, sr = a.sr;
    const int2 bk = a.K > 0 ? a.bucket[img * 4 + lvl] : make_int2(0, 0);

    f32x4 acc[RB_PIX];
#pragma unroll
    for (int i = 0; i < RB_PIX; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int j = 0; j < bk.y; ++j) {
        const int k = a.list[bk.x + j];                          // block-uniform
        const int4 box = a.box[k];
        if (box.x > tx0 + RB_TILE - 1 || box.y < tx0 || box.z > ty0 + RB_TILE - 1 || box.w < ty0) continue;
        const float4 geo = a.geo[k];
        __syncthreads();                                         // the previous ROI's table reads are done
        for (int e = tid; e < 2 * RB_TILE * P; e += 256) {
            const int axis = e / (RB_TILE * P), rem = e - axis * RB_TILE * P;
            const int row = rem / P, p = rem - row * P;
            const int pix = (axis ? tx0 : ty0) + row, size = axis ? W : H;
            const float start = axis ? geo.x : geo.y, bin = axis ? geo.z : geo.w;
            float ws = 0.f;
            for (int i = 0; i < sr; ++i) {
                float pos = sample_pos(start, bin, p, i, sr);
                if (!(pos >= -1.f && pos <= (float)size)) continue;      // outside (or NaN): the sample contributes nothing
                pos = fmaxf(pos, 0.f);
                int lo = (int)pos, hi;
                if (lo >= size - 1) { lo = hi = size - 1; pos = (float)lo; } else { hi = lo + 1; }
                const float l = pos - (float)lo, hw = 1.f - l;
                if (lo == pix) ws += hw;
                if (hi == pix) ws += l;
            }
            s_tab[axis][row][p] = ws;
        }
        __syncthreads();
        if (tid < 2 * RB_TILE) {
            const int axis = tid >> 3, row = tid & 7;
            int lo = P, hi = 0;
            for (int p = 0; p < P; ++p)
                if (s_tab[axis][row][p] != 0.f) { lo = min(lo, p); hi = p + 1; }
            s_rng[axis][row][0] = lo;
            s_rng[axis][row][1] = hi;
        }
        __syncthreads();
        const float* g = a.dout + (size_t)k * P * P * a.C + (cact ? c0 : 0);
#pragma unroll
        for (int i = 0; i < RB_PIX; ++i) {
            const int py = wave * (RB_TILE / 4) + i / RB_TILE, px = i % RB_TILE;
            const int ylo = s_rng[0][py][0], yhi = s_rng[0][py][1], xlo = s_rng[1][px][0], xhi = s_rng[1][px][1];
            for (int ph = ylo; ph < yhi; ++ph) {
                const float wy = s_tab[0][py][ph];
                for (int pw = xlo; pw < xhi; ++pw) {
                    const float w = wy * s_tab[1][px][pw];
                    if (cact) {
                        const f32x4 v = *reinterpret_cast<const f32x4*>(g + (size_t)(ph * P + pw) * a.C);
                        acc[i] = __builtin_elementwise_fma((f32x4){w, w, w, w}, v, acc[i]);
                    }
                }
            }
        }
    }
    if (!cact) return;
    const float cnt = (float)(sr * sr);
#pragma unroll
    for (int i = 0; i < RB_PIX; ++i) {
        const int y = ty0 + wave * (RB_TILE / 4) + i / RB_TILE, x = tx0 + i % RB_TILE;
        if (y < H && x < W)
            *reinterpret_cast<f32x4*>(dmap + ((size_t)((size_t)img * H + y) * W + x) * a.C + c0) = acc[i] / cnt;
    }
}

// ---------------------------------------------------------------------------------------------------- window scatter
constexpr int SC_MAX_LEVELS = 8;
constexpr int SC_Q = 16;            // float4 channel groups per workgroup (64 channels)

struct ScatterArgs {
    float* maps[SC_MAX_LEVELS];
    int H[SC_MAX_LEVELS], W[SC_MAX_LEVELS];
    const int* rows;
    const float* dpatch;
    int M, N, L, C;
};

// one workgroup per (image, level, 64-channel chunk): the rows of that image and level in row order, a barrier between two
// rows (windows overlap, and slots of one pixel are separate rows); the nine taps of one row never collide
__global__ __launch_bounds__(256) void rpn_scatter_kernel(const ScatterArgs a) {
    const int img = blockIdx.x / a.L, lvl = blockIdx.x - img * a.L;
    int H = 0, W = 0;
    float4* map = nullptr;
    for (int l = 0; l < SC_MAX_LEVELS; ++l)
        if (l == lvl) { H = a.H[l]; W = a.W[l]; map = reinterpret_cast<float4*>(a.maps[l]); }
    const int c4 = a.C >> 2, q0 = blockIdx.y * SC_Q;
    const int tap = threadIdx.x / SC_Q, q = q0 + (threadIdx.x % SC_Q);
    const bool active = tap < 9 && q < c4;
    const float4* dp = reinterpret_cast<const float4*>(a.dpatch);
    for (int r = 0; r < a.M; ++r) {
        const int4 row = reinterpret_cast<const int4*>(a.rows)[r];           // block-uniform
        if (row.x != img || row.y != lvl) continue;
        const int y = row.z, x = row.w;
        if (y < 0 || y >= H || x < 0 || x >= W) continue;
        if (active) {
            const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
            if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
                float4* p = map + (((size_t)img * H + yy) * W + xx) * c4 + q;
                const float4 g = dp[((size_t)r * 9 + tap) * c4 + q];
                float4 v = *p;
                v.x += g.x; v.y += g.y; v.z += g.z; v.w += g.w;
                *p = v;
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------- top-down merge
__global__ __launch_bounds__(256) void upsample_add_bwd_kernel(const float* __restrict__ dlat, const float* base,
                                                              float* dtop, int N, int H, int W, int Ht, int Wt, int C) {
    const int c4 = C >> 2;
    const size_t total = (size_t)N * Ht * Wt * c4;
    const float sh = (float)Ht / (float)H, sw = (float)Wt / (float)W;       // the forward's scales
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int q = (int)(i % c4);
        size_t r = i / c4;
        const int wt = (int)(r % Wt);
        r /= Wt;
        const int ht = (int)(r % Ht);
        const int n = (int)(r / Ht);
        // first fine row / column the forward maps to (ht, wt): the map is non-decreasing, so walk from a guess below it
        int h0 = max(min((int)((float)ht / sh) - 2, H - 1), 0), w0 = max(min((int)((float)wt / sw) - 2, W - 1), 0);
        while (h0 > 0 && seam_fpn::nearest_src(h0 - 1, sh, Ht) >= ht) --h0;
        while (h0 < H && seam_fpn::nearest_src(h0, sh, Ht) < ht) ++h0;
        while (w0 > 0 && seam_fpn::nearest_src(w0 - 1, sw, Wt) >= wt) --w0;
        while (w0 < W && seam_fpn::nearest_src(w0, sw, Wt) < wt) ++w0;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int h = h0; h < H && seam_fpn::nearest_src(h, sh, Ht) == ht; ++h)
            for (int w = w0; w < W && seam_fpn::nearest_src(w, sw, Wt) == wt; ++w) {
                const float4 v = reinterpret_cast<const float4*>(dlat)[(((size_t)n * H + h) * W + w) * c4 + q];
                acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
            }
        if (base) {
            const float4 b = reinterpret_cast<const float4*>(base)[i];
            acc.x += b.x; acc.y += b.y; acc.z += b.z; acc.w += b.w;
        }
        reinterpret_cast<float4*>(dtop)[i] = acc;
    }
}

__global__ __launch_bounds__(256) void subsample_add_bwd_kernel(float* d, const float* __restrict__ dpool, int N, int H, int W,
                                                               int Hp, int Wp, int C) {
    const int c4 = C >> 2;
    const size_t total = (size_t)N * Hp * Wp * c4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int q = (int)(i % c4);
        size_t r = i / c4;
        const int wp = (int)(r % Wp);
        r /= Wp;
        const int hp = (int)(r % Hp);
        const int n = (int)(r / Hp);
        float4* p = reinterpret_cast<float4*>(d) + (((size_t)n * H + 2 * hp) * W + 2 * wp) * c4 + q;
        const float4 g = reinterpret_cast<const float4*>(dpool)[i];
        float4 v = *p;
        v.x += g.x; v.y += g.y; v.z += g.z; v.w += g.w;
        *p = v;
    }
}

inline int64_t align16(int64_t v) { return (v + 15) / 16 * 16; }
inline unsigned grid_for(size_t total) { return (unsigned)((total + 255) / 256 > 65535 * 16 ? 65535 * 16 : (total + 255) / 256); }

constexpr int RB_MAX_ROIS = 1 << 20;
constexpr int RB_MAX_IMAGES = 4096;

}  // namespace

extern "C" {

int64_t seam_roi_align_bwd_workspace_bytes(int N, int K) {
    if (N <= 0 || N > RB_MAX_IMAGES || K < 0 || K > RB_MAX_ROIS) return 0;
    const int64_t k = K > 0 ? K : 1;
    return align16(k * 4) + k * 16 + k * 16 + align16(k * 4) + (int64_t)N * 4 * 8;
}

int seam_roi_align_bwd_f32(const float* dout, const float* rois, const int* levels, const int* hw, int C, float scale0,
                           float scale1, float scale2, float scale3, int k_min, int N, int K, int P, int sampling_ratio,
                           float* dfeat0, float* dfeat1, float* dfeat2, float* dfeat3, void* ws, void* stream) {
    if (C <= 0 || (C & 3) || C > 4096 || P < 1 || P > RB_PMAX || sampling_ratio <= 0 || sampling_ratio > 64 || N <= 0 ||
        N > RB_MAX_IMAGES || K < 0 || K > RB_MAX_ROIS || !hw || !dfeat0 || !dfeat1 || !dfeat2 || !dfeat3 || !ws ||
        (K > 0 && (!dout || !rois)))
        return (int)hipErrorInvalidValue;
    RoiBwdArgs a;
    a.dmap[0] = dfeat0; a.dmap[1] = dfeat1; a.dmap[2] = dfeat2; a.dmap[3] = dfeat3;
    a.scale[0] = scale0; a.scale[1] = scale1; a.scale[2] = scale2; a.scale[3] = scale3;
    int64_t tiles = 0;
    for (int l = 0; l < 4; ++l) {
        const int h = hw[2 * l], w = hw[2 * l + 1];
        if (h <= 0 || w <= 0 || (int64_t)N * h * w * C * 4 >= ((int64_t)1 << 31)) return (int)hipErrorInvalidValue;
        a.h[l] = h; a.w[l] = w;
        a.tw[l] = (w + RB_TILE - 1) / RB_TILE;
        a.tpi[l] = a.tw[l] * ((h + RB_TILE - 1) / RB_TILE);
        a.tile0[l] = (int)tiles;
        tiles += (int64_t)N * a.tpi[l];
    }
    if (tiles >= ((int64_t)1 << 31)) return (int)hipErrorInvalidValue;
    a.tile0[4] = (int)tiles;
    a.C = C; a.k_min = k_min; a.N = N; a.K = K; a.P = P; a.sr = sampling_ratio;
    a.rois = rois; a.levels = levels; a.dout = dout;
    char* w = static_cast<char*>(ws);
    const int64_t k = K > 0 ? K : 1;
    a.key = reinterpret_cast<int*>(w);      w += align16(k * 4);
    a.geo = reinterpret_cast<float4*>(w);   w += k * 16;
    a.box = reinterpret_cast<int4*>(w);     w += k * 16;
    a.list = reinterpret_cast<int*>(w);     w += align16(k * 4);
    a.bucket = reinterpret_cast<int2*>(w);
    hipStream_t s = (hipStream_t)stream;
    if (K > 0) {
        hipLaunchKernelGGL(roi_bwd_prepare_kernel, dim3((K + 255) / 256), dim3(256), 0, s, a);
        hipLaunchKernelGGL(roi_bwd_lists_kernel, dim3(N * 4), dim3(256), 0, s, a);
    }
    hipLaunchKernelGGL(roi_bwd_tile_kernel, dim3((unsigned)tiles, (C + RB_CCHUNK - 1) / RB_CCHUNK), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

int seam_rpn_scatter_patches_f32(const float* dpatch, const int* rows, int M, int N, int L, int C, void* const* dmaps,
                                 const int* hw, void* stream) {
    if (M <= 0 || M > (1 << 20) || N <= 0 || N > RB_MAX_IMAGES || L <= 0 || L > SC_MAX_LEVELS || C <= 0 || C > 4096 ||
        (C & 3) || !dmaps || !hw || !rows || !dpatch)
        return (int)hipErrorInvalidValue;
    ScatterArgs a{};
    for (int l = 0; l < L; ++l) {
        if (!dmaps[l] || hw[2 * l] <= 0 || hw[2 * l + 1] <= 0) return (int)hipErrorInvalidValue;
        a.maps[l] = static_cast<float*>(dmaps[l]);
        a.H[l] = hw[2 * l];
        a.W[l] = hw[2 * l + 1];
    }
    a.rows = rows; a.dpatch = dpatch; a.M = M; a.N = N; a.L = L; a.C = C;
    hipStream_t s = (hipStream_t)stream;
    for (int l = 0; l < L; ++l) {
        const hipError_t e = hipMemsetAsync(a.maps[l], 0, (size_t)N * a.H[l] * a.W[l] * C * sizeof(float), s);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(rpn_scatter_kernel, dim3(N * L, ((C >> 2) + SC_Q - 1) / SC_Q), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

int seam_upsample_add_bwd_f32(const float* dlat, const float* base, float* dtop, int N, int H, int W, int Ht, int Wt, int C,
                              void* stream) {
    if (N <= 0 || H <= 0 || W <= 0 || Ht <= 0 || Wt <= 0 || C <= 0 || (C & 3) || !dlat || !dtop) return (int)hipErrorInvalidValue;
    const size_t total = (size_t)N * Ht * Wt * (C >> 2);
    hipLaunchKernelGGL(upsample_add_bwd_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, dlat, base, dtop, N, H,
                       W, Ht, Wt, C);
    return (int)hipGetLastError();
}

int seam_subsample_add_bwd_f32(float* d, const float* dpool, int N, int H, int W, int Hp, int Wp, int C, void* stream) {
    if (N <= 0 || H <= 0 || W <= 0 || Hp != (H - 1) / 2 + 1 || Wp != (W - 1) / 2 + 1 || C <= 0 || (C & 3) || !d || !dpool)
        return (int)hipErrorInvalidValue;
    const size_t total = (size_t)N * Hp * Wp * (C >> 2);
    hipLaunchKernelGGL(subsample_add_bwd_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, d, dpool, N, H, W, Hp,
                       Wp, C);
    return (int)hipGetLastError();
}

}  // extern "C"
