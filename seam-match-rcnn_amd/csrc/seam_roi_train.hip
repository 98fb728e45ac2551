// Training branch of the RoI heads (ref models/matchrcnn.py:333-472 with torchvision's roi_heads helpers [TV]):
// proposal sampling per image, the Fast R-CNN losses and the mask loss, each fused with its logits gradient.
//
// Every kernel here reduces in a fixed order (per-thread loops, then a fixed butterfly / tree), so a launch is
// bit-identical to the next.  There are no float atomics; the sampler's LDS histograms use integer atomics, whose
// result does not depend on the order of the adds.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "seam_hip.h"
#include "seam_train_common.h"

namespace {

using namespace seam_train;       // block_sum256, ord_key, iou_gt_prop, box_area

constexpr int SAMPLE_THREADS = 1024;
constexpr int SAMPLE_MAX_CAND = 16384;     // == NMS_MAX_BOXES: rpn_post_nms_top_n_train (8000) + the GT boxes fit
constexpr int SAMPLE_IDX_BITS = 14;        // 2^14 == SAMPLE_MAX_CAND: a candidate index fits below the key
constexpr int MASK_M = 28;                 // mask target resolution (MaskRCNNPredictor output)

// exclusive prefix sum of v over a 1024-thread block (thread order); *total = the sum of all v
__device__ __forceinline__ int block_scan1024(int v, int* s_wave, int* total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    __syncthreads();
    if (lane == 63) s_wave[wid] = x;
    __syncthreads();
    int base = 0, tot = 0;
    for (int w = 0; w < SAMPLE_THREADS / 64; ++w) {
        const int t = s_wave[w];
        base += w < wid ? t : 0;
        tot += t;
    }
    *total = tot;
    return base + x - v;
}

struct SampleArgs {
    const float* cand;         // [N,P,4] proposals followed by the image's GT boxes
    const int* n_cand;         // [N]
    const float* keys;         // [N,P] one uniform key per candidate
    const float* gt;           // [N,G,4]
    const int64_t* gt_labels;  // [N,G]
    const int* n_gt;           // [N]
    int64_t* idx;              // [N,B] sampled candidate index, ascending; -1 past the count
    int64_t* labels;           // [N,B]
    int64_t* matched;          // [N,B] matched GT (0 for background, as Matcher's clamp gives)
    float* boxes;              // [N,B,4] the sampled candidate boxes
    float* targets;            // [N,B,4] BoxCoder.encode(matched GT, candidate)
    int* count;                // [N,2] (sampled rows, positives); -1 when the image has no GT box
    int P, G, B, pos_max;
    float wx, wy, ww, wh;
};

// One workgroup per image.  1) Matcher(0.5, 0.5, allow_low_quality_matches=False) on the max over GT boxes, first index
// on ties; labels from the matched GT, 0 below 0.5.  2) BalancedPositiveNegativeSampler: the num_pos positives
// (label >= 1) and num_neg negatives (label == 0) with the smallest (key, index), found by a radix select over the
// 46-bit composite ord(key) << 14 | index (unique, so exactly k of each class are kept).  3) Compaction in ascending
// index order (nonzero(pos | neg)).  4) encode with weights (wx, wy, ww, wh).
__global__ __launch_bounds__(SAMPLE_THREADS) void roi_sample_kernel(SampleArgs a) {
    __shared__ short s_match[SAMPLE_MAX_CAND];          // matched GT, -1 = below the threshold
    __shared__ unsigned char s_cls[SAMPLE_MAX_CAND];    // 0 negative, 1 positive, 2 neither
    __shared__ unsigned s_hist[2][256];
    __shared__ unsigned long long s_pref[2];
    __shared__ int s_rem[2], s_cnt[2], s_k[2];
    __shared__ int s_wave[SAMPLE_THREADS / 64];
    const int img = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(a.n_cand[img], 0), a.P);
    const int ng = min(max(a.n_gt[img], 0), a.G);
    const float4* cand = reinterpret_cast<const float4*>(a.cand) + (size_t)img * a.P;
    const float* keys = a.keys + (size_t)img * a.P;
    const float4* gt = reinterpret_cast<const float4*>(a.gt) + (size_t)img * a.G;
    const int64_t* gl = a.gt_labels + (size_t)img * a.G;
    const size_t ob = (size_t)img * a.B;
    if (ng == 0) {                                      // Matcher raises on an image without GT boxes: flag it
        for (int j = tid; j < a.B; j += SAMPLE_THREADS) {
            a.idx[ob + j] = -1; a.labels[ob + j] = -1; a.matched[ob + j] = -1;
            for (int c = 0; c < 4; ++c) { a.boxes[(ob + j) * 4 + c] = 0.f; a.targets[(ob + j) * 4 + c] = 0.f; }
        }
        if (tid == 0) { a.count[2 * img] = -1; a.count[2 * img + 1] = -1; }
        return;
    }
    if (tid < 2) s_cnt[tid] = 0;
    __syncthreads();
    // 1) match
    int my_cnt[2] = {0, 0};
    for (int i = tid; i < n; i += SAMPLE_THREADS) {
        const float4 p = cand[i];
        const float ap = box_area(p);
        float best = 0.f;
        int bj = 0;
        for (int j = 0; j < ng; ++j) {
            const float4 g = gt[j];
            const float v = iou_gt_prop(g, box_area(g), p, ap);
            // torch.max: the first maximum, NaN counts as the maximum
            if (j == 0 || v > best || (v != v && best == best)) { best = v; bj = j; }
        }
        const bool fg = !(best < 0.5f);                  // below the low threshold -> background (NaN stays matched)
        s_match[i] = fg ? (short)bj : (short)-1;
        const int64_t lab = fg ? gl[bj] : 0;
        const int c = lab >= 1 ? 1 : (lab == 0 ? 0 : 2);
        s_cls[i] = (unsigned char)c;
        if (c < 2) ++my_cnt[c];
    }
    if (my_cnt[0]) atomicAdd(&s_cnt[0], my_cnt[0]);
    if (my_cnt[1]) atomicAdd(&s_cnt[1], my_cnt[1]);
    __syncthreads();
    if (tid == 0) {
        const int np = min(s_cnt[1], a.pos_max);
        const int nn = min(s_cnt[0], a.B - np);
        s_k[1] = np; s_k[0] = nn;
        s_rem[0] = nn; s_rem[1] = np;
        s_pref[0] = 0ull; s_pref[1] = 0ull;
    }
    __syncthreads();
    // 2) radix select, 8 bits per pass from bit 40 down; a class whose k is 0 or its whole count needs no threshold
    const bool sel_some[2] = {s_k[0] > 0 && s_k[0] < s_cnt[0], s_k[1] > 0 && s_k[1] < s_cnt[1]};
    if (sel_some[0] || sel_some[1]) {
        for (int shift = 40; shift >= 0; shift -= 8) {
            for (int j = tid; j < 512; j += SAMPLE_THREADS) (&s_hist[0][0])[j] = 0u;
            __syncthreads();
            const unsigned long long hi0 = s_pref[0] >> (shift + 8), hi1 = s_pref[1] >> (shift + 8);
            for (int i = tid; i < n; i += SAMPLE_THREADS) {
                const int c = s_cls[i];
                if (c > 1 || !sel_some[c]) continue;
                const unsigned long long comp = ((unsigned long long)ord_key(keys[i]) << SAMPLE_IDX_BITS) | (unsigned)i;
                if ((comp >> (shift + 8)) == (c ? hi1 : hi0)) atomicAdd(&s_hist[c][(comp >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0 || tid == 64) {                 // one lane of two different waves, one class each
                const int c = tid ? 1 : 0;
                if (sel_some[c]) {
                    int rem = s_rem[c], cum = 0, b = 0;
                    for (; b < 255; ++b) {
                        if (cum + (int)s_hist[c][b] >= rem) break;
                        cum += (int)s_hist[c][b];
                    }
                    s_rem[c] = rem - cum;
                    s_pref[c] |= (unsigned long long)b << shift;
                }
            }
            __syncthreads();
        }
    }
    const unsigned long long thr0 = s_pref[0], thr1 = s_pref[1];
    const int k0 = s_k[0], k1 = s_k[1];
    // 3) compaction: thread t owns the contiguous index range [t*per, (t+1)*per)
    const int per = (n + SAMPLE_THREADS - 1) / SAMPLE_THREADS;
    const int i0 = min(tid * per, n), i1 = min(i0 + per, n);
    auto selected = [&](int i) -> bool {
        const int c = s_cls[i];
        if (c > 1) return false;
        const bool some = c ? sel_some[1] : sel_some[0];
        if (!some) return (c ? k1 : k0) > 0;              // none or all of the class
        const unsigned long long comp = ((unsigned long long)ord_key(keys[i]) << SAMPLE_IDX_BITS) | (unsigned)i;
        return comp <= (c ? thr1 : thr0);
    };
    int mine = 0;
    for (int i = i0; i < i1; ++i) mine += selected(i) ? 1 : 0;
    int total = 0;
    int pos = block_scan1024(mine, s_wave, &total);
    // 4) write the sampled rows
    for (int i = i0; i < i1; ++i) {
        if (!selected(i)) continue;
        const int m = s_match[i];
        const int mg = m < 0 ? 0 : m;
        const float4 p = cand[i];
        const float4 g = gt[mg];
        const size_t o = ob + pos;
        a.idx[o] = i;
        a.labels[o] = m < 0 ? 0 : gl[m];
        a.matched[o] = mg;
        {
#pragma clang fp contract(off)
            const float exw = p.z - p.x, exh = p.w - p.y;
            const float excx = p.x + 0.5f * exw, excy = p.y + 0.5f * exh;
            const float gw = g.z - g.x, gh = g.w - g.y;
            const float gcx = g.x + 0.5f * gw, gcy = g.y + 0.5f * gh;
            float* bo = a.boxes + o * 4;
            float* to = a.targets + o * 4;
            bo[0] = p.x; bo[1] = p.y; bo[2] = p.z; bo[3] = p.w;
            to[0] = a.wx * (gcx - excx) / exw;
            to[1] = a.wy * (gcy - excy) / exh;
            to[2] = a.ww * logf(gw / exw);
            to[3] = a.wh * logf(gh / exh);
        }
        ++pos;
    }
    for (int j = total + tid; j < a.B; j += SAMPLE_THREADS) {
        const size_t o = ob + j;
        a.idx[o] = -1; a.labels[o] = -1; a.matched[o] = -1;
        for (int c = 0; c < 4; ++c) { a.boxes[o * 4 + c] = 0.f; a.targets[o * 4 + c] = 0.f; }
    }
    if (tid == 0) { a.count[2 * img] = total; a.count[2 * img + 1] = k1; }
}

// fastrcnn_loss [TV]: cross entropy over all R rows (mean) and smooth-L1 (beta 1/9, summed, / R) on the label's 4 deltas of
// the positive rows, with both logits gradients.  One 256-thread block: thread t takes rows t, t+256, ...
__global__ __launch_bounds__(256) void fastrcnn_loss_kernel(const float* __restrict__ cls, const float* __restrict__ box,
                                                            const int64_t* __restrict__ labels, const float* __restrict__ tgt,
                                                            float* __restrict__ loss, float* __restrict__ dcls,
                                                            float* __restrict__ dbox, int R, int ncls) {
    __shared__ float red[4];
    const float beta = 1.f / 9.f;
    const float rn = (float)R;
    float s_ce = 0.f, s_box = 0.f;
    bool bad = false;
    for (int r = threadIdx.x; r < R; r += 256) {
        const float* x = cls + (size_t)r * ncls;
        float* dx = dcls + (size_t)r * ncls;
        float* db = dbox + (size_t)r * ncls * 4;
        const int64_t y64 = labels[r];
        const bool ok = y64 >= 0 && y64 < ncls;
        bad |= !ok;
        const int y = ok ? (int)y64 : 0;
        float m = x[0];
        for (int j = 1; j < ncls; ++j) m = fmaxf(m, x[j]);
        float s = 0.f;
        for (int j = 0; j < ncls; ++j) s += expf(x[j] - m);
        s_ce += (m + logf(s)) - x[y];
        for (int j = 0; j < ncls; ++j) dx[j] = ok ? (expf(x[j] - m) / s - (j == y ? 1.f : 0.f)) / rn : 0.f;
        for (int j = 0; j < 4 * ncls; ++j) db[j] = 0.f;
        if (ok && y > 0) {
            const float* bx = box + (size_t)r * ncls * 4 + (size_t)y * 4;
            for (int c = 0; c < 4; ++c) {
                const float d = bx[c] - tgt[(size_t)r * 4 + c];
                const float an = fabsf(d);
                s_box += an < beta ? 0.5f * an * an / beta : an - 0.5f * beta;
                db[y * 4 + c] = (an < beta ? d / beta : (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f))) / rn;
            }
        }
    }
    s_ce = block_sum256(s_ce, red);
    s_box = block_sum256(s_box, red);
    const float nbad = block_sum256(bad ? 1.f : 0.f, red);
    if (threadIdx.x == 0) {
        loss[0] = nbad > 0.f ? __int_as_float(0x7fc00000) : s_ce / rn;
        loss[1] = nbad > 0.f ? __int_as_float(0x7fc00000) : s_box / rn;
    }
}

struct MaskLossArgs {
    const float* logits;       // [P,14,14,4,ncls] sub-pixel layout of MaskRCNNPredictor.forward
    const int64_t* labels;     // [P]
    const float* rois;         // [P,4] xyxy, in the masks' frame
    const unsigned char* masks;
    const int64_t* mask_off;   // [P] byte offset of each ROI's GT mask in `masks`
    const int* mask_hw;        // [P,2]
    float* dlogits;            // like logits
    float* partial;            // [P]
    int P, ncls;
    float total;               // P * 784 (exact in fp32)
};

// maskrcnn_loss [TV] per ROI: the target is roi_align(gt_mask[:,None], roi, 28, spatial_scale=1, sampling_ratio=-1,
// aligned=False) computed here from the uint8 mask (adaptive grid of ceil(roi_h/28) x ceil(roi_w/28) samples per bin, any
// size: the loops have no fixed bound), never stored; the loss is BCE-with-logits on the label channel, its gradient is
// written into the sub-pixel layout (zeros in every other channel).  One 256-thread block per ROI, thread t takes bins t, t+256, ...
__global__ __launch_bounds__(256) void mask_loss_kernel(MaskLossArgs a) {
    __shared__ float red[4];
    const int k = blockIdx.x;
    const float4 b = reinterpret_cast<const float4*>(a.rois)[k];
    const int H = a.mask_hw[2 * k], W = a.mask_hw[2 * k + 1];
    const int64_t lab64 = a.labels[k];
    const bool ok = lab64 >= 0 && lab64 < a.ncls && H > 0 && W > 0;
    const int lab = ok ? (int)lab64 : 0;
    const unsigned char* m = a.masks + (ok ? a.mask_off[k] : 0);
    float roi_w, roi_h, bin_w, bin_h;
    int grid_w, grid_h;
    {
#pragma clang fp contract(off)
        roi_w = fmaxf(b.z - b.x, 1.f);
        roi_h = fmaxf(b.w - b.y, 1.f);
        bin_h = roi_h / (float)MASK_M;
        bin_w = roi_w / (float)MASK_M;
        grid_h = (int)ceilf(roi_h / (float)MASK_M);
        grid_w = (int)ceilf(roi_w / (float)MASK_M);
    }
    const float count = (float)max(grid_h * grid_w, 1);
    float s = 0.f;
    for (int o = threadIdx.x; o < MASK_M * MASK_M; o += 256) {
        const int ph = o / MASK_M, pw = o - ph * MASK_M;
        float acc = 0.f;
        if (ok) {
#pragma clang fp contract(off)
            for (int iy = 0; iy < grid_h; ++iy) {
                float y = b.y + (float)ph * bin_h + ((float)iy + .5f) * bin_h / (float)grid_h;
                for (int ix = 0; ix < grid_w; ++ix) {
                    float x = b.x + (float)pw * bin_w + ((float)ix + .5f) * bin_w / (float)grid_w;
                    if (y < -1.f || y > (float)H || x < -1.f || x > (float)W) continue;
                    float yy = y <= 0.f ? 0.f : y, xx = x <= 0.f ? 0.f : x;
                    int yl = (int)yy, xl = (int)xx, yh, xh;
                    if (yl >= H - 1) { yh = yl = H - 1; yy = (float)yl; } else yh = yl + 1;
                    if (xl >= W - 1) { xh = xl = W - 1; xx = (float)xl; } else xh = xl + 1;
                    const float ly = yy - (float)yl, lx = xx - (float)xl, hy = 1.f - ly, hx = 1.f - lx;
                    const float v1 = m[(size_t)yl * W + xl], v2 = m[(size_t)yl * W + xh];
                    const float v3 = m[(size_t)yh * W + xl], v4 = m[(size_t)yh * W + xh];
                    acc += ((hy * hx) * v1 + (hy * lx) * v2) + ((ly * hx) * v3 + (ly * lx) * v4);
                }
            }
        }
        const float t = acc / count;
        const int h = ph >> 1, w = pw >> 1, g = ((ph & 1) << 1) | (pw & 1);
        const size_t base = ((((size_t)k * 14 + h) * 14 + w) * 4 + g) * a.ncls;
        const float xv = a.logits[base + lab];
        s += ok ? (fmaxf(xv, 0.f) - xv * t) + log1pf(expf(-fabsf(xv))) : __int_as_float(0x7fc00000);
        const float gr = (1.f / (1.f + expf(-xv)) - t) / a.total;
        float* d = a.dlogits + base;
        for (int c = 0; c < a.ncls; ++c) d[c] = (ok && c == lab) ? gr : 0.f;
    }
    s = block_sum256(s, red);
    if (threadIdx.x == 0) a.partial[k] = s;
}

__global__ __launch_bounds__(256) void mask_loss_final_kernel(const float* __restrict__ partial, float* __restrict__ loss, int P,
                                                              float total) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < P; i += 256) s += partial[i];
    s = block_sum256(s, red);
    if (threadIdx.x == 0) loss[0] = s / total;
}

}  // namespace

extern "C" {

int seam_roi_sample_f32(const float* cand, const int* n_cand, const float* keys, const float* gt_boxes, const int64_t* gt_labels,
                        const int* n_gt, int N, int P, int G, int batch, int pos_max, float wx, float wy, float ww, float wh,
                        int64_t* idx, int64_t* labels, int64_t* matched, float* boxes, float* targets, int* count,
                        void* stream) {
    if (N <= 0 || P <= 0 || P > SAMPLE_MAX_CAND || G <= 0 || G > 32767 || batch <= 0 || batch > SAMPLE_MAX_CAND ||
        pos_max < 0 || pos_max > batch || !cand || !n_cand || !keys || !gt_boxes || !gt_labels || !n_gt || !idx || !labels ||
        !matched || !boxes || !targets || !count)
        return (int)hipErrorInvalidValue;
    SampleArgs a{cand, n_cand, keys, gt_boxes, gt_labels, n_gt, idx, labels, matched, boxes, targets, count,
                 P, G, batch, pos_max, wx, wy, ww, wh};
    hipLaunchKernelGGL(roi_sample_kernel, dim3(N), dim3(SAMPLE_THREADS), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int seam_fastrcnn_loss_fwd_bwd_f32(const float* class_logits, const float* box_regression, const int64_t* labels,
                                   const float* targets, int R, int ncls, float* loss, float* dclass, float* dbox,
                                   void* stream) {
    if (R <= 0 || ncls <= 0 || ncls > (1 << 20) || !class_logits || !box_regression || !labels || !targets || !loss || !dclass ||
        !dbox)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(fastrcnn_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, class_logits, box_regression, labels,
                       targets, loss, dclass, dbox, R, ncls);
    return (int)hipGetLastError();
}

int seam_mask_loss_fwd_bwd_f32(const float* logits, const int64_t* labels, const float* rois, const uint8_t* masks,
                               const int64_t* mask_off, const int* mask_hw, int P, int ncls, float* loss, float* dlogits,
                               float* ws, void* stream) {
    if (P <= 0 || P > (1 << 24) / (MASK_M * MASK_M) || ncls <= 0 || ncls > (1 << 16) || !logits || !labels || !rois || !masks ||
        !mask_off || !mask_hw || !loss || !dlogits || !ws)
        return (int)hipErrorInvalidValue;
    const float total = (float)(P * MASK_M * MASK_M);        // exact: P * 784 < 2^24
    MaskLossArgs a{logits, labels, rois, masks, mask_off, mask_hw, dlogits, ws, P, ncls, total};
    hipLaunchKernelGGL(mask_loss_kernel, dim3(P), dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(mask_loss_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)ws, loss, P, total);
    return (int)hipGetLastError();
}

}  // extern "C"
