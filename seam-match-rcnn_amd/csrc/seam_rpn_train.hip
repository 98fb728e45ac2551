// Training branch of the RPN (torchvision RegionProposalNetwork.assign_targets_to_anchors / compute_loss [TV]): anchor
// matching with the low-quality rule, balanced sampling, the gather of the sampled 3x3 conv windows, and the two RPN losses
// fused with their gradient.
//
// A frame has up to 2^20 anchors, so nothing per anchor lives in LDS: the kernels run many workgroups per image and keep
// their state in a caller-provided workspace.  As in seam_roi_train.hip every float reduction runs in a fixed order (the
// per-GT maxima are maxima, which no order changes), and the only atomics are integer ones: histogram counts, and slot
// tickets whose order is erased by the sort that follows.  A launch is bit-identical to the next.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "seam_hip.h"
#include "seam_train_common.h"

namespace {

using namespace seam_train;

constexpr int RPN_MAX_ANCHORS = 1 << 20;   // per image
constexpr int RPN_IDX_BITS = 20;           // 2^20 == RPN_MAX_ANCHORS: an anchor index fits below the key
constexpr int RPN_MAX_GT = 128;            // GT boxes per image (they sit in LDS)
constexpr int RPN_MAX_BATCH = 1024;        // sampled anchors per image
constexpr int RPN_MAX_IMAGES = 4096;
constexpr int MATCH_CHUNK = 1024;          // anchors per workgroup of the match kernels (4 per thread)
constexpr int SAMPLE_CHUNK = 4096;         // anchors per workgroup of the sampler's streaming kernels
constexpr int GATHER_MAX_LEVELS = 8;

// ---------------------------------------------------------------------------------------------------- matcher
struct MatchArgs {
    const float* anchors;      // [A,4] shared by the batch
    const float* gt;           // [N,G,4]
    const int* n_gt;           // [N]
    int8_t* labels;            // [N,A]  -1 ignored / 0 background / 1 foreground
    int* matched;              // [N,A]  argmax GT of a foreground anchor, 0 otherwise (Matcher's clamp)
    float* partial;            // [N,nblk,G] per-workgroup maxima of each GT box's IoU
    float* gmax;               // [N,G]      each GT box's largest IoU over the image's anchors
    int A, G, nblk;
    float fg, bg;
};

__device__ __forceinline__ int load_gt(const MatchArgs& a, int img, float4* s_gt, float* s_area) {
    const int ng = min(max(a.n_gt[img], 0), a.G);
    const float4* gt = reinterpret_cast<const float4*>(a.gt) + (size_t)img * a.G;
    for (int j = threadIdx.x; j < ng; j += blockDim.x) {
        const float4 g = gt[j];
        s_gt[j] = g;
        s_area[j] = box_area(g);
    }
    return ng;
}

// pass 1: per workgroup and GT box, the largest IoU over the workgroup's MATCH_CHUNK anchors
__global__ __launch_bounds__(256) void rpn_match_gtmax_kernel(MatchArgs a) {
    __shared__ float4 s_gt[RPN_MAX_GT];
    __shared__ float s_area[RPN_MAX_GT];
    __shared__ float s_wmax[4][RPN_MAX_GT];
    const int img = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
    const int ng = load_gt(a, img, s_gt, s_area);
    __syncthreads();
    float4 p[4];
    float ap[4];
    bool ok[4];
    for (int k = 0; k < 4; ++k) {
        const int i = blk * MATCH_CHUNK + k * 256 + tid;
        ok[k] = i < a.A;
        p[k] = ok[k] ? reinterpret_cast<const float4*>(a.anchors)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        ap[k] = box_area(p[k]);
    }
    for (int j = 0; j < ng; ++j) {
        const float4 g = s_gt[j];
        const float ag = s_area[j];
        float m = -1.f;                                       // below every IoU
        for (int k = 0; k < 4; ++k)
            if (ok[k]) m = fmaxf(m, iou_gt_prop(g, ag, p[k], ap[k]));
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        if ((tid & 63) == 0) s_wmax[tid >> 6][j] = m;
    }
    __syncthreads();
    float* out = a.partial + ((size_t)img * a.nblk + blk) * a.G;
    for (int j = tid; j < ng; j += 256) out[j] = fmaxf(fmaxf(s_wmax[0][j], s_wmax[1][j]), fmaxf(s_wmax[2][j], s_wmax[3][j]));
}

// the per-GT maxima of one image from its workgroups' maxima
__global__ __launch_bounds__(256) void rpn_match_reduce_kernel(MatchArgs a) {
    __shared__ float red[4];
    const int img = blockIdx.x, tid = threadIdx.x;
    const int ng = min(max(a.n_gt[img], 0), a.G);
    const float* part = a.partial + (size_t)img * a.nblk * a.G;
    for (int j = 0; j < ng; ++j) {
        float m = -1.f;
        for (int b = tid; b < a.nblk; b += 256) m = fmaxf(m, part[(size_t)b * a.G + j]);
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        __syncthreads();
        if ((tid & 63) == 0) red[tid >> 6] = m;
        __syncthreads();
        if (tid == 0) a.gmax[(size_t)img * a.G + j] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    }
}

// pass 2: Matcher(fg, bg, allow_low_quality_matches=True).  The IoUs are the same expression on the same operands as in
// pass 1, hence the same bits: `v == gmax` finds exactly the anchors that attain a GT box's maximum.
__global__ __launch_bounds__(256) void rpn_match_label_kernel(MatchArgs a) {
    __shared__ float4 s_gt[RPN_MAX_GT];
    __shared__ float s_area[RPN_MAX_GT];
    __shared__ float s_gmax[RPN_MAX_GT];
    const int img = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
    const int ng = load_gt(a, img, s_gt, s_area);
    for (int j = tid; j < ng; j += 256) s_gmax[j] = a.gmax[(size_t)img * a.G + j];
    __syncthreads();
    for (int k = 0; k < 4; ++k) {
        const int i = blk * MATCH_CHUNK + k * 256 + tid;
        if (i >= a.A) continue;
        const float4 p = reinterpret_cast<const float4*>(a.anchors)[i];
        const float ap = box_area(p);
        float best = 0.f;
        int bj = 0;
        bool lowq = false;
        for (int j = 0; j < ng; ++j) {
            const float v = iou_gt_prop(s_gt[j], s_area[j], p, ap);
            // torch.max: the first maximum, NaN counts as the maximum
            if (j == 0 || v > best || (v != v && best == best)) { best = v; bj = j; }
            lowq |= v == s_gmax[j];
        }
        int lab;
        if (ng == 0 || best < a.bg) lab = 0;                  // an image without GT boxes: all background
        else if (best >= a.bg && best < a.fg) lab = -1;
        else lab = 1;
        if (lowq) lab = 1;                                    // restored to its own argmax GT, whichever GT box it ties
        const size_t o = (size_t)img * a.A + i;
        a.labels[o] = (int8_t)lab;
        a.matched[o] = lab == 1 ? bj : 0;
    }
}

// ---------------------------------------------------------------------------------------------------- sampler
struct SampleState {                       // per image, in the workspace
    unsigned long long pref[2];            // the selected class-c threshold, built digit by digit
    int rem[2];                            // rank still to find inside the current prefix
    int k[2];                              // anchors to keep of class c (0 negatives, 1 positives)
    int cnt[2];                            // anchors of class c
    int some[2];                           // 0 < k < cnt: a threshold is needed
    int slots;                             // ticket counter of the collect kernel
    int pad;
};

struct RpnSampleArgs {
    const int8_t* labels;      // [N,A]
    const int* matched;        // [N,A]
    const float* keys;         // [N,A]
    const float* anchors;      // [A,4]
    const float* gt;           // [N,G,4]
    int64_t* idx;              // [N,B] sampled anchor index, ascending; -1 past the count
    int64_t* slab;             // [N,B] 1 / 0; -1 past the count
    int64_t* smatched;         // [N,B]
    float* targets;            // [N,B,4] BoxCoder((1,1,1,1)).encode(matched GT, anchor) of the foreground rows, 0 elsewhere
    int* count;                // [N,2] (rows, positives)
    unsigned* hist;            // [N,2,256]
    SampleState* state;        // [N]
    int* list;                 // [N,B] sampled anchors in ticket order
    int A, G, B, pos_max;
};

__device__ __forceinline__ unsigned long long composite(float key, int i) {
    return ((unsigned long long)ord_key(key) << RPN_IDX_BITS) | (unsigned)i;
}

__global__ __launch_bounds__(256) void rpn_sample_init_kernel(RpnSampleArgs a) {
    const int img = blockIdx.x;
    for (int j = threadIdx.x; j < 512; j += 256) a.hist[(size_t)img * 512 + j] = 0u;
    if (threadIdx.x == 0) {
        SampleState s;
        s.pref[0] = s.pref[1] = 0ull;
        s.rem[0] = s.rem[1] = s.k[0] = s.k[1] = s.cnt[0] = s.cnt[1] = 0;
        s.some[0] = s.some[1] = 1;                            // the first pass counts every anchor of both classes
        s.slots = 0;
        s.pad = 0;
        a.state[img] = s;
    }
}

// one digit (8 bits at `shift`) of the composites that share the prefix found so far, per class
__global__ __launch_bounds__(256) void rpn_sample_hist_kernel(RpnSampleArgs a, int shift) {
    __shared__ unsigned s_hist[2][256];
    const int img = blockIdx.y, tid = threadIdx.x;
    const SampleState st = a.state[img];
    if (!st.some[0] && !st.some[1]) return;
    s_hist[0][tid] = 0u;
    s_hist[1][tid] = 0u;
    __syncthreads();
    const int8_t* lab = a.labels + (size_t)img * a.A;
    const float* keys = a.keys + (size_t)img * a.A;
    const unsigned long long hi0 = st.pref[0] >> (shift + 8), hi1 = st.pref[1] >> (shift + 8);
    const int i1 = min((blockIdx.x + 1) * SAMPLE_CHUNK, a.A);
    for (int i = blockIdx.x * SAMPLE_CHUNK + tid; i < i1; i += 256) {
        const int c = lab[i];
        if (c < 0 || c > 1 || !st.some[c]) continue;
        const unsigned long long comp = composite(keys[i], i);
        if ((comp >> (shift + 8)) == (c ? hi1 : hi0)) atomicAdd(&s_hist[c][(comp >> shift) & 255u], 1u);
    }
    __syncthreads();
    for (int c = 0; c < 2; ++c)
        if (s_hist[c][tid]) atomicAdd(&a.hist[((size_t)img * 2 + c) * 256 + tid], s_hist[c][tid]);
}

// the digit that holds the k-th smallest composite; `first`: the histogram is of every anchor, so it also gives the
// class counts and with them num_pos / num_neg of BalancedPositiveNegativeSampler
__global__ __launch_bounds__(64) void rpn_sample_select_kernel(RpnSampleArgs a, int shift, int first) {
    const int img = blockIdx.x, tid = threadIdx.x;
    unsigned* hist = a.hist + (size_t)img * 512;
    if (tid == 0) {
        SampleState st = a.state[img];
        if (first) {
            for (int c = 0; c < 2; ++c) {
                int s = 0;
                for (int b = 0; b < 256; ++b) s += (int)hist[c * 256 + b];
                st.cnt[c] = s;
            }
            const int np = min(st.cnt[1], a.pos_max);
            const int nn = min(st.cnt[0], a.B - np);
            st.k[1] = np; st.k[0] = nn;
            st.rem[1] = np; st.rem[0] = nn;
            st.some[0] = nn > 0 && nn < st.cnt[0];
            st.some[1] = np > 0 && np < st.cnt[1];
        }
        for (int c = 0; c < 2; ++c) {
            if (!st.some[c]) continue;
            int cum = 0, b = 0;
            for (; b < 255; ++b) {
                const int h = (int)hist[c * 256 + b];
                if (cum + h >= st.rem[c]) break;
                cum += h;
            }
            st.rem[c] -= cum;
            st.pref[c] |= (unsigned long long)b << shift;
        }
        a.state[img] = st;
    }
    __syncthreads();                                           // thread 0 has read the histogram: clear it for the next pass
    for (int j = tid; j < 512; j += 64) hist[j] = 0u;
}

// every kept anchor takes a ticket and writes its index there; the ticket order is erased by the rank sort below
__global__ __launch_bounds__(256) void rpn_sample_collect_kernel(RpnSampleArgs a) {
    const int img = blockIdx.y, tid = threadIdx.x;
    const SampleState st = a.state[img];
    const int8_t* lab = a.labels + (size_t)img * a.A;
    const float* keys = a.keys + (size_t)img * a.A;
    const int i1 = min((blockIdx.x + 1) * SAMPLE_CHUNK, a.A);
    for (int i = blockIdx.x * SAMPLE_CHUNK + tid; i < i1; i += 256) {
        const int c = lab[i];
        if (c < 0 || c > 1) continue;
        bool sel;
        if (!st.some[c]) sel = st.k[c] > 0;                   // none or all of the class
        else sel = composite(keys[i], i) <= st.pref[c];
        if (!sel) continue;
        const int slot = atomicAdd(&a.state[img].slots, 1);
        if (slot < a.B) a.list[(size_t)img * a.B + slot] = i;
    }
}

// ascending order (nonzero(pos | neg)) by ranking the <= B distinct indices, then labels, matches and targets
__global__ __launch_bounds__(256) void rpn_sample_final_kernel(RpnSampleArgs a) {
    __shared__ int s_list[RPN_MAX_BATCH];
    const int img = blockIdx.x, tid = threadIdx.x;
    const SampleState st = a.state[img];
    const int total = min(st.slots, a.B);
    for (int t = tid; t < total; t += 256) s_list[t] = a.list[(size_t)img * a.B + t];
    __syncthreads();
    const size_t ob = (size_t)img * a.B;
    const float4* gt = reinterpret_cast<const float4*>(a.gt) + (size_t)img * a.G;
    for (int t = tid; t < total; t += 256) {
        const int v = s_list[t];
        int rank = 0;
        for (int u = 0; u < total; ++u) rank += s_list[u] < v ? 1 : 0;
        const size_t o = ob + rank;
        const size_t src = (size_t)img * a.A + v;
        const int lab = a.labels[src];
        const int m = a.matched[src];
        a.idx[o] = v;
        a.slab[o] = lab;
        a.smatched[o] = m;
        float* to = a.targets + o * 4;
        if (lab == 1 && m >= 0 && m < a.G) {
#pragma clang fp contract(off)
            const float4 p = reinterpret_cast<const float4*>(a.anchors)[v];
            const float4 g = gt[m];
            const float exw = p.z - p.x, exh = p.w - p.y;
            const float excx = p.x + 0.5f * exw, excy = p.y + 0.5f * exh;
            const float gw = g.z - g.x, gh = g.w - g.y;
            const float gcx = g.x + 0.5f * gw, gcy = g.y + 0.5f * gh;
            to[0] = (gcx - excx) / exw;
            to[1] = (gcy - excy) / exh;
            to[2] = logf(gw / exw);
            to[3] = logf(gh / exh);
        } else {
            to[0] = 0.f; to[1] = 0.f; to[2] = 0.f; to[3] = 0.f;
        }
    }
    for (int j = total + tid; j < a.B; j += 256) {
        const size_t o = ob + j;
        a.idx[o] = -1; a.slab[o] = -1; a.smatched[o] = -1;
        for (int c = 0; c < 4; ++c) a.targets[o * 4 + c] = 0.f;
    }
    if (tid == 0) { a.count[2 * img] = total; a.count[2 * img + 1] = st.k[1]; }
}

// ---------------------------------------------------------------------------------------------------- patch gather
struct GatherArgs {
    const float* maps[GATHER_MAX_LEVELS];  // NHWC [N,H_l,W_l,C]
    int H[GATHER_MAX_LEVELS], W[GATHER_MAX_LEVELS];
    const int* rows;                       // [M,4] (image, level, y, x)
    float* out;                            // [M,3,3,C]
    int M, N, L, C;
};

// one workgroup per row: the 3x3 window around (y, x), zeros outside the map (the conv's padding) and for a row whose
// image / level / pixel is out of range; a tap is C contiguous floats, moved as float4
__global__ __launch_bounds__(256) void rpn_gather_kernel(GatherArgs a) {
    const int r = blockIdx.x;
    const int4 row = reinterpret_cast<const int4*>(a.rows)[r];
    const int img = row.x, lvl = row.y, y = row.z, x = row.w;
    const int c4 = a.C >> 2;
    float4* out = reinterpret_cast<float4*>(a.out) + (size_t)r * 9 * c4;
    const bool ok = img >= 0 && img < a.N && lvl >= 0 && lvl < a.L;
    int H = 0, W = 0;
    const float4* map = nullptr;
    if (ok) {
        // (a select chain, not an indexed read of the by-value argument arrays: those would go through scratch)
        for (int l = 0; l < GATHER_MAX_LEVELS; ++l)
            if (l == lvl) { H = a.H[l]; W = a.W[l]; map = reinterpret_cast<const float4*>(a.maps[l]); }
    }
    const bool in = ok && y >= 0 && y < H && x >= 0 && x < W;
    for (int e = threadIdx.x; e < 9 * c4; e += 256) {
        const int tap = e / c4, q = e - tap * c4;
        const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (in && yy >= 0 && yy < H && xx >= 0 && xx < W) v = map[(((size_t)img * H + yy) * W + xx) * c4 + q];
        out[e] = v;
    }
}

// ---------------------------------------------------------------------------------------------------- losses
// RegionProposalNetwork.compute_loss [TV] on the M sampled rows: BCE-with-logits of the row's objectness logit (mean),
// smooth-L1 (beta 1/9, summed, / M) of the foreground rows' 4 deltas; both gradients into grad [M,GC] (zeros elsewhere).
// One 256-thread block, thread t takes rows t, t+256, ...
__global__ __launch_bounds__(256) void rpn_loss_kernel(const float* __restrict__ head, const int* __restrict__ slot,
                                                       const int64_t* __restrict__ labels, const float* __restrict__ tgt,
                                                       float* __restrict__ loss, float* __restrict__ grad, int M, int A, int ld,
                                                       int GC) {
    __shared__ float red[4];
    const float beta = 1.f / 9.f;
    const float rn = (float)M;
    float s_obj = 0.f, s_box = 0.f;
    bool bad = false;
    for (int r = threadIdx.x; r < M; r += 256) {
        const float* h = head + (size_t)r * ld;
        float* g = grad + (size_t)r * GC;
        for (int j = 0; j < GC; ++j) g[j] = 0.f;
        const int s = slot[r];
        const int64_t y64 = labels[r];
        const bool ok = s >= 0 && s < A && (y64 == 0 || y64 == 1);
        bad |= !ok;
        if (!ok) continue;
        const float x = h[s], y = (float)y64;
        s_obj += (fmaxf(x, 0.f) - x * y) + log1pf(expf(-fabsf(x)));
        g[s] = (1.f / (1.f + expf(-x)) - y) / rn;
        if (y64 == 1) {
            for (int c = 0; c < 4; ++c) {
                const float d = h[A + 4 * s + c] - tgt[(size_t)r * 4 + c];
                const float an = fabsf(d);
                s_box += an < beta ? 0.5f * an * an / beta : an - 0.5f * beta;
                g[A + 4 * s + c] = (an < beta ? d / beta : (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f))) / rn;
            }
        }
    }
    s_obj = block_sum256(s_obj, red);
    s_box = block_sum256(s_box, red);
    const float nbad = block_sum256(bad ? 1.f : 0.f, red);
    if (threadIdx.x == 0) {
        loss[0] = nbad > 0.f ? __int_as_float(0x7fc00000) : s_obj / rn;
        loss[1] = nbad > 0.f ? __int_as_float(0x7fc00000) : s_box / rn;
    }
}

inline int64_t align16(int64_t v) { return (v + 15) / 16 * 16; }
inline int match_blocks(int A) { return (A + MATCH_CHUNK - 1) / MATCH_CHUNK; }

}  // namespace

extern "C" {

int seam_rpn_max_gt(void) { return RPN_MAX_GT; }

int64_t seam_rpn_match_workspace_floats(int N, int A, int G) {
    if (N <= 0 || N > RPN_MAX_IMAGES || A <= 0 || A > RPN_MAX_ANCHORS || G <= 0 || G > RPN_MAX_GT) return 0;
    return (int64_t)N * match_blocks(A) * G + (int64_t)N * G;
}

int seam_rpn_match_f32(const float* anchors, const float* gt_boxes, const int* n_gt, int N, int A, int G, float fg_thresh,
                       float bg_thresh, int8_t* labels, int* matched, float* ws, void* stream) {
    if (N <= 0 || N > RPN_MAX_IMAGES || A <= 0 || A > RPN_MAX_ANCHORS || G <= 0 || G > RPN_MAX_GT || !(bg_thresh <= fg_thresh) ||
        !anchors || !gt_boxes || !n_gt || !labels || !matched || !ws)
        return (int)hipErrorInvalidValue;
    const int nblk = match_blocks(A);
    MatchArgs a{anchors, gt_boxes, n_gt, labels, matched, ws, ws + (size_t)N * nblk * G, A, G, nblk, fg_thresh, bg_thresh};
    hipLaunchKernelGGL(rpn_match_gtmax_kernel, dim3(nblk, N), dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(rpn_match_reduce_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(rpn_match_label_kernel, dim3(nblk, N), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int64_t seam_rpn_sample_workspace_bytes(int N, int batch) {
    if (N <= 0 || N > RPN_MAX_IMAGES || batch <= 0 || batch > RPN_MAX_BATCH) return 0;
    return align16((int64_t)N * 512 * sizeof(unsigned)) + align16((int64_t)N * sizeof(SampleState)) +
           align16((int64_t)N * batch * sizeof(int));
}

int seam_rpn_sample_f32(const int8_t* labels, const int* matched, const float* keys, const float* anchors, const float* gt_boxes,
                        int N, int A, int G, int batch, int pos_max, int64_t* idx, int64_t* slabels, int64_t* smatched,
                        float* targets, int* count, void* ws, void* stream) {
    if (N <= 0 || N > RPN_MAX_IMAGES || A <= 0 || A > RPN_MAX_ANCHORS || G <= 0 || G > RPN_MAX_GT || batch <= 0 ||
        batch > RPN_MAX_BATCH || pos_max < 0 || pos_max > batch || !labels || !matched || !keys || !anchors || !gt_boxes || !idx ||
        !slabels || !smatched || !targets || !count || !ws)
        return (int)hipErrorInvalidValue;
    char* w = static_cast<char*>(ws);
    unsigned* hist = reinterpret_cast<unsigned*>(w);
    w += align16((int64_t)N * 512 * sizeof(unsigned));
    SampleState* state = reinterpret_cast<SampleState*>(w);
    w += align16((int64_t)N * sizeof(SampleState));
    int* list = reinterpret_cast<int*>(w);
    RpnSampleArgs a{labels, matched, keys, anchors, gt_boxes, idx, slabels, smatched, targets, count, hist, state, list,
                    A, G, batch, pos_max};
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((A + SAMPLE_CHUNK - 1) / SAMPLE_CHUNK, N);
    hipLaunchKernelGGL(rpn_sample_init_kernel, dim3(N), dim3(256), 0, s, a);
    // 52-bit composite ord(key) << 20 | index, 8 bits per pass from bit 48 down
    for (int shift = 48; shift >= 0; shift -= 8) {
        hipLaunchKernelGGL(rpn_sample_hist_kernel, grid, dim3(256), 0, s, a, shift);
        hipLaunchKernelGGL(rpn_sample_select_kernel, dim3(N), dim3(64), 0, s, a, shift, shift == 48 ? 1 : 0);
    }
    hipLaunchKernelGGL(rpn_sample_collect_kernel, grid, dim3(256), 0, s, a);
    hipLaunchKernelGGL(rpn_sample_final_kernel, dim3(N), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

int seam_rpn_gather_patches_f32(const void* const* maps, const int* hw, const int* rows, int M, int N, int L, int C, float* out,
                                void* stream) {
    if (M <= 0 || M > (1 << 20) || N <= 0 || L <= 0 || L > GATHER_MAX_LEVELS || C <= 0 || C > 4096 || (C & 3) || !maps || !hw ||
        !rows || !out)
        return (int)hipErrorInvalidValue;
    GatherArgs a{};
    for (int l = 0; l < L; ++l) {
        if (!maps[l] || hw[2 * l] <= 0 || hw[2 * l + 1] <= 0) return (int)hipErrorInvalidValue;
        a.maps[l] = static_cast<const float*>(maps[l]);
        a.H[l] = hw[2 * l];
        a.W[l] = hw[2 * l + 1];
    }
    a.rows = rows; a.out = out; a.M = M; a.N = N; a.L = L; a.C = C;
    hipLaunchKernelGGL(rpn_gather_kernel, dim3(M), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int seam_rpn_loss_fwd_bwd_f32(const float* head, const int* slot, const int64_t* labels, const float* targets, int M, int A,
                              int head_cols, int grad_cols, float* loss, float* grad, void* stream) {
    if (M <= 0 || M > (1 << 20) || A <= 0 || A > 64 || head_cols < 5 * A || head_cols > 1024 || grad_cols < 5 * A ||
        grad_cols > 1024 || !head || !slot || !labels || !targets || !loss || !grad)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(rpn_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, head, slot, labels, targets, loss, grad, M, A,
                       head_cols, grad_cols);
    return (int)hipGetLastError();
}

}  // extern "C"
