// seam_body_train.hip -- what the ResNet body backward needs beyond the stride-1 convolutions (include/seam_hip.h, "Training the
// ResNet body"):
//   seam_pack_conv3x3s2_dgrad_f32  OIHW weight (+ FrozenBN scale) -> the tap-major [9][C][K] rows of the kernel below
//   seam_conv3x3s2_dgrad_f32       input gradient of a 3x3 / stride-2 / pad-1 conv (layer{2,3,4}.0.conv2), gather form
//   seam_relu_mask_add_f32         out = y > 0 ? a + b : 0 (the ReLU at a block's output, where two gradients meet)
//   seam_maxpool3s2_relu_bwd_f32   adjoint of the stem's 3x3 / stride-2 / pad-1 max-pool with the stem's ReLU mask (below)
//
// The stride-2 input gradient.  h = 2*ho + r - 1, so an even input row has the one tap r = 1 (ho = h/2) and an odd row the taps
// r = 0 (ho = (h+1)/2) and r = 2 (ho = (h-1)/2); columns alike.  The input pixels fall into four (row parity, column parity)
// classes whose gradients are GEMMs over 1, 2, 2 and 4 taps of K channels each: 9/4 taps per pixel instead of the 9 a stride-1
// kernel spends on the zero-stuffed dy.  ONE launch covers the four classes: blockIdx.x walks the 128-pixel tiles of class 0, then
// of class 1, ...; blockIdx.y the BN-channel tiles of C.  A block reduces over (row tap, column tap, 32-channel chunk of K) in that
// fixed order on v_mfma_f32_32x32x2_f32 (exact fp32 fma chain), so two launches give the same bits; every dx element belongs to one
// class, one pixel tile and one channel tile, so it is written exactly once.  Taps with ho == Ho or wo == Wo (the last odd row /
// column of an even-sized map) do not exist: their rows are staged as zeros.
//
// Staging follows the implicit GEMM of seam_conv.hip: both operands go to LDS as rows of one 128-byte k-chunk (+16 bytes of padding:
// the 16-byte fragment reads of 32 consecutive rows then spread over all banks), each lane reads 4 consecutive k of its row per
// k-slot, and the global loads of chunk q+1 are in flight while the MFMAs of chunk q run.
#include <hip/hip_runtime.h>
#include "seam_device.h"
#include <stdint.h>

namespace {

constexpr int S2_BM = 128;             // pixels (of one parity class) per block: 4 waves x 32 rows
constexpr int S2_LDB = 128 + 16;       // LDS row: 32 floats of k + padding (bytes)

struct S2Args {
    const float* dy;
    const float* wp;
    const float* mask;
    float* dx;
    int N, H, W, C, Ho, Wo, K;
    int Hc0, Hc1, Wc0, Wc1;            // rows / columns of each parity
    int t1, t2, t3;                    // first pixel tile of classes 1, 2, 3 (class = row parity * 2 + column parity)
};

template <int BN>
__global__ __launch_bounds__(256) void conv3x3s2_dgrad_kernel(const S2Args p) {
    constexpr int NT = BN / 32;        // 32x32 accumulators per wave = 16-byte weight loads per thread and chunk
    __shared__ __attribute__((aligned(16))) char As[S2_BM * S2_LDB];
    __shared__ __attribute__((aligned(16))) char Bs[BN * S2_LDB];
    __shared__ long long rowoff[S2_BM];                 // element offset of the tile's pixels in dx (-1: past the class)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = tid >> 6;
    const int lcol = tid & 7;          // which 16-byte vector of the chunk
    const int lrow = tid >> 3;         // 0..31

    const int bx = (int)blockIdx.x;
    const int cls = bx >= p.t3 ? 3 : (bx >= p.t2 ? 2 : (bx >= p.t1 ? 1 : 0));
    const int ph = cls >> 1, pw = cls & 1;
    const int Hc = ph ? p.Hc1 : p.Hc0, Wc = pw ? p.Wc1 : p.Wc0;
    const int Mc = p.N * Hc * Wc;
    const int m0 = (bx - (cls == 3 ? p.t3 : (cls == 2 ? p.t2 : (cls == 1 ? p.t1 : 0)))) * S2_BM;
    const int c0 = (int)blockIdx.y * BN;
    const int HWc = Hc * Wc;

    // this thread's four staged pixel rows: offset of dy[n, i, j, lcol*4] and whether the taps at i+1 / j+1 exist
    int abase[4];
    bool aok[4], ah1[4], aw1[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + lrow + 32 * i;
        aok[i] = m < Mc;
        const int mm = aok[i] ? m : 0;
        const int n = mm / HWc;
        const int rm = mm - n * HWc;
        const int ii = rm / Wc;
        const int jj = rm - ii * Wc;
        abase[i] = ((n * p.Ho + ii) * p.Wo + jj) * p.K + lcol * 4;
        ah1[i] = ii + 1 < p.Ho;
        aw1[i] = jj + 1 < p.Wo;
    }
    if (tid < S2_BM) {
        const int m = m0 + tid;
        long long off = -1;
        if (m < Mc) {
            const int n = m / HWc;
            const int rm = m - n * HWc;
            const int ii = rm / Wc;
            const int jj = rm - ii * Wc;
            off = (((long long)n * p.H + (2 * ii + ph)) * p.W + (2 * jj + pw)) * p.C;
        }
        rowoff[tid] = off;
    }

    const int nkc = p.K >> 5;
    const int nts = 1 + pw;
    const int nq = (1 + ph) * nts * nkc;          // chunks: (row tap, column tap, k-chunk), k-chunk fastest

    f32x4 areg[4], breg[NT];
    auto load_chunk = [&](int q) {
        const int tap = q / nkc;
        const int kc = q - tap * nkc;
        const int tr = tap / nts;
        const int ts = tap - tr * nts;
        const int r = ph ? (tr ? 2 : 0) : 1;
        const int s = pw ? (ts ? 2 : 0) : 1;
        const bool dh = ph && tr == 0;             // the tap reads ho = i + 1
        const bool dw = pw && ts == 0;             // ... wo = j + 1
        const int toff = ((dh ? p.Wo : 0) + (dw ? 1 : 0)) * p.K + kc * 32;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool ok = aok[i] && (!dh || ah1[i]) && (!dw || aw1[i]);
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (ok) v = *reinterpret_cast<const f32x4*>(p.dy + abase[i] + toff);
            areg[i] = v;
        }
        const float* wt = p.wp + ((size_t)(r * 3 + s) * p.C + c0) * p.K + kc * 32 + lcol * 4;
#pragma unroll
        for (int i = 0; i < NT; ++i) breg[i] = *reinterpret_cast<const f32x4*>(wt + (size_t)(lrow + 32 * i) * p.K);
    };

    f32x16 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    const int aoff = (wid * 32 + (lane & 31)) * S2_LDB + (lane >> 5) * 16;
    const int boff = (lane & 31) * S2_LDB + (lane >> 5) * 16;

    load_chunk(0);
    for (int q = 0; q < nq; ++q) {
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(&As[(lrow + 32 * i) * S2_LDB + lcol * 16]) = areg[i];
#pragma unroll
        for (int i = 0; i < NT; ++i) *reinterpret_cast<f32x4*>(&Bs[(lrow + 32 * i) * S2_LDB + lcol * 16]) = breg[i];
        __syncthreads();
        if (q + 1 < nq) load_chunk(q + 1);         // in flight under this chunk's MFMAs
#pragma unroll
        for (int k8 = 0; k8 < 4; ++k8) {
            const f32x4 fa = *reinterpret_cast<const f32x4*>(&As[aoff + k8 * 32]);
            f32x4 fb[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) fb[j] = *reinterpret_cast<const f32x4*>(&Bs[boff + j * 32 * S2_LDB + k8 * 32]);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[kk], fb[j][kk], acc[j], 0, 0, 0);
        }
        __syncthreads();
    }

    // epilogue: lane = channel (lane & 31) of 16 pixel rows; 32 lanes write 128 consecutive bytes of one pixel
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const long long off = rowoff[wid * 32 + row];
        if (off < 0) continue;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const long long e = off + c0 + j * 32 + (lane & 31);
            float v = acc[j][r];
            if (p.mask) v = p.mask[e] > 0.f ? v : 0.f;
            p.dx[e] = v;
        }
    }
}

__global__ __launch_bounds__(256) void pack_s2_dgrad_kernel(const float* __restrict__ w, const float* __restrict__ scale,
                                                            float* __restrict__ wp, int K, int C) {
    const size_t total = (size_t)9 * C * K;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int k = (int)(i % K);
        const size_t r = i / K;
        const int c = (int)(r % C);
        const int t = (int)(r / C);
        const float v = w[((size_t)k * C + c) * 9 + t];
        wp[i] = scale ? v * scale[k] : v;
    }
}

__global__ __launch_bounds__(256) void relu_mask_add_kernel(const f32x4* __restrict__ y, const f32x4* __restrict__ a,
                                                            const f32x4* __restrict__ b, f32x4* __restrict__ out, size_t total) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const f32x4 m = y[i];
        f32x4 v = a[i];
        if (b) v += b[i];
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = m[e] > 0.f ? v[e] : 0.f;
        out[i] = o;
    }
}

// The adjoint of max-pool(3, 2, 1) behind a ReLU, gather form.  Window ph covers the rows 2ph-1 .. 2ph+1, so the 2 x 2 pixels
// (2a + {0,1}, 2b + {0,1}) lie in the windows (a + {0,1}, b + {0,1}) and in no other: a lane owns those four pixels of 4 channels.
// It reads the 5 x 5 cells (2a-1 .. 2a+3) x (2b-1 .. 2b+3) once, scans them in row-major order and keeps per window the first
// maximum among the POSITIVE cells (strict > to replace, starting from 0) -- torch's argmax wherever it matters: a pixel with
// y > 0 is the first maximum of a window exactly when it is the first maximum of the window's positive cells, and a pixel with
// y <= 0 gets a zero from the ReLU mask whatever the pool gave it.  Cells outside the image are read as 0 (a buffer load past the
// descriptor's range), so they take no part.  Each pixel then takes the dpool of the windows whose argmax it is, added in ascending
// (ph, pw) order onto 0, and is zeroed where y <= 0.
// 25 loads of y per 4 outputs (6.25 per pixel, where a pixel-per-lane gather re-reads 16); no LDS: the overlap between
// neighbouring patches -- columns inside a block, rows between the blocks of two pooled rows -- is served by L1 / L2.
// A block is (n * Ho + a) * nchunks + chunk; a chunk is 256 lanes of one pooled row, lane = (b, 16-byte channel vector).  Blocks
// are dealt round-robin over the 8 XCDs, so blockIdx.x is remapped (a bijection, for speed only) to give each XCD one contiguous
// run of pooled rows: the three y rows two neighbouring pooled rows share then meet in one L2 instead of being fetched by two.
struct PoolBwdArgs {
    const float* y;
    const float* dpool;
    float* dy;
    int N, H, W, C, Ho, Wo, cv, nchunks, nblocks;
};

__global__ __launch_bounds__(256) void maxpool3s2_relu_bwd_kernel(const PoolBwdArgs p) {
    const int xcd = (int)(blockIdx.x & 7u), per = p.nblocks >> 3, rem = p.nblocks & 7;
    const int bid = xcd * per + min(xcd, rem) + (int)(blockIdx.x >> 3);
    const int row = bid / p.nchunks;                                   // n * Ho + a
    const int j = (bid - row * p.nchunks) * 256 + (int)threadIdx.x;
    if (j >= p.Wo * p.cv) return;
    const int n = row / p.Ho, a = row - n * p.Ho;
    const int b = j / p.cv, c = (j - b * p.cv) * 4;
    const int h0 = 2 * a - 1, w0 = 2 * b - 1;
    // y of the whole launch is below 2^31 bytes (checked by the launcher): 32-bit byte offsets, 0x80000000 = out of range = 0.0f
    const __amdgpu_buffer_rsrc_t y_rsrc =
        __builtin_amdgcn_make_buffer_rsrc((void*)p.y, 0, (int)((unsigned)p.N * p.H * p.W * p.C * 4u), 0x00020000);

    f32x4 m[4];                        // running maximum of window (a + (q >> 1), b + (q & 1)) over its positive cells
    int am[4][4];                      // ... and the cell r * 5 + s that holds it, per channel (-1: no positive cell)
    f32x4 own[4];                      // y at the lane's pixels: cells (1,1) (1,2) (2,1) (2,2)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        m[q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) am[q][e] = -1;
    }
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        const int hi = h0 + r;
        const bool rok = (unsigned)hi < (unsigned)p.H;
        const int rbase = ((n * p.H + hi) * p.W + w0) * p.C + c;
#pragma unroll
        for (int s = 0; s < 5; ++s) {
            const bool ok = rok && (unsigned)(w0 + s) < (unsigned)p.W;
            const unsigned off = ok ? (unsigned)(rbase + s * p.C) * 4u : 0x80000000u;
            const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(y_rsrc, off, 0, 0));
            if ((r == 1 || r == 2) && (s == 1 || s == 2)) own[(r - 1) * 2 + (s - 1)] = v;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bool in = ((q >> 1) ? r >= 2 : r <= 2) && ((q & 1) ? s >= 2 : s <= 2);
                if (!in) continue;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    am[q][e] = v[e] > m[q][e] ? r * 5 + s : am[q][e];
                    m[q][e] = fmaxf(m[q][e], v[e]);
                }
            }
        }
    }

    const bool a1 = a + 1 < p.Ho, b1 = b + 1 < p.Wo;                 // the windows below / right of (a, b) exist
    const float* dpn = p.dpool + (((size_t)n * p.Ho + a) * p.Wo + b) * p.C + c;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 dp[4];
    dp[0] = *reinterpret_cast<const f32x4*>(dpn);
    dp[1] = b1 ? *reinterpret_cast<const f32x4*>(dpn + p.C) : zero;
    dp[2] = a1 ? *reinterpret_cast<const f32x4*>(dpn + (size_t)p.Wo * p.C) : zero;
    dp[3] = (a1 && b1) ? *reinterpret_cast<const f32x4*>(dpn + ((size_t)p.Wo + 1) * p.C) : zero;

    float* dyn = p.dy + (size_t)n * p.H * p.W * p.C + c;
#pragma unroll
    for (int o = 0; o < 4; ++o) {      // pixel (2a + (o >> 1), 2b + (o & 1)) = cell (1 + (o >> 1), 1 + (o & 1))
        const int hi = 2 * a + (o >> 1), wi = 2 * b + (o & 1);
        if (hi >= p.H || wi >= p.W) continue;
        const int id = (1 + (o >> 1)) * 5 + 1 + (o & 1);
        f32x4 g = zero;
#pragma unroll
        for (int q = 0; q < 4; ++q) {  // ascending (ph, pw); a pixel on an even row / column is in no window q with that bit set
            if (((q >> 1) && !(o >> 1)) || ((q & 1) && !(o & 1))) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                g[e] += am[q][e] == id ? dp[q][e] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) g[e] = own[o][e] > 0.f ? g[e] : 0.f;
        *reinterpret_cast<f32x4*>(dyn + ((size_t)hi * p.W + wi) * p.C) = g;
    }
}

inline unsigned grid_for(size_t total) { return (unsigned)((total + 255) / 256 > 65535 * 16 ? 65535 * 16 : (total + 255) / 256); }

}  // namespace

extern "C" {

int seam_pack_conv3x3s2_dgrad_f32(const float* w, const float* scale, float* w_packed, int K, int C, void* stream) {
    if (K <= 0 || C <= 0 || (K % 32) || (C % 32) || !w || !w_packed) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(pack_s2_dgrad_kernel, dim3(grid_for((size_t)9 * C * K)), dim3(256), 0, (hipStream_t)stream, w, scale,
                       w_packed, K, C);
    return (int)hipGetLastError();
}

int seam_conv3x3s2_dgrad_f32(const float* dy, const float* w_packed, const float* mask, float* dx, int N, int H, int W, int C, int K,
                             void* stream) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || K <= 0 || (C % 32) || (K % 32) || !dy || !w_packed || !dx)
        return (int)hipErrorInvalidValue;
    S2Args a;
    a.dy = dy; a.wp = w_packed; a.mask = mask; a.dx = dx;
    a.N = N; a.H = H; a.W = W; a.C = C; a.K = K;
    a.Ho = (H - 1) / 2 + 1;
    a.Wo = (W - 1) / 2 + 1;
    if ((double)N * H * W * C * 4 >= 2147483648.0 || (double)N * a.Ho * a.Wo * K * 4 >= 2147483648.0) return (int)hipErrorInvalidValue;
    a.Hc0 = (H + 1) / 2; a.Hc1 = H / 2;
    a.Wc0 = (W + 1) / 2; a.Wc1 = W / 2;
    const int hc[2] = {a.Hc0, a.Hc1}, wc[2] = {a.Wc0, a.Wc1};
    int first[5] = {0, 0, 0, 0, 0};
    for (int cls = 0; cls < 4; ++cls) {
        const long long mc = (long long)N * hc[cls >> 1] * wc[cls & 1];
        first[cls + 1] = first[cls] + (int)((mc + S2_BM - 1) / S2_BM);
    }
    a.t1 = first[1]; a.t2 = first[2]; a.t3 = first[3];
    const int bn = (C % 128 == 0) ? 128 : ((C % 64 == 0) ? 64 : 32);
    const dim3 grid(first[4], C / bn);
    if (bn == 128) hipLaunchKernelGGL(conv3x3s2_dgrad_kernel<128>, grid, dim3(256), 0, (hipStream_t)stream, a);
    else if (bn == 64) hipLaunchKernelGGL(conv3x3s2_dgrad_kernel<64>, grid, dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(conv3x3s2_dgrad_kernel<32>, grid, dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int seam_relu_mask_add_f32(const float* y, const float* a, const float* b, float* out, int64_t M, int C, void* stream) {
    if (M <= 0 || C <= 0 || (C & 3) || !y || !a || !out) return (int)hipErrorInvalidValue;
    const size_t total = (size_t)M * (size_t)(C >> 2);
    hipLaunchKernelGGL(relu_mask_add_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const f32x4*>(y), reinterpret_cast<const f32x4*>(a), reinterpret_cast<const f32x4*>(b),
                       reinterpret_cast<f32x4*>(out), total);
    return (int)hipGetLastError();
}

int seam_maxpool3s2_relu_bwd_f32(const float* y, const float* dpool, float* dy, int N, int H, int W, int C, void* stream) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 3) || !y || !dpool || !dy) return (int)hipErrorInvalidValue;
    if ((double)N * H * W * C * 4 >= 2147483648.0) return (int)hipErrorInvalidValue;      // dpool is never the larger one
    PoolBwdArgs a;
    a.y = y; a.dpool = dpool; a.dy = dy;
    a.N = N; a.H = H; a.W = W; a.C = C;
    a.Ho = (H - 1) / 2 + 1;
    a.Wo = (W - 1) / 2 + 1;
    a.cv = C >> 2;
    a.nchunks = (a.Wo * a.cv + 255) / 256;
    const long long blocks = (long long)N * a.Ho * a.nchunks;         // < 2^31: at most one block per 16 bytes of y
    a.nblocks = (int)blocks;
    hipLaunchKernelGGL(maxpool3s2_relu_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // extern "C"
