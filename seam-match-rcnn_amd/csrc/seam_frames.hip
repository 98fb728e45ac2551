// seam_frames.hip -- the step in front of the path: what MovingFashionDataset.__getitem__ does to a
// decoded video frame on the CPU (ref datasets/MFDataset.py:79-93) as device kernels on the uint8 frame:
//   BGR -> RGB, additive Gaussian noise in [0,1] units (float64, as NumPy computes it), clip, truncate to uint8,
//   then PIL's Image.resize to half resolution.  Image.resize defaults to BICUBIC with an antialiasing support scaled
//   by the reduction factor and 8-bit fixed-point coefficients (Pillow src/libImaging/Resample.c: precompute_coeffs,
//   normalize_coeffs_8bpc, ImagingResampleHorizontal/Vertical_8bpc); the kernels below restate that arithmetic
//   operation for operation (float64 coefficient maths with contraction off, 22-bit fixed point, horizontal pass
//   rounded to uint8 before the vertical pass) so the result is bit-identical to Pillow's.
// ToTensor (/255) and GeneralizedRCNNTransform are fused further down the line in seam_preprocess_u8.
#include <hip/hip_runtime.h>
#include "seam_launch.h"
#include <stdint.h>

#pragma STDC FP_CONTRACT OFF

namespace {

constexpr int KMAX = 24;               // taps per output sample: 2*ceil(2*scale)+1  (scale <= 5.5)
constexpr int PRECISION_BITS = 32 - 8 - 2;

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// standard normal draw number i of the stream `seed`: counter-based Box-Muller on two splitmix64 hashes
__device__ __forceinline__ double normal_draw(uint64_t seed, size_t i) {
    const uint64_t r0 = splitmix64(seed ^ (i * 2 + 1)), r1 = splitmix64(seed ^ (i * 2 + 2) ^ 0xD1B54A32D192ED03ull);
    const double u0 = ((double)(r0 >> 11) + 1.0) * (1.0 / 9007199254740993.0);    // (0,1)
    const double u1 = (double)(r1 >> 11) * (1.0 / 9007199254740992.0);
    return sqrt(-2.0 * log(u0)) * cos(6.283185307179586 * u1);
}

// uint8(clip((v / 255.0 + n * sigma) * 255.0, 0, 255)) step by step as NumPy evaluates it (contraction is off in this file)
__device__ __forceinline__ uint8_t noisy_byte(uint8_t v, double n, double sigma) {
    double x = (double)v / 255.0;
    x = x + n * sigma;
    x = x * 255.0;
    x = x < 0.0 ? 0.0 : (x > 255.0 ? 255.0 : x);
    return (uint8_t)x;
}

// out[y][x][c] = noisy_byte(in[y][x][2-c], n, sigma)     (ref MFDataset.py:81-88)
// n = noise[y][x][c] (float64 standard normal draws, e.g. np.random.randn) or, when noise == NULL, normal_draw(seed, element
// index).  sigma == 0 and noise == NULL: plain channel flip.
__global__ void frame_noise_kernel(const uint8_t* __restrict__ in, const double* __restrict__ noise, uint8_t* __restrict__ out,
                                   size_t n_elem, double sigma, uint64_t seed) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_elem; i += (size_t)gridDim.x * blockDim.x) {
        const size_t px = i / 3;
        const int c = (int)(i - px * 3);
        const uint8_t v = in[px * 3 + (2 - c)];
        if (sigma == 0.0 && noise == nullptr) { out[i] = v; continue; }
        out[i] = noisy_byte(v, noise ? noise[i] : normal_draw(seed, i), sigma);
    }
}

// The noise of MultiDeepFashion2Dataset.__getitem__ (ref MultiDF2Dataset.py:157-167) on a staged batch, in place: grid (element
// blocks, images); byte e of image `img` (RGB order, unflipped) becomes noisy_byte(v, n, sigma[img]) with
// n = draws[draws_off[img] + e] or, draws == NULL, normal_draw(seed[img], e).  An image with sigma 0 is not touched, nor is one
// whose table entry does not lie inside the buffer (the buffer half of preprocess_u8_batch_kernel's `ok`, which then writes that
// image as zeros).  Images start at any byte and rows have odd lengths: one byte load and one byte store per element.
__global__ void noise_u8_batch_kernel(uint8_t* __restrict__ buf, int64_t buf_bytes, const int64_t* __restrict__ img_off,
                                      const int* __restrict__ img_dims, const double* __restrict__ sigma,
                                      const uint64_t* __restrict__ seed, const double* __restrict__ draws,
                                      const int64_t* __restrict__ draws_off) {
    const int img = blockIdx.y;
    const double s = sigma[img];
    if (s == 0.0) return;
    const int64_t in_h = img_dims[5 * img], in_w = img_dims[5 * img + 1], off = img_off[img];
    if (in_h <= 0 || in_w <= 0 || off < 0 || off > buf_bytes || in_h * in_w > (buf_bytes - off) / 3) return;
    const size_t n_elem = (size_t)(in_h * in_w) * 3;
    uint8_t* p = buf + off;
    const double* d = draws ? draws + draws_off[img] : nullptr;
    const uint64_t sd = seed[img];
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_elem; e += (size_t)gridDim.x * blockDim.x)
        p[e] = noisy_byte(p[e], d ? d[e] : normal_draw(sd, e), s);
}

__device__ __forceinline__ double bicubic_filter(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// Pillow's precompute_coeffs + normalize_coeffs_8bpc for output sample xx of one axis: the first input sample, the number of taps
// and kk[NT] fixed-point weights (zero from the tap count on).  NT >= the tap count: the weights do not depend on NT, since taps
// past the count add nothing to the sum they are normalised by.  The one definition, for the per-frame table kernel below
// (NT = KMAX) and for the fused batch kernel (NT = FK).
template <int NT>
__device__ __forceinline__ void resize_coeffs(int inSize, int outSize, int xx, int& first, int& count, int* __restrict__ kk) {
    const float in0 = 0.f, in1 = (float)inSize;
    double scale = (double)(in1 - in0) / outSize;
    double filterscale = scale;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = 2.0 * filterscale;
    const double center = in0 + (xx + 0.5) * scale;
    const double ss = 1.0 / filterscale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > inSize) xmax = inSize;
    xmax -= xmin;
    double k[NT];
    double ww = 0.0;
    for (int x = 0; x < NT; ++x) {
        double w = 0.0;
        if (x < xmax) {
            w = bicubic_filter((x + xmin - center + 0.5) * ss);
            ww += w;
        }
        k[x] = w;
    }
    for (int x = 0; x < NT; ++x) {
        double v = k[x];
        if (x < xmax && ww != 0.0) v /= ww;
        kk[x] = v < 0 ? (int)(-0.5 + v * (1 << PRECISION_BITS)) : (int)(0.5 + v * (1 << PRECISION_BITS));
    }
    first = xmin;
    count = xmax;
}

// one axis' tables for seam_resize_bicubic_u8: bounds[xx] = (xmin, count), kk[xx][KMAX]
__global__ void resize_coeff_kernel(int inSize, int outSize, int* __restrict__ bounds, int* __restrict__ kk) {
    const int xx = blockIdx.x * blockDim.x + threadIdx.x;
    if (xx >= outSize) return;
    resize_coeffs<KMAX>(inSize, outSize, xx, bounds[2 * xx], bounds[2 * xx + 1], kk + (size_t)xx * KMAX);
}

__device__ __forceinline__ uint8_t clip8(int v) {
    v >>= PRECISION_BITS;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// one resampling pass over an interleaved uint8 image [H][W][3]; axis 0: along x (out [H][OW][3]), axis 1: along y
__global__ void resize_pass_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int H, int W, int OH, int OW,
                                   const int* __restrict__ bounds, const int* __restrict__ kk, int axis) {
    const size_t total = (size_t)OH * OW * 3;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % 3);
        const int x = (int)((i / 3) % OW);
        const int y = (int)(i / ((size_t)3 * OW));
        const int o = axis == 0 ? x : y;
        const int lo = bounds[2 * o], cnt = bounds[2 * o + 1];
        const int* k = kk + (size_t)o * KMAX;
        int ss = 1 << (PRECISION_BITS - 1);
        if (axis == 0) {
            const uint8_t* row = in + ((size_t)y * W + lo) * 3 + c;
            for (int t = 0; t < cnt; ++t) ss += (int)row[(size_t)t * 3] * k[t];
        } else {
            const uint8_t* col = in + ((size_t)lo * W + x) * 3 + c;
            for (int t = 0; t < cnt; ++t) ss += (int)col[(size_t)t * W * 3] * k[t];
        }
        out[i] = clip8(ss);
    }
}

// ------------------------------------------------------------------------------------------------ the fused batch kernel
// The per-frame work of MovingFashionDataset.__getitem__ for N images of different sizes in one launch: grid (tiles, images).
//   mode 0  bytes copied (the shop image, the zero placeholder)        mode 1  BGR -> RGB (noise=False)
//   mode 2  BGR -> RGB, noise, Pillow's resize to (h / 2, w / 2): a block makes one FT x FT tile of the half-size image.
// Halving has scale s = in / (in / 2) in [2, 3] and support 2 s, so an output sample has at most 4 s + 1 <= 13 taps (FK = 16) and
// the n <= FT samples of a tile read at most (n + 3) s + 1 input samples: at most 2 FT + 1 when the whole axis is one tile
// (n = in / 2), at most 67 (2 + 1 / 64) + 1 < 137 otherwise -- FWIN = 2 FT + 16 covers both.  The window is walked in chunks of
// FCH rows: noisy RGB bytes of the chunk into LDS (every draw keyed by its element index in the full frame: a halo sample gets
// the draw its owner gets, whatever the tiling), the horizontal pass from there into the window's half-width rows, also LDS, and
// once all rows are there the vertical pass out to memory.  LDS: 2 FT FK ints of weights + 4 FT ints of bounds + FCH FWIN 3 +
// FWIN FT 3 bytes = 43,776 bytes.
constexpr int FT = 64;
constexpr int FK = 16;
constexpr int FWIN = 2 * FT + 16;
constexpr int FCH = 16;

__global__ __launch_bounds__(256) void frames_prepare_batch_kernel(
        const uint8_t* __restrict__ in, int64_t in_bytes, const int64_t* __restrict__ in_off, const int* __restrict__ dims,
        const double* __restrict__ sigma, const uint64_t* __restrict__ seed, const double* __restrict__ draws,
        const int64_t* __restrict__ draws_off, int64_t draws_len, uint8_t* __restrict__ out, int64_t out_bytes,
        const int64_t* __restrict__ out_off, int max_h, int max_w) {
    __shared__ int s_kx[FT * FK], s_ky[FT * FK], s_bx[2 * FT], s_by[2 * FT];
    __shared__ uint8_t s_rgb[FCH * FWIN * 3], s_h[FWIN * FT * 3];
    const int img = blockIdx.y, tid = threadIdx.x;
    const int64_t H = dims[3 * img], W = dims[3 * img + 1];
    const int mode = dims[3 * img + 2];
    const int64_t ioff = in_off[img], ooff = out_off[img];
    // an entry that does not lie inside both buffers, or that the grid was not sized for, is never touched
    if (H <= 0 || W <= 0 || H > max_h || W > max_w || mode < 0 || mode > 2 || (mode == 2 && (H < 2 || W < 2))) return;
    if (ioff < 0 || ioff > in_bytes || H * W > (in_bytes - ioff) / 3) return;
    const int OH = mode == 2 ? (int)(H / 2) : (int)H, OW = mode == 2 ? (int)(W / 2) : (int)W;
    if (ooff < 0 || ooff > out_bytes || (int64_t)OH * OW > (out_bytes - ooff) / 3) return;
    const uint8_t* src = in + ioff;
    uint8_t* dst = out + ooff;
    if (mode != 2) {
        const size_t n_elem = (size_t)(H * W) * 3;
        for (size_t e = (size_t)blockIdx.x * 256 + tid; e < n_elem; e += (size_t)gridDim.x * 256) {
            const size_t px = e / 3;
            dst[e] = mode == 0 ? src[e] : src[px * 3 + (2 - (int)(e - px * 3))];
        }
        return;
    }
    const double* d = nullptr;
    if (draws) {
        const int64_t doff = draws_off[img];
        if (doff < 0 || doff > draws_len || H * W > (draws_len - doff) / 3) return;
        d = draws + doff;
    }
    const int tiles_x = (OW + FT - 1) / FT, tiles_y = (OH + FT - 1) / FT;
    if (blockIdx.x >= (unsigned)(tiles_x * tiles_y)) return;
    const int ox0 = (int)(blockIdx.x % tiles_x) * FT, oy0 = (int)(blockIdx.x / tiles_x) * FT;
    const int nx = OW - ox0 < FT ? OW - ox0 : FT, ny = OH - oy0 < FT ? OH - oy0 : FT;
    if (tid < nx) resize_coeffs<FK>((int)W, OW, ox0 + tid, s_bx[2 * tid], s_bx[2 * tid + 1], s_kx + tid * FK);
    else if (tid >= FT && tid - FT < ny)
        resize_coeffs<FK>((int)H, OH, oy0 + tid - FT, s_by[2 * (tid - FT)], s_by[2 * (tid - FT) + 1], s_ky + (tid - FT) * FK);
    __syncthreads();
    const int xlo = s_bx[0], win_w = s_bx[2 * (nx - 1)] + s_bx[2 * (nx - 1) + 1] - xlo;
    const int ylo = s_by[0], win_h = s_by[2 * (ny - 1)] + s_by[2 * (ny - 1) + 1] - ylo;
    if (win_w > FWIN || win_h > FWIN) return;       // cannot happen for a halving (above); the same in every thread of the block
    const double s = sigma[img];
    const uint64_t sd = seed[img];
    const bool plain = s == 0.0 && d == nullptr;    // frame_noise_kernel's rule: the channel flip alone
    const int row_len = win_w * 3, out_len = nx * 3;
    for (int r0 = 0; r0 < win_h; r0 += FCH) {
        const int rows = win_h - r0 < FCH ? win_h - r0 : FCH;
        for (int e = tid; e < rows * row_len; e += 256) {
            const int r = e / row_len, j = e - r * row_len, px = j / 3, c = j - px * 3;
            const size_t at = ((size_t)(ylo + r0 + r) * W + (xlo + px)) * 3;
            const uint8_t v = src[at + (2 - c)];
            s_rgb[e] = plain ? v : noisy_byte(v, d ? d[at + c] : normal_draw(sd, at + c), s);
        }
        __syncthreads();
        for (int e = tid; e < rows * out_len; e += 256) {
            const int r = e / out_len, j = e - r * out_len, x = j / 3, c = j - x * 3;
            const int cnt = s_bx[2 * x + 1];
            const int* k = s_kx + x * FK;
            const uint8_t* p = s_rgb + r * row_len + (s_bx[2 * x] - xlo) * 3 + c;
            int ss = 1 << (PRECISION_BITS - 1);
            for (int t = 0; t < cnt; ++t) ss += (int)p[3 * t] * k[t];
            s_h[((r0 + r) * FT + x) * 3 + c] = clip8(ss);
        }
        __syncthreads();
    }
    for (int e = tid; e < ny * out_len; e += 256) {
        const int y = e / out_len, j = e - y * out_len, x = j / 3, c = j - x * 3;
        const int cnt = s_by[2 * y + 1];
        const int* k = s_ky + y * FK;
        const uint8_t* p = s_h + ((s_by[2 * y] - ylo) * FT + x) * 3 + c;
        int ss = 1 << (PRECISION_BITS - 1);
        for (int t = 0; t < cnt; ++t) ss += (int)p[t * FT * 3] * k[t];
        dst[((size_t)(oy0 + y) * OW + (ox0 + x)) * 3 + c] = clip8(ss);
    }
}

inline int taps_needed(int inSize, int outSize) {
    double fs = (double)inSize / outSize;
    if (fs < 1.0) fs = 1.0;
    const double support = 2.0 * fs;
    int c = (int)support;
    if ((double)c < support) ++c;
    return c * 2 + 1;
}

}  // namespace

extern "C" {

int seam_frame_noise_u8(const uint8_t* bgr, const double* noise, uint8_t* rgb, int H, int W, double sigma, uint64_t seed,
                        void* stream) {
    const size_t n = (size_t)H * W * 3;
    if (n == 0) return 0;
    const unsigned grid = seam_launch::grid256(n, 8192);
    hipLaunchKernelGGL(frame_noise_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, bgr, noise, rgb, n, sigma, seed);
    return (int)hipGetLastError();
}

int seam_noise_u8_batch(uint8_t* buf, int64_t buf_bytes, const int64_t* img_off, const int* img_dims, const double* sigma,
                        const uint64_t* seed, const double* draws, const int64_t* draws_off, int n_images, void* stream) {
    if (n_images < 1 || n_images > 65535 || buf_bytes < 0) return (int)hipErrorInvalidValue;
    if (!buf || !img_off || !img_dims || !sigma || !seed || (draws && !draws_off)) return (int)hipErrorInvalidValue;
    // the image sizes are on the device: no image is larger than the buffer, and about 16k blocks in all keep every CU busy
    // when three images in four exit at once
    const unsigned cap = 16384u / (unsigned)n_images;
    const dim3 grid(seam_launch::grid256((size_t)buf_bytes, cap < 32 ? 32 : cap), (unsigned)n_images);
    if (grid.x == 0) return 0;
    hipLaunchKernelGGL(noise_u8_batch_kernel, grid, dim3(256), 0, (hipStream_t)stream, buf, buf_bytes, img_off, img_dims, sigma,
                       seed, draws, draws_off);
    return (int)hipGetLastError();
}

int seam_frames_prepare_batch_u8(const uint8_t* in, int64_t in_bytes, const int64_t* in_off, const int* dims, const double* sigma,
                                 const uint64_t* seed, const double* draws, const int64_t* draws_off, int64_t draws_len,
                                 uint8_t* out, int64_t out_bytes, const int64_t* out_off, int n_images, int max_h, int max_w,
                                 void* stream) {
    if (n_images < 1 || n_images > 65535 || in_bytes < 0 || out_bytes < 0 || draws_len < 0 || max_h < 1 || max_w < 1)
        return (int)hipErrorInvalidValue;
    if (!in || !out || !in_off || !out_off || !dims || !sigma || !seed || (draws && !draws_off)) return (int)hipErrorInvalidValue;
    // the image sizes are on the device; the caller's largest height and width size the grid: one block per tile of the largest
    // half-size image, and an image beyond them is skipped as a bad entry is.  Copies (modes 0 and 1) stride over these blocks.
    const int64_t tiles = (int64_t)((max_h / 2 + FT - 1) / FT) * ((max_w / 2 + FT - 1) / FT);
    if (tiles > 0x7FFFFFFF) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)(tiles < 1 ? 1 : tiles), (unsigned)n_images);
    hipLaunchKernelGGL(frames_prepare_batch_kernel, grid, dim3(256), 0, (hipStream_t)stream, in, in_bytes, in_off, dims, sigma, seed,
                       draws, draws_off, draws_len, out, out_bytes, out_off, max_h, max_w);
    return (int)hipGetLastError();
}

// bytes of scratch for seam_resize_bicubic_u8: coefficient tables of both axes + the horizontally resampled image
int64_t seam_resize_workspace_bytes(int H, int W, int OH, int OW) {
    return (int64_t)(OW + OH) * (KMAX + 2) * 4 + (int64_t)H * OW * 3 + 64;
}

int seam_resize_bicubic_u8(const uint8_t* in, uint8_t* out, int H, int W, int OH, int OW, void* ws, void* stream) {
    if (H <= 0 || W <= 0 || OH <= 0 || OW <= 0) return (int)hipErrorInvalidValue;
    if (taps_needed(W, OW) > KMAX || taps_needed(H, OH) > KMAX) return (int)hipErrorInvalidValue;
    int* bx = (int*)ws;
    int* kx = bx + 2 * OW;
    int* by = kx + (size_t)OW * KMAX;
    int* ky = by + 2 * OH;
    uint8_t* tmp = (uint8_t*)(ky + (size_t)OH * KMAX);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(resize_coeff_kernel, dim3((OW + 255) / 256), dim3(256), 0, s, W, OW, bx, kx);
    hipLaunchKernelGGL(resize_coeff_kernel, dim3((OH + 255) / 256), dim3(256), 0, s, H, OH, by, ky);
    auto grid = [](size_t n) { size_t g = (n + 255) / 256; return dim3((unsigned)(g > 16384 ? 16384 : g)); };
    // Pillow resamples horizontally first (ImagingResample), rounding to uint8 between the passes
    hipLaunchKernelGGL(resize_pass_kernel, grid((size_t)H * OW * 3), dim3(256), 0, s, in, tmp, H, W, H, OW, bx, kx, 0);
    hipLaunchKernelGGL(resize_pass_kernel, grid((size_t)OH * OW * 3), dim3(256), 0, s, tmp, out, H, OW, OH, OW, by, ky, 1);
    return (int)hipGetLastError();
}

}  // extern "C"
