// seam_pack_items.h -- one output item of every fp32 weight-pack form, as a device function of (source, destination, dimensions,
// item index).  The per-layer pack kernels (seam_conv.hip, seam_wino.hip, seam_wino24.hip, seam_pwpc.hip, seam_narrow.hip) and the
// table-driven seam_repack_many_f32 (seam_optim.hip) run the same function over the same index range, so the two routes write the
// same bytes.  The layouts are described at the kernels that read them.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "seam_device.h"
#include "seam_split.h"

namespace seam_pack {

// Value of item i of the tile-contiguous implicit-GEMM pack [rows/bn][kred/BKE][bn][BKE] (BKE elements per 128-byte chunk) from
// OIHW fp32 [K,Cin,R,S] (mode 0), ConvTranspose2d [Cin,Cout,2,2] (mode 1) or input-gradient weights (mode 2); 0 in the padding.
template <int BKE>
__device__ __forceinline__ float igemm_value(const float* __restrict__ w, size_t i, int K, int Cin, int R, int S, int Cstore, int nk,
                                             int bn, int mode) {
    const int col = (int)(i % BKE);
    size_t rest = i / BKE;
    const int row_in = (int)(rest % bn);
    rest /= bn;
    const int q = (int)(rest % nk);
    const int tn = (int)(rest / nk);
    const int row = tn * bn + row_in;
    int r, s2, c;
    if (Cstore >= BKE) {
        const int ccn = Cstore / BKE;
        s2 = q % S;
        c = ((q / S) % ccn) * BKE + col;
        r = q / (S * ccn);
    } else {
        const int kk = q * BKE + col;
        const int pos = kk / Cstore;
        c = kk - pos * Cstore;
        r = pos / S;
        s2 = pos - r * S;
    }
    float v = 0.f;
    if (row < K && c < Cin && r < R) {
        if (mode == 0) {
            v = w[(((size_t)row * Cin + c) * R + r) * S + s2];
        } else if (mode == 2) {   // input-gradient weights of a Conv2d [Cin(out), K(in), R, S]: rotate 180, swap channels
            v = w[(((size_t)c * K + row) * R + (R - 1 - r)) * S + (S - 1 - s2)];
        } else {  // ConvTranspose2d weight [Cin, Cout, 2, 2]; row = (a*2+b)*Cout + co
            const int cout = K / 4;
            const int ab = row / cout;
            const int co = row - ab * cout;
            v = w[(((size_t)c * cout + co) * 2 + (ab >> 1)) * 2 + (ab & 1)];
        }
    }
    return v;
}

// item i of the fp32 pack -> its three bf16 planes [slab][chunk][plane][row][32 bf16] (the truncation split of split3_bf16)
__device__ __forceinline__ void split3_item(float x, unsigned short* __restrict__ out, size_t i, int slab_bn) {
    const unsigned x0 = __builtin_bit_cast(unsigned, x) & 0xffff0000u;
    const float r = x - __builtin_bit_cast(float, x0);
    const unsigned y0 = __builtin_bit_cast(unsigned, r) & 0xffff0000u;
    const float s = r - __builtin_bit_cast(float, y0);
    const size_t rowchunk = i >> 5;
    const int col = (int)(i & 31);
    const size_t slabchunk = rowchunk / (size_t)slab_bn;
    const int row = (int)(rowchunk - slabchunk * slab_bn);
    unsigned short* o = out + slabchunk * 3 * (size_t)slab_bn * 32 + (size_t)row * 32 + col;
    o[0] = (unsigned short)(x0 >> 16);
    o[(size_t)slab_bn * 32] = (unsigned short)(y0 >> 16);
    o[(size_t)slab_bn * 64] = (unsigned short)(__builtin_bit_cast(unsigned, s) >> 16);
}

// the 3x3 taps of (output n, input c) in fp64, then G g (4x3): the part the two Winograd packs share
__device__ __forceinline__ void wino_gg(const float* __restrict__ w, int n, int c, int K, int Cin, int mode, double gg[4][3]) {
    double g[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            float v = 0.f;
            if (c < Cin) v = mode == 2 ? w[(((size_t)c * K + n) * 3 + (2 - r)) * 3 + (2 - s)] : w[(((size_t)n * Cin + c) * 3 + r) * 3 + s];
            g[r][s] = (double)v;
        }
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        gg[0][s] = g[0][s];
        gg[1][s] = 0.5 * (g[0][s] + g[1][s] + g[2][s]);
        gg[2][s] = 0.5 * (g[0][s] - g[1][s] + g[2][s]);
        gg[3][s] = g[2][s];
    }
}

// F(2x2,3x3): item i = (tn, chunk, lane) of [K/32][Cstore/8][16][64][4]: 4 channels x 16 positions
__device__ __forceinline__ void wino_item(const float* __restrict__ w, float* __restrict__ out, size_t i, int K, int Cin, int nch, int mode) {
    const int lane = (int)(i & 63);
    const size_t rest = i >> 6;
    const int chunk = (int)(rest % nch);
    const int tn = (int)(rest / nch);
    const int n = tn * 32 + (lane & 31);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int c = chunk * 8 + (lane >> 5) * 4 + e;
        double gg[4][3];
        wino_gg(w, n, c, K, Cin, mode, gg);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double u0 = gg[q][0];
            const double u1 = 0.5 * (gg[q][0] + gg[q][1] + gg[q][2]);
            const double u2 = 0.5 * (gg[q][0] - gg[q][1] + gg[q][2]);
            const double u3 = gg[q][2];
            const size_t base = ((((size_t)tn * nch + chunk) * 16 + q * 4) * 64 + lane) * 4 + e;
            out[base] = (float)u0;
            out[base + 256] = (float)u1;
            out[base + 512] = (float)u2;
            out[base + 768] = (float)u3;
        }
    }
}

// one row of (G g) times G4t: the six F(4,3) weight points of F(2x4,3x3), in fp64
__device__ __forceinline__ void wino24_g4(double a0, double a1, double a2, double uu[6]) {
    uu[0] = a0 / 4.0;
    uu[1] = -(a0 + a1 + a2) / 6.0;
    uu[2] = -(a0 - a1 + a2) / 6.0;
    uu[3] = a0 / 24.0 + a1 / 12.0 + a2 / 6.0;
    uu[4] = a0 / 24.0 - a1 / 12.0 + a2 / 6.0;
    uu[5] = a2;
}

// F(2x4,3x3): item i = (tn, chunk, lane) of [K/32][Cstore/8][24][64][4]; fp64 arithmetic, one rounding
__device__ __forceinline__ void wino24_item(const float* __restrict__ w, float* __restrict__ out, size_t i, int K, int Cin, int nch, int mode) {
    const int lane = (int)(i & 63);
    const size_t rest = i >> 6;
    const int chunk = (int)(rest % nch);
    const int tn = (int)(rest / nch);
    const int n = tn * 32 + (lane & 31);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int c = chunk * 8 + (lane >> 5) * 4 + e;
        double gg[4][3];
        wino_gg(w, n, c, K, Cin, mode, gg);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double a0 = gg[q][0], a1 = gg[q][1], a2 = gg[q][2];
            double uu[6];
            wino24_g4(a0, a1, a2, uu);
            const size_t base = ((((size_t)tn * nch + chunk) * 24 + q * 6) * 64 + lane) * 4 + e;
#pragma unroll
            for (int nu = 0; nu < 6; ++nu) out[base + (size_t)nu * 256] = (float)uu[nu];
        }
    }
}

// split F(2x4,3x3) form (conv3x3_wino24sx): item i = (tn, k-step, lane) of [K/32][C/16][24 positions][3 planes][64 lanes][8 bf16].
// k slot e of lane (n, h = lane >> 5) is channel 16 step + 4 h + e (e < 4) or 16 step + 8 + 4 h + (e - 4): the two 8-channel chunks
// of the k-step side by side, as the kernel's lanes hold them.  Each value is wino24_item's (fp64 arithmetic, one rounding to fp32)
// cut into its three bf16 pieces (the truncation split of split3_bf16): the planes sum back to it bit for bit.
__device__ __forceinline__ void wino24sx_item(const float* __restrict__ w, unsigned short* __restrict__ out, size_t i, int K, int Cin, int nks, int mode) {
    const int lane = (int)(i & 63);
    const size_t rest = i >> 6;
    const int step = (int)(rest % nks);
    const int tn = (int)(rest / nks);
    const int n = tn * 32 + (lane & 31);
    unsigned short* o = out + ((size_t)tn * nks + step) * (24 * 3 * 512) + lane * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = step * 16 + (e >> 2) * 8 + (lane >> 5) * 4 + (e & 3);
        double gg[4][3];
        wino_gg(w, n, c, K, Cin, mode, gg);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            double uu[6];
            wino24_g4(gg[q][0], gg[q][1], gg[q][2], uu);
#pragma unroll
            for (int nu = 0; nu < 6; ++nu) {
                const float x = (float)uu[nu];
                const float x0 = top16(x);
                const float r = x - x0;
                const float y0 = top16(r);
                const float s = r - y0;
                unsigned short* d = o + (size_t)(q * 6 + nu) * 1536 + e;
                d[0] = (unsigned short)(__builtin_bit_cast(unsigned, x0) >> 16);
                d[512] = (unsigned short)(__builtin_bit_cast(unsigned, y0) >> 16);
                d[1024] = (unsigned short)(__builtin_bit_cast(unsigned, s) >> 16);
            }
        }
    }
}

// producer / consumer 1x1 form: item i = four floats of [K/128][4][C/8][64][4] from row-major [K, C] (16-byte aligned, C % 8 == 0)
__device__ __forceinline__ void pwpc_item(const float* __restrict__ w, float* __restrict__ out, size_t i, int C) {
    const int nsteps = C / 8;
    const int lane = (int)(i & 63);
    size_t rest = i >> 6;
    const int step = (int)(rest % nsteps); rest /= nsteps;
    const int nt = (int)rest;                // tn * 4 + w
    const int nn = nt * 32 + (lane & 31);
    const int c = 8 * step + 4 * (lane >> 5);
    *reinterpret_cast<f32x4*>(out + i * 4) = *reinterpret_cast<const f32x4*>(w + (size_t)nn * C + c);
}

// producer / consumer split 1x1 form (conv1x1_sxpc): item i = (n-tile of 32, k-step, lane) of [K/32][C/16][3 planes][64 lanes][8 bf16]
// from row-major [K, C]: the lane's eight weights W[32 nt + (lane & 31)][16 step + 8 (lane >> 5) + e] cut into their three bf16
// pieces (the truncation split of split3_bf16; top16 keeps every value its own register, see seam_split.h)
__device__ __forceinline__ void sxpc_item(const float* __restrict__ w, unsigned short* __restrict__ out, size_t i, int C) {
    const int nsteps = C / 16;
    const int lane = (int)(i & 63);
    const size_t rest = i >> 6;
    const int step = (int)(rest % nsteps);
    const size_t nt = rest / nsteps;
    const float* src = w + (nt * 32 + (lane & 31)) * (size_t)C + 16 * step + 8 * (lane >> 5);
    unsigned short* o = out + (nt * nsteps + step) * 1536 + lane * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float x = src[e];
        const float x0 = top16(x);
        const float r = x - x0;
        const float y0 = top16(r);
        const float s = r - y0;
        o[e] = (unsigned short)(__builtin_bit_cast(unsigned, x0) >> 16);
        o[512 + e] = (unsigned short)(__builtin_bit_cast(unsigned, y0) >> 16);
        o[1024 + e] = (unsigned short)(__builtin_bit_cast(unsigned, s) >> 16);
    }
}

// narrow (<= 16 outputs) form: item i of [C/16][64 lanes][4] from row-major [K, C]
__device__ __forceinline__ void narrow_item(const float* __restrict__ w, float* __restrict__ out, int i, int K, int C) {
    const int e = i & 3, lane = (i >> 2) & 63, j = i >> 8;
    const int col = lane & 15, kq = lane >> 4;
    out[i] = col < K ? w[(size_t)col * C + 16 * j + 4 * kq + e] : 0.f;
}

// weights-stationary form: row-major [K, C] with the row's epilogue scale folded in (one fp32 multiply; scale NULL: a copy)
__device__ __forceinline__ void sw_item(const float* __restrict__ w, const float* __restrict__ scale, float* __restrict__ out, size_t i, int C) {
    const float v = w[i];
    out[i] = scale ? v * scale[i / (size_t)C] : v;
}

}  // namespace seam_pack
