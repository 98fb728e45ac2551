// seam_wino24_common.h -- what the F(2x4,3x3) Winograd kernel files share: the launch arguments and their planner (the n-tile rules
// and the fastdiv magics; the block layout comes from seam_wino_layout.h, form F24), the raw-patch loader with its LDS rules, the
// symmetric block w24_block (K loop of conv3x3_wino24<NT> or, SX, of conv3x3_wino24sx; one epilogue) and the block's tile decode.
// seam_wino24.hip (fp32 MFMAs) and seam_wino24sx.hip (six-term split-bf16 MFMAs) include it; each describes its own kernel.
#pragma once
#include <hip/hip_runtime.h>
#include "seam_device.h"
#include <stdint.h>
#include <stdlib.h>
#include "seam_fastdiv.h"
#include "seam_launch.h"
#include "seam_opts.h"
#include "seam_split.h"
#include "seam_wino_layout.h"

namespace {

using namespace seam_wino_layout;      // Layout, choose_layout, wino_ok and the planners' shared tail

#ifndef SEAM_W24_PK
#define SEAM_W24_PK 1       // 1 (default): the in-loop input transform on packed fp32 VALU ops; 0: scalar-lane v_fma_f32 / v_add_f32
#endif
// The input transform's VALU work sits between fp32 MFMAs.  MI355X_MICROARCH.md lists packed fp32 VALU instructions as an
// anti-lever beside (bf16) MFMAs; beside FP32 MFMAs that does not hold -- measured on the bench's twelve layer shapes
// (profiles/r02_w24_scalar_valu.txt, one box): the scalar-lane form (72 v_fma/add/sub per chunk, SEAM_W24_PK=0) is 1-2 % SLOWER
// than the packed form (36 v_pk_*): the fp32 MFMA and the fp32 VALU share the SIMD's FMA lanes, what counts is FMAs, not opcodes.
__device__ __forceinline__ float s_fma(float c, float b, float a) {        // a + c * b, c wave-uniform (SGPR)
    float d;
    asm("v_fma_f32 %0, %1, %2, %3" : "=v"(d) : "s"(c), "v"(b), "v"(a));
    return d;
}
__device__ __forceinline__ float s_add(float a, float b) {
    float d;
    asm("v_add_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
    return d;
}
__device__ __forceinline__ float s_sub(float a, float b) {
    float d;
    asm("v_sub_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
    return d;
}
// the same with a wave-uniform multiplier held in an SGPR pair (one scalar source per VOP3P): the constants of B4t cost no
// VGPRs -- the register file is full (96 accumulators, two weight sets), and a VGPR temporary that aliases the
// destination of an in-flight weight load makes hipcc wait for that load
__device__ __forceinline__ f32x2 pk_fma_s(f32x2 cs, f32x2 b, f32x2 c) {
    f32x2 d;
    asm("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(d) : "s"(cs), "v"(b), "v"(c));
    return d;
}
__device__ __forceinline__ f32x4 fma4s(f32x2 cs, f32x4 b, f32x4 a) {      // a + cs * b
#if SEAM_W24_PK
    const f32x2 lo = pk_fma_s(cs, __builtin_shufflevector(b, b, 0, 1), __builtin_shufflevector(a, a, 0, 1));
    const f32x2 hi = pk_fma_s(cs, __builtin_shufflevector(b, b, 2, 3), __builtin_shufflevector(a, a, 2, 3));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3);
#else
    const float c = cs[0];
    return f32x4{s_fma(c, b[0], a[0]), s_fma(c, b[1], a[1]), s_fma(c, b[2], a[2]), s_fma(c, b[3], a[3])};
#endif
}
__device__ __forceinline__ f32x4 add4(f32x4 a, f32x4 b) {
#if SEAM_W24_PK
    const f32x2 lo = pk_add(__builtin_shufflevector(a, a, 0, 1), __builtin_shufflevector(b, b, 0, 1));
    const f32x2 hi = pk_add(__builtin_shufflevector(a, a, 2, 3), __builtin_shufflevector(b, b, 2, 3));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3);
#else
    return f32x4{s_add(a[0], b[0]), s_add(a[1], b[1]), s_add(a[2], b[2]), s_add(a[3], b[3])};
#endif
}
__device__ __forceinline__ f32x4 sub4(f32x4 a, f32x4 b) {
#if SEAM_W24_PK
    const f32x2 lo = pk_sub(__builtin_shufflevector(a, a, 0, 1), __builtin_shufflevector(b, b, 0, 1));
    const f32x2 hi = pk_sub(__builtin_shufflevector(a, a, 2, 3), __builtin_shufflevector(b, b, 2, 3));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3);
#else
    return f32x4{s_sub(a[0], b[0]), s_sub(a[1], b[1]), s_sub(a[2], b[2]), s_sub(a[3], b[3])};
#endif
}

#ifndef SEAM_W24_ABL
#define SEAM_W24_ABL 0      // kernel experiments (tools/experiments/wino24_abl.sh; operands keep the REAL data of chunks 0/1):
                            // 1 no in-loop patch loads / LDS stores, 2 no in-loop weight loads, 4 no barrier, 8 no in-loop transforms, 16 no epilogue
#endif

#ifndef SEAM_W24SX_ABL
#define SEAM_W24SX_ABL 0    // conv3x3_wino24sx experiments (tools/w24sx_abl_build.sh; operands keep the REAL data of k-steps 0 / 1):
                            // 1 no in-loop patch requests / LDS stores, 2 no in-loop weight loads, 8 no in-loop transform + split, 16 no epilogue arithmetic
#endif

struct Wino24Args {
    const float* x;
    const float* u;       // packed transformed weights
    const float* scale;
    const float* shift;
    const float* res;
    float* y;
    int N, H, W, C, K;
    int Ho, Wo, pad, relu;
    // Up to three regions tile an image (main region + right strip + bottom strip), each with its own block patch shape,
    // or -- stacked mode, maps narrower than a block -- TY[0] consecutive tile rows of the whole batch per block
    // (the conventions of seam_wino.hip's WinoArgs, chosen by the same seam_wino_layout.h; only the tile is 4 output columns wide).
    int nreg;
    int rx0[3], ry0[3];
    int rxe[3], rye[3];
    int TX[3], TY[3];     // tiles per block patch (TX*TY <= 32)
    int bx[3], by[3];
    int per_img;
    int stack;
    int tiles_y;
    int PH;
    int G;
    int nt;               // n-tiles per block (kernel template NT)
    int tiles_n;          // K / (32 * NT)
    int nchunks;          // C / 8
    // ceil(2^32 / d) of the divisors the block prologue needs (fdivu, seam_fastdiv.h): an integer division costs ~20 VALU instructions,
    // and VALU instructions of either resident block delay the matrix pipe
    unsigned m_tiles_n, m_per_img, m_tys, m_pitch, m_bx[3], m_TX[3], m_PW[3];
    // n-tile split over XCD groups (see the kernel's tile decode): nsplit groups, tns = tiles_n / nsplit n-tiles per group, the
    // patches (tm) cut into 8 / nsplit partitions of part_q (+1 for the first part_r) each
    int nsplit, tns, part_q, part_r;
    unsigned m_tns;
    int total_tiles;             // conv3x3_wino24pc: tiles of the launch (the grid is persistent: min(tiles, CUs) blocks)
    // conv3x3_wino24pc: a region's parameters side by side -- ONE wide scalar load per tile decode instead of a dozen dependent ones
    // (the kernel re-derives a tile's geometry from its index in several places; every dependent s_load is ~250 cycles of latency)
    struct Rg { int TX, TY, bx, by, rx0, ry0, rxe, rye; unsigned m_bx, m_TX, m_PW; int pad_[5]; } rg[3];
    unsigned long long* trace;   // SEAM_W24PC_TRACE builds only: s_memtime stamps of one block's waves 0 and 4 (else null)
};


constexpr int NPIXMAX = F24.npixmax;                // raw patch pixels per buffer (384: 3 x 16-byte loads per thread per chunk)
constexpr int NI = (2 * NPIXMAX + 255) / 256;
constexpr int ENTMAX = F24.entmax;                  // 16-byte LDS entries per channel half (672; row pairs x PR, see the kernel)
constexpr int RAWB = (2 * ENTMAX + 1) * 16;        // bytes per raw buffer (+1 dump slot for idle loader lanes)
static_assert(F24.tile_w == 4 && F24.slots == 32, "the chooser's tile and tile slots are the block's");

// NT = 32-channel n-tiles per block.  NT = 1: 96 accumulator VGPRs, two blocks per CU.  NT = 2: 192 accumulators (AccVGPRs), one block
// per CU, one wave per SIMD: every A fragment (the transform's output) and the raw patch feed twice the MFMAs.  Measured on this
// kernel: a SIMD does not overlap its MFMAs with anything else it issues -- one resident block instead of two costs only 10 %,
// MFMAs-only runs at the same speed with one or two blocks, and the K loop's time is the sum of its MFMA cycles and ~16 cycles per
// other vector instruction -- so what counts is MFMAs per transform / LDS / load instruction, not occupancy.
// HSC: the LDS phase stride HS = (TX + 1) | 1 as a compile-time constant (0 = take it from TX at run time).  With a constant HS every
// ds_read_b128 of the input transform is one base register + an immediate offset; with a run-time HS the compiler keeps 8-12 loop-
// invariant address registers per buffer alive through the K loop (and, in the NT = 2 form, spills them to AccVGPRs and reads them
// back every chunk).  The kernel dispatches on the block's region: HS = 9 (TX 7..8: the main region of every large map), 5 (TX 3..4),
// 3 (TX <= 2: the right-hand strips), anything else through the run-time form.
template <int NT, int HSC, bool SX = false>
__device__ __forceinline__ void w24_block(const Wino24Args& p, char* smem, const int reg, const int rb, const int tm, const int tn,
                                          const int tm_img) {
    char (*raw)[RAWB] = reinterpret_cast<char (*)[RAWB]>(smem);
    float* const ex = reinterpret_cast<float*>(smem);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int xi = tid >> 6;
    const int TX = p.TX[reg], TY = p.TY[reg];
    const int byi = fdivu(rb, p.bx[reg], p.m_bx[reg]);
    const int bxi = rb - byi * p.bx[reg];
    const int tys = p.tiles_y, pitch = 2 * tys + 2;
    const int R0 = tm * TY;                                // stacked mode: first tile row (global) of this block
    const int n_img = p.stack ? fdivu(R0, tys, p.m_tys) : tm_img;   // first image of this block
    const int prow0 = p.stack ? 2 * (R0 - n_img * tys) : 0;
    const int n_here = min(p.G, p.N - n_img);
    const int ty0 = p.stack ? 0 : p.ry0[reg] + byi * TY, tx0 = p.stack ? 0 : p.rx0[reg] + bxi * TX;
    const int tye = p.rye[reg], txe = p.rxe[reg];
    const int iy0 = 2 * ty0 - p.pad, ix0 = 4 * tx0 - p.pad; // top-left input pixel of the raw patch (regions mode)

    const int PW = 4 * TX + 2, PH = p.stack ? p.PH : 2 * TY + 2;
    const int NPIX = PW * PH;
    const int HS = HSC ? HSC : ((TX + 1) | 1);             // 16-byte entries per (patch row, x mod 4); odd: the four x phases of
                                                           // consecutive pixels land in four different 16-byte bank groups (stores)
    // A pair of patch rows (= one tile row step) takes PR entries, PR = 8 * HS rounded up to TX (mod 8): tile (r, tx) then
    // sits at r * PR + tx = lane (mod 8) -- the eight lanes of a ds_read_b128 phase always hit eight different 16-byte
    // bank groups, whatever the patch shape (without it tile rows alias: 8 * HS = 0 mod 8, two-way conflicts for TX < 8)
    const int PR = 8 * HS + (TX & 7);
    const int NENT0 = PR * ((PH + 1) >> 1);                // entries per channel half ...
    const int NENT = NENT0 + ((4 - NENT0) & 7);            // ... placed 4 (mod 8) apart: the two halves of a pixel (adjacent loader
                                                           // lanes) never share a bank group
    const int nslots = TX * TY;
    auto slot = [&](int id, int& g, int& ty, int& tx, int& prow) -> bool {
        const int r = fdivu(id, TX, p.m_TX[reg]);
        tx = tx0 + (id - r * TX);
        if (p.stack) {
            const int R = R0 + r;
            const int n = fdivu(R, tys, p.m_tys);
            g = n - n_img;
            ty = R - n * tys;
            prow = pitch * g + 2 * ty - prow0;
            return id < nslots && n < p.N;
        }
        g = 0;
        ty = ty0 + r;
        prow = 2 * r;
        return id < nslots && ty < tye && tx < txe;
    };

    // ---- raw patch loader -----------------------------------------------------------------------------------------
    const size_t img_bytes = (size_t)p.H * p.W * p.C * 4;
    const __amdgpu_buffer_rsrc_t x_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void*)((const char*)p.x + (size_t)n_img * img_bytes), 0, (int)(img_bytes * n_here), 0x00020000);
    unsigned goff[NI];
    int loff[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int idx = tid + 256 * i;
        const int half = idx & 1;
        const int pix = idx >> 1;
        const bool ok = pix < NPIX;
        const int v = fdivu(pix, PW, p.m_PW[reg]);          // patch row
        const int px = pix - v * PW;
        int g = 0, gy = iy0 + v;
        if (p.stack) {
            const int vr = prow0 + v;
            g = fdivu(vr, pitch, p.m_pitch);
            gy = vr - g * pitch - p.pad;
        }
        const int gx = ix0 + px;
        const bool inb = ok && g < n_here && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
        goff[i] = inb ? (unsigned)((((g * p.H + gy) * p.W + gx) * p.C + half * 4) * 4) : kOob;
        loff[i] = ok ? (half * NENT + (v >> 1) * PR + ((v & 1) * 4 + (px & 3)) * HS + (px >> 2)) * 16 : 2 * ENTMAX * 16;
    }
    constexpr int NRS = SX || NT == 1 ? 2 : 1;     // (SX: the two chunks of a k-step) register sets of the raw patch: prefetch distance 2 chunks / 1 (twice as long) chunk
    f32x4 rset[NRS][NI];
    auto load_raw = [&](f32x4 (&rs)[NI], int chunk) {
        // chunks past the end (the prefetch runs 2-4 ahead) re-read the last chunk and are never used (one s_min; unclamped they
        // would read the next pixel's channels or, at the image group's last pixel, fall outside the descriptor and read zeros:
        // gfx950 range-checks the scalar offset too, profiles/r06_soffset_probe.txt)
        const int so = min(chunk, p.nchunks - 1) * 32;
#pragma unroll
        for (int i = 0; i < NI; ++i)
            rs[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(x_rsrc, goff[i], so, 0));
    };
    auto store_raw = [&](const f32x4 (&rs)[NI], int buf) {
#pragma unroll
        for (int i = 0; i < NI; ++i) *reinterpret_cast<f32x4*>(&raw[buf][loff[i]]) = rs[i];
    };


    // ---- weight fragments: [tn32][chunk][p = 6*xi + nu][lane][4]; this block's n-tiles are tn32 = NT * tn + nt --------
    const int ntile_bytes = p.nchunks * 24576;
    const __amdgpu_buffer_rsrc_t u_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void*)((const char*)p.u + (size_t)tn * NT * ntile_bytes), 0, NT * ntile_bytes, 0x00020000);
    // lane offsets of positions nu = 0..3 and 4..5: the per-position 1 KiB steps then fit the instruction's 12-bit immediate, and the
    // scalar offset is one value per chunk (and n-tile).  Chunks past the end are clamped to the last one and never used.
    // (ONE lane offset, made opaque once per chunk: hipcc otherwise hoists the six "offset + nu KiB" sums out of the K loop, parks
    //  them in AccVGPRs and pays a v_accvgpr_read -- a vector-ALU instruction, i.e. ~20 idle cycles of the fp32 matrix pipe -- per load)
    int uoff0 = (xi * 6 * 64 + lane) * 16;
    constexpr int NBS = 2;                   // weight register sets: chunk t + 1's are requested at the top of chunk t
    f32x4 bfs[NBS][NT][6];
    auto load_b = [&](f32x4 (&bf)[NT][6], int nu, int chunk) {       // position nu of every n-tile
        const int so = min(chunk, p.nchunks - 1) * 24576 + (nu >> 2) * 4096;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
            bf[nt][nu] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(u_rsrc, uoff0 + (nu & 3) * 1024, so + nt * ntile_bytes, 0));
    };

    // ---- input transform --------------------------------------------------------------------------------------------
    // columns (B4t over j = 0..5):
    //   V0 = 4 T0 - 5 T2 + T4            V5 = 4 T1 - 5 T3 + T5
    //   V1 = (T4 - 4 T2) + (T3 - 4 T1)   V2 = (T4 - 4 T2) - (T3 - 4 T1)
    //   V3 = (T4 - T2) + 2 (T3 - T1)     V4 = (T4 - T2) - 2 (T3 - T1)
    // rows (B2t, this wave's xi): xi0: d0 - d2, xi1: d1 + d2, xi2: d2 - d1, xi3: d1 - d3   =>  T_j = d[ra][j] + cb * d[rb][j]
    const int ra = xi == 0 ? 0 : xi == 2 ? 2 : 1;
    const int rbw = xi == 0 ? 2 : xi == 1 ? 2 : xi == 2 ? 1 : 3;
    const float cb = __builtin_amdgcn_readfirstlane(xi) == 1 ? 1.f : -1.f;
    int rbase;
    {
        int g, ty, tx, prow;
        if (!slot(lane & 31, g, ty, tx, prow)) slot(0, g, ty, tx, prow);
        rbase = ((lane >> 5) * NENT + (prow >> 1) * PR + (tx - tx0)) * 16;
    }
    const int oa = ((ra >> 1) * PR + (ra & 1) * 4 * HS) * 16, ob = ((rbw >> 1) * PR + (rbw & 1) * 4 * HS) * 16;
    const int c1 = HS * 16;
    const f32x2 cb2 = {cb, cb};
    const f32x2 k4 = {4.f, 4.f}, km5 = {-5.f, -5.f}, km4 = {-4.f, -4.f}, k2 = {2.f, 2.f}, km2 = {-2.f, -2.f};
    f32x4 va[6];            // A fragments of the current chunk (rolling: overwritten pair by pair with the next chunk's)
    f32x4 vb[2];            // NT = 2: the second set of positions 3, 4 (chunks alternate between va[3..4] and vb[0..1])
    f32x4 T0, T1, T2, T3, T4, T5;
    f32x4 xa[3], xb[3];
    f32x4 ya[3], yb[3];     // NT = 2: the odd columns, so that all twelve reads of a chunk are in flight together
    auto rdA = [&](int buf) {            // columns 0, 2, 4
        const char* base = &raw[buf][rbase];
        xa[0] = *reinterpret_cast<const f32x4*>(base + oa);
        xb[0] = *reinterpret_cast<const f32x4*>(base + ob);
        xa[1] = *reinterpret_cast<const f32x4*>(base + oa + 2 * c1);
        xb[1] = *reinterpret_cast<const f32x4*>(base + ob + 2 * c1);
        xa[2] = *reinterpret_cast<const f32x4*>(base + oa + 16);
        xb[2] = *reinterpret_cast<const f32x4*>(base + ob + 16);
    };
    auto rdB = [&](int buf) {            // columns 1, 3, 5
        const char* base = &raw[buf][rbase];
        xa[0] = *reinterpret_cast<const f32x4*>(base + oa + c1);
        xb[0] = *reinterpret_cast<const f32x4*>(base + ob + c1);
        xa[1] = *reinterpret_cast<const f32x4*>(base + oa + 3 * c1);
        xb[1] = *reinterpret_cast<const f32x4*>(base + ob + 3 * c1);
        xa[2] = *reinterpret_cast<const f32x4*>(base + oa + c1 + 16);
        xb[2] = *reinterpret_cast<const f32x4*>(base + ob + c1 + 16);
    };
    auto rdB2 = [&](int buf) {           // columns 1, 3, 5 into their own registers
        const char* base = &raw[buf][rbase];
        ya[0] = *reinterpret_cast<const f32x4*>(base + oa + c1);
        yb[0] = *reinterpret_cast<const f32x4*>(base + ob + c1);
        ya[1] = *reinterpret_cast<const f32x4*>(base + oa + 3 * c1);
        yb[1] = *reinterpret_cast<const f32x4*>(base + ob + 3 * c1);
        ya[2] = *reinterpret_cast<const f32x4*>(base + oa + c1 + 16);
        yb[2] = *reinterpret_cast<const f32x4*>(base + ob + c1 + 16);
    };
    auto cTB2 = [&]() { T1 = fma4s(cb2, yb[0], ya[0]); T3 = fma4s(cb2, yb[1], ya[1]); T5 = fma4s(cb2, yb[2], ya[2]); };
    auto cV34to = [&](f32x4& v3, f32x4& v4) {
        const f32x4 c = sub4(T4, T2), d = sub4(T3, T1);
        v3 = fma4s(k2, d, c);
        v4 = fma4s(km2, d, c);
    };
    auto cTA = [&]() { T0 = fma4s(cb2, xb[0], xa[0]); T2 = fma4s(cb2, xb[1], xa[1]); T4 = fma4s(cb2, xb[2], xa[2]); };
    auto cTB = [&]() { T1 = fma4s(cb2, xb[0], xa[0]); T3 = fma4s(cb2, xb[1], xa[1]); T5 = fma4s(cb2, xb[2], xa[2]); };
    auto cV05 = [&]() {
        va[0] = fma4s(km5, T2, fma4s(k4, T0, T4));
        va[5] = fma4s(km5, T3, fma4s(k4, T1, T5));
    };
    auto cV12 = [&]() {
        const f32x4 a = fma4s(km4, T2, T4), bq = fma4s(km4, T1, T3);
        va[1] = add4(a, bq);
        va[2] = sub4(a, bq);
    };
    auto cV34 = [&]() {
        const f32x4 c = sub4(T4, T2), d = sub4(T3, T1);
        va[3] = fma4s(k2, d, c);
        va[4] = fma4s(km2, d, c);
    };


    f32x16 acc[6][NT];
#pragma unroll
    for (int nu = 0; nu < 6; ++nu)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[nu][nt][r] = 0.f;

#define MF(nu, kk) do { _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) { \
        acc[nu][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(va[nu][kk], bcur[nt][nu][kk], acc[nu][nt], 0, 0, 0); if (nt + 1 < NT) SB(); } } while (0)
#define MG(frag, nu, kk) do { _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) { \
        acc[nu][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(frag[kk], bcur[nt][nu][kk], acc[nu][nt], 0, 0, 0); if (nt + 1 < NT) SB(); } } while (0)

    // ---- prologue -------------------------------------------------------------------------------------------------
    if constexpr (!SX) {
    load_raw(rset[0], 0);
    if constexpr (NRS == 2) load_raw(rset[1], 1);
#pragma unroll
    for (int nu = 0; nu < 6; ++nu) load_b(bfs[0], nu, 0);
    store_raw(rset[0], 0);
    if constexpr (NRS == 2) {
        store_raw(rset[1], 1);
        load_raw(rset[0], 2);
        load_raw(rset[1], 3);
    } else {
        load_raw(rset[0], 1);
        store_raw(rset[0], 1);
        load_raw(rset[0], 2);
    }
    __syncthreads();
    rdA(0); cTA(); rdB(0); cTB(); cV05(); cV12();     // NT = 1: V3, V4 of chunk 0 are made in its first slot
    if constexpr (NT == 2) cV34to(va[3], va[4]);
    __syncthreads();                                  // chunk 0 overwrites raw[0] right away
    }

    // At the top of chunk t: raw[t&1] = patch(t) (already consumed), raw[(t+1)&1] = patch(t+1), rset[t&1] = patch(t+2) in
    // flight, rset[(t+1)&1] = patch(t+3) in flight, bf = weights(t), va[0,5,1,2] = A fragments of chunk t, T0..T5 = the
    // row transform of chunk t (V3, V4 still to be made from it).
#define A1(x) do { if (!(SEAM_W24_ABL & 1)) { x; } } while (0)
#define A2(x) do { if (!(SEAM_W24_ABL & 2)) { x; } } while (0)
#define A8(x) do { if (!(SEAM_W24_ABL & 8)) { x; } } while (0)
    // Weights: two register sets, all six loads of chunk t+1 issued at the top of chunk t, BEFORE the patch loads -- the
    // vector-memory counter retires in order, so a wait for a weight fragment also waits for every older load: with the
    // weights first, the (HBM-latency) patch loads of chunk t are not forced to complete before the top of chunk t+2.
    auto chunk = [&](int t, int par, f32x4 (&bcur)[NT][6], f32x4 (&bnext)[NT][6]) {
        asm volatile("" : "+v"(uoff0));
        if constexpr (NT == 1) {
            SB(); MF(0, 0); A8(cV34());
            SB(); MF(5, 0); A8(rdA(par ^ 1));
            SB(); MF(0, 1);
            SB(); MF(5, 1);
            SB(); MF(0, 2); A8(cTA());
            SB(); MF(5, 2); A8(rdB(par ^ 1));
            SB(); MF(0, 3);
            SB(); MF(5, 3);
            SB(); MF(1, 0); A8(cTB());
            SB(); MF(2, 0); A8(cV05());
            SB(); MF(1, 1); A2(load_b(bnext, 0, t + 1); load_b(bnext, 5, t + 1));
            SB(); MF(2, 1); A2(load_b(bnext, 1, t + 1); load_b(bnext, 2, t + 1));
            SB(); MF(1, 2); A2(load_b(bnext, 3, t + 1); load_b(bnext, 4, t + 1));
            SB(); MF(2, 2);
            SB(); MF(1, 3);
            SB(); MF(2, 3);
            SB(); MF(3, 0); A8(cV12());
            SB(); MF(4, 0); A1(store_raw(rset[par], par));
            SB(); MF(3, 1); A1(load_raw(rset[par], t + 4));
            SB(); MF(4, 1);
            SB(); MF(3, 2);
            SB(); MF(4, 2);
            SB(); MF(3, 3);
            SB(); MF(4, 3);
            SB();
        } else {
            // Two MFMAs per MF().  What tools/mfma_shadow_probe.hip measured (profiles/r04_mfma_shadow_probe.txt): in ONE wave no
            // vector-ALU instruction overlaps an fp32 MFMA -- a group of k of them between two MFMAs idles the matrix pipe for
            // ~17 + 4.5 k cycles -- while LDS reads, global loads and scalar instructions are free.  So the whole input
            // transform of chunk t + 1 (36 packed ops) is ONE group, placed behind the 32 MFMAs of positions 0, 5, 1, 2 (whose
            // fragments it overwrites); positions 3, 4 alternate between two register sets (va[3..4] / vb[0..1] by chunk
            // parity), so nothing of the transform is carried across the chunk boundary; the twelve patch reads it needs are
            // issued together, 8 MFMAs ahead.  Two weight register sets (the arch file has room: 162 of 256 were in use): chunk
            // t + 1's twelve fragments are requested at the top of chunk t, ahead of the patch loads in the in-order vmcnt queue.
            SB(); MF(0, 0); A2(load_b(bnext, 0, t + 1));
            SB(); MF(5, 0); A2(load_b(bnext, 5, t + 1));
            SB(); MF(0, 1); A2(load_b(bnext, 1, t + 1));
            SB(); MF(5, 1); A2(load_b(bnext, 2, t + 1));
            SB(); MF(0, 2); A2(load_b(bnext, 3, t + 1));
            SB(); MF(5, 2); A2(load_b(bnext, 4, t + 1));
            SB(); MF(0, 3);
            SB(); MF(5, 3);
            SB(); MF(1, 0);
            SB(); MF(2, 0);
            SB(); MF(1, 1); A1(store_raw(rset[0], par));
            SB(); MF(2, 1); A1(load_raw(rset[0], t + 3));
            SB(); MF(1, 2); A8(rdA(par ^ 1); rdB2(par ^ 1));
            SB(); MF(2, 2);
            SB(); MF(1, 3);
            SB(); MF(2, 3);
            SB();
            A8(cTA(); cTB2(); cV05(); cV12());
            if (par == 0) {
                A8(cV34to(vb[0], vb[1]));
                SB(); MG(va[3], 3, 0);
                SB(); MG(va[4], 4, 0);
                SB(); MG(va[3], 3, 1);
                SB(); MG(va[4], 4, 1);
                SB(); MG(va[3], 3, 2);
                SB(); MG(va[4], 4, 2);
                SB(); MG(va[3], 3, 3);
                SB(); MG(va[4], 4, 3);
            } else {
                A8(cV34to(va[3], va[4]));
                SB(); MG(vb[0], 3, 0);
                SB(); MG(vb[1], 4, 0);
                SB(); MG(vb[0], 3, 1);
                SB(); MG(vb[1], 4, 1);
                SB(); MG(vb[0], 3, 2);
                SB(); MG(vb[1], 4, 2);
                SB(); MG(vb[0], 3, 3);
                SB(); MG(vb[1], 4, 3);
            }
            SB();
        }
        if (!(SEAM_W24_ABL & 4)) __syncthreads();
    };
    if constexpr (!SX) {
    for (int t = 0; t < p.nchunks; t += 2) {
        chunk(t, 0, bfs[0], bfs[NBS - 1]);
        if (t + 1 < p.nchunks) chunk(t + 1, 1, bfs[NBS - 1], bfs[0]);
    }
    }
#undef MF
#undef MG
#undef A1
#undef A2
#undef A8

    if constexpr (SX) {
        // ---- conv3x3_wino24sx: the K loop on six-term split-bf16 MFMAs (arithmetic and schedule: seam_wino24sx.hip) ---------
        static_assert(NT == 2, "the split form is the two n-tile block");
        const int nks = p.nchunks >> 1;                    // k-steps of 16 channels = two raw chunks; raw[2 * (q & 1) + j] = chunk j of k-step q
        // weight planes [tn32][k-step][p = 6*xi + nu][plane][lane][8 bf16]: 1 KiB per (position, plane), 72 KiB per k-step.  The lane
        // offset is one register (made opaque once per k-step, as in the fp32 loop); plane index (3 nu + pl) & 3 goes into the
        // instruction's immediate, the rest into the scalar offset.  k-steps past the end are clamped to the last one and never used.
        const int xtile_bytes = nks * 73728;
        const __amdgpu_buffer_rsrc_t ux_rsrc = __builtin_amdgcn_make_buffer_rsrc(
            (void*)((const char*)p.u + (size_t)tn * 2 * xtile_bytes), 0, 2 * xtile_bytes, 0x00020000);
        int uxoff = (xi * 18 * 64 + lane) * 16;
        u32x4 wr[3][2][3];                                 // ring of three positions: [slot][n-tile][plane]
        auto load_w = [&](u32x4 (&w)[2][3], int nu, int ks) {
            const int so = min(ks, nks - 1) * 73728;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) {
                    const int idx = nu * 3 + pl;
                    w[nt][pl] = __builtin_amdgcn_raw_buffer_load_b128(ux_rsrc, uxoff + (idx & 3) * 1024, so + nt * xtile_bytes + (idx >> 2) * 4096, 0);
                }
        };

        // input transform: the fp32 loop's expressions on scalar-lane fmas (the same results as its packed form), then the
        // three-way cut; chunk j of the k-step fills words 2j, 2j + 1 of a plane register (k slots 4j .. 4j + 3 of the lane)
        auto fmal = [](float c, f32x4 b, f32x4 a) -> f32x4 {       // a + c * b
            return f32x4{__builtin_fmaf(c, b[0], a[0]), __builtin_fmaf(c, b[1], a[1]), __builtin_fmaf(c, b[2], a[2]), __builtin_fmaf(c, b[3], a[3])};
        };
        u32x4 ap[6][3];         // A planes of the current k-step (rolling: overwritten position by position with the next k-step's)
        u32x4 aq[2][3];         // the second set of positions 3, 4 (k-steps alternate between ap[3..4] and aq[0..1])
        f32x4 T[2][6];
        auto rdT = [&](int j, int buf) {                           // chunk j: the twelve patch reads and the row transform
            const char* base = &raw[buf][rbase];
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                const int col = (c & 3) * c1 + (c >> 2) * 16;
                const f32x4 xa = *reinterpret_cast<const f32x4*>(base + oa + col);
                const f32x4 xb = *reinterpret_cast<const f32x4*>(base + ob + col);
                T[j][c] = fmal(cb, xb, xa);
            }
        };
        auto put = [&](u32x4 (&pl)[3], int j, const f32x4 v) {
            u32x2 p0, p1, p2;
            split3_bf16(v, p0, p1, p2);
            pl[0][2 * j] = p0[0]; pl[0][2 * j + 1] = p0[1];
            pl[1][2 * j] = p1[0]; pl[1][2 * j + 1] = p1[1];
            pl[2][2 * j] = p2[0]; pl[2][2 * j + 1] = p2[1];
        };
        auto cV0 = [&](int j) { put(ap[0], j, fmal(-5.f, T[j][2], fmal(4.f, T[j][0], T[j][4]))); };
        auto cV5 = [&](int j) { put(ap[5], j, fmal(-5.f, T[j][3], fmal(4.f, T[j][1], T[j][5]))); };
        auto cV1 = [&](int j) { put(ap[1], j, fmal(-4.f, T[j][2], T[j][4]) + fmal(-4.f, T[j][1], T[j][3])); };
        auto cV2 = [&](int j) { put(ap[2], j, fmal(-4.f, T[j][2], T[j][4]) - fmal(-4.f, T[j][1], T[j][3])); };
        auto cV3 = [&](u32x4 (&pl)[3], int j) { put(pl, j, fmal(2.f, T[j][3] - T[j][1], T[j][4] - T[j][2])); };
        auto cV4 = [&](u32x4 (&pl)[3], int j) { put(pl, j, fmal(-2.f, T[j][3] - T[j][1], T[j][4] - T[j][2])); };

        // the six piece products of both accumulator tiles of a position, (activation piece, weight piece) in the project's order;
        // the MFMA group takes one MFMA and up to six plain vector-ALU instructions of the step's transform work in turn
#define MX1(nu, A, W, i, j) do { _Pragma("unroll") for (int nt = 0; nt < 2; ++nt) \
        acc[nu][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A[i]), __builtin_bit_cast(bf16x8, W[nt][j]), acc[nu][nt], 0, 0, 0); } while (0)
#define MX(nu, A, W) do { MX1(nu, A, W, 2, 0); MX1(nu, A, W, 1, 1); MX1(nu, A, W, 0, 2); MX1(nu, A, W, 1, 0); MX1(nu, A, W, 0, 1); MX1(nu, A, W, 0, 0); \
        _Pragma("unroll") for (int g = 0; g < 12; ++g) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x002, 6, 0); } \
        SB(); } while (0)
#define X1(x) do { if (!(SEAM_W24SX_ABL & 1)) { x; } } while (0)
#define X2(x) do { if (!(SEAM_W24SX_ABL & 2)) { x; } } while (0)
#define X8(x) do { if (!(SEAM_W24SX_ABL & 8)) { x; } } while (0)

        // ---- prologue: k-steps 0, 1 into LDS, k-step 2 in flight, the first three positions' weights, the planes of k-step 0 ----
        load_raw(rset[0], 0); load_raw(rset[1], 1);
        load_w(wr[0], 0, 0); load_w(wr[1], 5, 0); load_w(wr[2], 1, 0);
        store_raw(rset[0], 0); store_raw(rset[1], 1);
        load_raw(rset[0], 2); load_raw(rset[1], 3);
        store_raw(rset[0], 2); store_raw(rset[1], 3);
        load_raw(rset[0], 4); load_raw(rset[1], 5);
        LDS_BAR();
#pragma unroll
        for (int j = 0; j < 2; ++j) { rdT(j, j); cV0(j); cV5(j); cV1(j); cV2(j); cV3(ap[3], j); cV4(ap[4], j); }
        if (SEAM_W24SX_ABL & 8) {
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) { aq[0][pl] = ap[3][pl]; aq[1][pl] = ap[4][pl]; }
        }
        LDS_BAR();                                         // k-step 0 overwrites raw[0], raw[1] right away

        // At the top of k-step s (par = s & 1): raw[2 par ..] = patch(s) (consumed), raw[2 (par ^ 1) ..] = patch(s + 1), rset = patch(s + 2)
        // in flight, ap (positions 3, 4: ap or aq by parity) = the planes of k-step s, wr[0..2] = the weights of positions 0, 5, 1.
        // The ring slot a position frees is refilled right behind its MFMAs with the position three places on; the patch requests
        // of k-step s + 3 go out at the top, behind the three weight requests already in flight.
        auto kstep = [&](int s, int par) {
            asm volatile("" : "+v"(uxoff));
            X1(store_raw(rset[0], 2 * par); store_raw(rset[1], 2 * par + 1));
            X1(load_raw(rset[0], 2 * s + 6); load_raw(rset[1], 2 * s + 7));
            SB();
            X8(rdT(0, 2 * (par ^ 1)); rdT(1, 2 * (par ^ 1) + 1));
            MX(0, ap[0], wr[0]); X2(load_w(wr[0], 2, s)); SB();
            X8(cV0(0); cV0(1));
            MX(5, ap[5], wr[1]); X2(load_w(wr[1], 3, s)); SB();
            X8(cV5(0); cV5(1));
            MX(1, ap[1], wr[2]); X2(load_w(wr[2], 4, s)); SB();
            X8(cV1(0); cV1(1));
            MX(2, ap[2], wr[0]); X2(load_w(wr[0], 0, s + 1)); SB();
            if (par == 0) {
                X8(cV2(0); cV2(1); cV3(aq[0], 0));
                MX(3, ap[3], wr[1]); X2(load_w(wr[1], 5, s + 1)); SB();
                X8(cV3(aq[0], 1); cV4(aq[1], 0); cV4(aq[1], 1));
                MX(4, ap[4], wr[2]); X2(load_w(wr[2], 1, s + 1)); SB();
            } else {
                X8(cV2(0); cV2(1); cV3(ap[3], 0));
                MX(3, aq[0], wr[1]); X2(load_w(wr[1], 5, s + 1)); SB();
                X8(cV3(ap[3], 1); cV4(ap[4], 0); cV4(ap[4], 1));
                MX(4, aq[1], wr[2]); X2(load_w(wr[2], 1, s + 1)); SB();
            }
            LDS_BAR();
        };
        for (int s = 0; s < nks; s += 2) {
            kstep(s, 0);
            kstep(s + 1, 1);
        }
#undef MX1
#undef MX
#undef X1
#undef X2
#undef X8
    }

    // ---- epilogue: output transform + scale/shift (+ residual, ReLU) ------------------------------------------------
    //   columns (A4t over nu): Y0 = m0+m1+m2+m3+m4, Y1 = (m1-m2) + 2(m3-m4), Y2 = (m1+m2) + 4(m3+m4), Y3 = (m1-m2) + 8(m3-m4) + m5
    //   rows (A2t over xi, across the waves): y0 = q0+q1+q2, y1 = q1-q2-q3
    if ((SX ? SEAM_W24SX_ABL : SEAM_W24_ABL) & 16) {            // experiment: no epilogue (one conditional store keeps the accumulators alive)
        float sum = 0.f;
#pragma unroll
        for (int nu = 0; nu < 6; ++nu)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) sum += acc[nu][nt][r];
        if (sum == 123456.789f) p.y[tid] = sum;
        return;
    }
    const size_t out_img = (size_t)p.Ho * p.Wo * p.K * 4;
    const __amdgpu_buffer_rsrc_t y_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void*)((char*)p.y + (size_t)n_img * out_img), 0, (int)(out_img * n_here), 0x00020000);
    const __amdgpu_buffer_rsrc_t r_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void*)((const char*)(p.res ? p.res : p.y) + (size_t)n_img * out_img), 0, (int)(out_img * n_here), 0x00020000);
    const int et = tid >> 3;          // tile of the exchange this thread finishes
    const int n4 = tid & 7;
    int g, tyt, txt, prow_unused;
    const bool tile_ok = slot(et, g, tyt, txt, prow_unused) && g < n_here;
    const int oy = 2 * tyt, ox = 4 * txt;
    const int cstep = p.K * 4, rstep = p.Wo * cstep;                      // bytes per output pixel / row
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int ncol = (tn * NT + nt) * 32 + n4 * 4;
        f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
        if (p.scale) sc = *reinterpret_cast<const f32x4*>(p.scale + ncol);
        if (p.shift) sh = *reinterpret_cast<const f32x4*>(p.shift + ncol);
        const unsigned obase = (unsigned)(((g * p.Ho + oy) * p.Wo + ox) * p.K + ncol) * 4u;
        __syncthreads();              // previous readers of `ex` (first pass: of the raw buffers it aliases) are done
        // nu half (A4t) on register PAIRS (acc[nu][nt][r], [r+1] are adjacent registers): packed fp32; each pair goes straight to LDS
        {
            const f32x2 c2 = {2.f, 2.f}, c4 = {4.f, 4.f}, c8 = {8.f, 8.f};
#pragma unroll
            for (int h = 0; h < 8; ++h) {
                // NT = 2: the 192 accumulators live in AccVGPRs; read the 12 values of this step explicitly, one step at a time --
                // left to itself the compiler copies ALL of them into arch VGPRs at the loop exit and pays for that register peak
                // by spilling the K loop's address registers
                auto rd = [&](int nu) -> f32x2 {
                    if constexpr (NT == 2) {
                        float x0, x1;
                        asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(x0) : "a"(acc[nu][nt][2 * h]));
                        asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(x1) : "a"(acc[nu][nt][2 * h + 1]));
                        return f32x2{x0, x1};
                    } else {
                        return f32x2{acc[nu][nt][2 * h], acc[nu][nt][2 * h + 1]};
                    }
                };
                const f32x2 m0 = rd(0), m1 = rd(1), m2 = rd(2), m3 = rd(3), m4 = rd(4), m5 = rd(5);
                const f32x2 s12 = pk_add(m1, m2), d12 = pk_sub(m1, m2), s34 = pk_add(m3, m4), d34 = pk_sub(m3, m4);
                const f32x2 y0 = pk_add(pk_add(m0, s12), s34);
                const f32x2 y1 = pk_fma_s(c2, d34, d12);
                const f32x2 y2 = pk_fma_s(c4, s34, s12);
                const f32x2 y3 = pk_add(pk_fma_s(c8, d34, d12), m5);
                const int r = 2 * h;
                const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                float* e0 = &ex[((xi * 4 + 0) * 32 + row) * 32 + (lane & 31)];
                e0[0] = y0[0];               e0[32] = y0[1];
                e0[1024] = y1[0];            e0[1024 + 32] = y1[1];
                e0[2048] = y2[0];            e0[2048 + 32] = y2[1];
                e0[3072] = y3[0];            e0[3072 + 32] = y3[1];
            }
        }
        __syncthreads();
#pragma unroll
        for (int bcol = 0; bcol < 4; ++bcol) {
            const f32x4 q0 = *reinterpret_cast<const f32x4*>(&ex[((0 * 4 + bcol) * 32 + et) * 32 + n4 * 4]);
            const f32x4 q1 = *reinterpret_cast<const f32x4*>(&ex[((1 * 4 + bcol) * 32 + et) * 32 + n4 * 4]);
            const f32x4 q2 = *reinterpret_cast<const f32x4*>(&ex[((2 * 4 + bcol) * 32 + et) * 32 + n4 * 4]);
            const f32x4 q3 = *reinterpret_cast<const f32x4*>(&ex[((3 * 4 + bcol) * 32 + et) * 32 + n4 * 4]);
            f32x4 yv[2];
            yv[0] = q0 + q1 + q2;
            yv[1] = q1 - q2 - q3;
#pragma unroll
            for (int aa = 0; aa < 2; ++aa) {
                const bool ok = tile_ok && (oy + aa) < p.Ho && (ox + bcol) < p.Wo;
                const unsigned off = ok ? obase + (unsigned)(aa * rstep + bcol * cstep) : kOob;
                f32x4 v = yv[aa] * sc + sh;
                if (p.res) {
                    const f32x4 rv = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r_rsrc, off, 0, 0));
                    if (p.relu == 2) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = rv[e] > 0.f ? v[e] : 0.f;
                    } else {
                        v += rv;
                    }
                }
                if (p.relu == 1) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
                }
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), y_rsrc, off, 0, 0);
            }
        }
    }
}

// the tile decode of the symmetric kernels (one tile per block): XCD-aware tile id (bijective), region, LDS phase stride
template <int NT, bool SX>
__device__ __forceinline__ void w24_tile(const Wino24Args& p, char* smem) {
    // ---- XCD-aware tile id (bijective) ----------------------------------------------------------------------------
    const int nblk = gridDim.x;
    const int b = blockIdx.x;
    const int xcd = b & 7;
    int tm, tn;
    if (p.nsplit > 1) {
        // The n-tiles are split over `nsplit` groups of XCDs (workgroup b runs on XCD b & 7): XCD x streams only the n-tile subset
        // g = x % nsplit -- its share of the transformed weights (24*K*C*4 / nsplit bytes) stays in the XCD's 4 MiB L2 instead of
        // being re-streamed from the Infinity Cache by every generation of resident blocks, so the latency-critical weight loads
        // hit -- and the 8 / nsplit XCDs of a group share the patch range of partition pi = x / nsplit (every patch is then read
        // by nsplit XCDs: patch loads run 2+ chunks ahead and tolerate the miss).
        const int g = xcd % p.nsplit, pi = xcd / p.nsplit;
        const int j = b >> 3;
        const int tml = fdivu(j, p.tns, p.m_tns);
        tn = g * p.tns + (j - tml * p.tns);
        const int size = p.part_q + (pi < p.part_r ? 1 : 0);
        if (tml >= size) return;                           // padding blocks of the shorter partitions
        tm = pi * p.part_q + min(pi, p.part_r) + tml;
    } else {
        const int q8 = nblk >> 3, rem8 = nblk & 7;
        const int tile = (xcd < rem8 ? xcd * (q8 + 1) : rem8 * (q8 + 1) + (xcd - rem8) * q8) + (b >> 3);
        tm = fdivu(tile, p.tiles_n, p.m_tiles_n);
        tn = tile - tm * p.tiles_n;
    }
    const int per_img = p.per_img;
    const int tm_img = fdivu(tm, per_img, p.m_per_img);
    int rb = tm - tm_img * per_img;
    int reg = 0;
    if (p.nreg > 1 && rb >= p.bx[0] * p.by[0]) {
        rb -= p.bx[0] * p.by[0];
        reg = 1;
        if (p.nreg > 2 && rb >= p.bx[1] * p.by[1]) { rb -= p.bx[1] * p.by[1]; reg = 2; }
    }
    const int hs = (p.TX[reg] + 1) | 1;                    // block-uniform
    if (hs == 9) w24_block<NT, 9, SX>(p, smem, reg, rb, tm, tn, tm_img);
    else if (hs == 3) w24_block<NT, 3, SX>(p, smem, reg, rb, tm, tn, tm_img);
    else if (hs == 5) w24_block<NT, 5, SX>(p, smem, reg, rb, tm, tn, tm_img);
    else w24_block<NT, 0, SX>(p, smem, reg, rb, tm, tn, tm_img);
}

// n-tiles per block.  NT = 2 (one block per CU, 192 accumulators in AccVGPRs, every A fragment and the raw patch feeding twice
// the MFMAs) is built and parity-clean but NOT the default: as compiled by hipcc 7.2 it ties on the 200^2 layers and loses
// 3-13 % elsewhere -- the register allocator parks the loop-invariant LDS / load addresses and 8 transform registers in spare
// AccVGPRs and re-reads them (~60 v_accvgpr_read per 96 MFMAs) although ~90 arch VGPRs stay unused in the loop, and an asm MFMA
// with pinned register classes did not change that.  SEAM_W24_NT=2 enables it for experiments.
inline int wino24_nt(int K, int C, long blocks_nt1) {
    // NT = 2 pays where the K loop is long enough to amortise a block that is alone on its CU (C >= 256) and the launch still fills
    // the chip several times over with half as many blocks (measured per layer shape with tools/w24_ab.py; both forms compute
    // bit-identical results, so the choice may depend on the batch).  SEAM_W24_NT=1|2 forces a form.
    const int force = seam_opt::get(seam_opt::W24_NT);
    if (K % 64) return 1;
    if (force == 1 || force == 2) return force;
    // round 5: on the producer / consumer kernel the shorter K loops of the C = 64 / 128 layers pay as well (80 x 100^2 x 128: -6 %)
    const int pc = seam_opt::get(seam_opt::W24_PC);
    const int cmin = pc && C % 64 == 0 ? 64 : 256;
    return (C >= cmin && blocks_nt1 / 2 >= 1024) ? 2 : 1;
}

// XCD groups the n-tiles are split over (1 = every XCD walks all n-tiles of its patches).  Default off until measured per shape.
inline int wino24_nsplit(int C, int K, long patch_blocks) {
    (void)C; (void)K; (void)patch_blocks;
    return 1;
}

// the producer / consumer kernel takes the NT = 2 launches (SEAM_W24_PC=0: conv3x3_wino24<2>, the round-4 kernel, stays selectable)
inline bool wino24_pc(const Wino24Args& a) {
    const int want = seam_opt::get(seam_opt::W24_PC);
    return want && a.nt == 2 && a.nsplit == 1 && a.nchunks >= 8 && a.nchunks % 8 == 0;
}

// force_nt: 0 = the n-tiles per block by wino24_nt's rule, 1 | 2 = that form (conv3x3_wino24sx is always the two n-tile block)
// nsplit_rule: the XCD groups wanted for (C, K, patch blocks); the fp32 kernels keep wino24_nsplit, conv3x3_wino24sx brings its own
// tiles: if given, the tiles of the launch (patch blocks x n-tiles) -- `blocks` is the grid, which an n-tile split pads
inline int wino24_plan(Wino24Args& a, int N, int H, int W, int C, int K, int pad, long& blocks, int force_nt = 0,
                       int (*nsplit_rule)(int, int, long) = wino24_nsplit, long* tiles = nullptr) {
    if (!wino_ok(C, K, 3, 3, 1) || N <= 0) return (int)hipErrorInvalidValue;
    a.N = N; a.H = H; a.W = W; a.C = C; a.K = K;
    a.Ho = H + 2 * pad - 2; a.Wo = W + 2 * pad - 2; a.pad = pad;
    if (a.Ho <= 0 || a.Wo <= 0) return (int)hipErrorInvalidValue;
    if ((size_t)H * W * C * 4 >= kOob || (size_t)a.Ho * a.Wo * K * 4 >= kOob) return (int)hipErrorInvalidValue;
    const int tiles_x = (a.Wo + 3) / 4, tiles_y = (a.Ho + 1) / 2;
    const Layout pp = choose_layout(F24, N, tiles_x, tiles_y, (size_t)H * W * C * 4, (size_t)a.Ho * a.Wo * K * 4, kOob);
    a.nt = force_nt ? force_nt : wino24_nt(K, C, pp.blocks * (K / 32));
    a.tiles_n = K / (32 * a.nt);
    a.nchunks = C / 8;
    set_layout(a, pp, tiles_y);
    if (tiles) *tiles = pp.blocks * a.tiles_n;
    blocks = split_ntiles(a, pp.blocks, nsplit_rule(C, K, pp.blocks));
    if (blocks >= (1L << 24)) return (int)hipErrorInvalidValue;
    // fdivu numerator bounds: a tile index (< blocks + grid, grid < 2^16) by tiles_n, a block's j by tns; tm by per_img; rb < per_img
    // by bx; stacked: a tile row R < (tm + 1) * TY by tiles_y, a patch row (< 2^15 + pitch) by pitch; a slot id, patch pixel (< 2^16)
    // by TX, PW
    {
        using seam_fastdiv::exact;
        const unsigned long long tile_max = (unsigned long long)blocks + (1ull << 16), tm_max = tile_max / a.tiles_n + 1;
        bool ok = exact(a.tiles_n, tile_max) && exact(a.tns, tile_max) && exact(a.per_img, tm_max);
        if (a.stack) ok = ok && exact(tiles_y, (tm_max + 1) * a.TY[0]) && exact(2 * tiles_y + 2, (1ull << 15) + 2 * tiles_y + 2);
        for (int r = 0; r < 3; ++r)
            ok = ok && exact(a.bx[r], a.per_img) && exact(a.TX[r], 1ull << 16) && exact(4 * a.TX[r] + 2, 1ull << 16);
        if (!ok) return (int)hipErrorInvalidValue;
    }
    using seam_fastdiv::magic;
    a.m_tns = magic(a.tns);
    a.m_tiles_n = magic(a.tiles_n); a.m_per_img = magic(a.per_img); a.m_tys = magic(tiles_y); a.m_pitch = magic(2 * tiles_y + 2);
    for (int r = 0; r < 3; ++r) { a.m_bx[r] = magic(a.bx[r]); a.m_TX[r] = magic(a.TX[r]); a.m_PW[r] = magic(4 * a.TX[r] + 2); }
    return 0;
}

}  // namespace
