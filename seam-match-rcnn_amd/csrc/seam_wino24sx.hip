// seam_wino24sx.hip -- Winograd F(2x4,3x3) convolution with its 24 position GEMMs as six-term split-bf16 products on the gfx950
// bf16 matrix cores (v_mfma_f32_32x32x16_bf16): conv3x3_wino24sx.
//
// The transform algebra, the block geometry, the raw patch in LDS and the epilogue are those of conv3x3_wino24<2> (seam_wino24.hip;
// the shared code is seam_wino24_common.h, w24_block<2, HS, SX = true>): one block of four waves per CU, wave xi owns the positions
// (xi, nu = 0..5) x 32 tiles x 2 n-tiles of 32 output channels -- 192 accumulators in AccVGPRs --, computes its own A operands from
// the raw patch (no operand goes through LDS) and streams its weights from global memory into a register ring.  Only the K loop
// differs: M_p[tile, n] = sum_c V_p[tile, c] * U_p[n, c] runs as fp32-grade products of bf16 pieces instead of fp32 MFMAs.
//
// Arithmetic (the contract):
//   V     computed in fp32 with conv3x3_wino24's transform expressions (scalar-lane fmas; the packed form gives the same results),
//         per lane for its tile and its four channels of each of the two 8-channel chunks of a k-step: the values of conv3x3_wino24.
//   split each V value is cut into three bf16 pieces by split3_bf16 (truncation; top16 kept opaque, seam_split.h).  U is cut at pack
//         time from the fp32 value wino24_item produces (fp64 arithmetic, one rounding to fp32, then the exact three-way cut): the
//         three planes of U sum back to that fp32 value bit for bit.
//   k     a k-step is 16 channels.  Lane (tile, h = lane >> 5) holds k slots 8h .. 8h + 7: slots 0-3 are channels 16 s + 4 h + e of
//         the first chunk, slots 4-7 channels 16 s + 8 + 4 h + e of the second.  The pack uses the same map: nothing is shuffled
//         across lanes.
//   terms per accumulator tile and k-step the piece products (activation piece, weight piece) go (2,0) (1,1) (0,2) (1,0) (0,1) (0,0);
//         k-steps ascend; accumulators start from zero; the MFMA's A operand is V (rows = tiles), as in conv3x3_wino24.
//   epilogue  output transform, scale / shift, residual and ReLU are conv3x3_wino24's code, 16-byte stores.
//   special values  below 2^-110 the low pieces are lost; Inf / NaN give NaN (as conv_igemm_sx, seam_conv.hip).
//
// K loop, per wave and k-step: 72 MFMAs (6 positions x 2 n-tiles x 6 terms).  The A planes are a single rolling set: as soon as a
// position's twelve MFMAs are issued its planes are overwritten with the next k-step's (positions 3, 4 alternate between two sets
// by k-step parity, so nothing is carried across the k-step boundary).  The transform + split of k-step s + 1 -- twelve patch reads
// per chunk, 48 fmas of the row transform, then per position the column expressions and the three-way cut -- is handed to the
// scheduler in six parts, one beside each position's MFMAs, with an MFMA : VALU interleave pattern (one MFMA, up to six plain
// VALU instructions; none packed).  Weights: a ring of three positions (3 x 2 n-tiles x 3 planes x 16 bytes per lane); the slot a
// position frees is refilled right behind its MFMAs with the position three places on, i.e. 24 MFMAs ahead of its use.  The raw
// patch is four LDS buffers (two k-steps x two chunks); k-step s + 2's patch, requested one k-step earlier, is stored at the top of
// k-step s, and k-step s + 3's is requested right behind.  One barrier per k-step that waits for LDS traffic only.
#include <hip/hip_runtime.h>
#include "seam_device.h"
#include <stdint.h>
#include <stdlib.h>
#include <atomic>
#include "seam_fastdiv.h"
#include "seam_launch.h"
#include "seam_opts.h"
#include "seam_pack_items.h"
#include "seam_split.h"
#include "seam_wino24_common.h"

namespace {

// four raw patch buffers; the epilogue's exchange array (64 KiB) reuses the same memory after the K loop
constexpr int SX_EXB = 4 * 4 * 32 * 32 * 4;
constexpr int SX_LDS = 4 * RAWB > SX_EXB ? 4 * RAWB : SX_EXB;
static_assert(SX_LDS <= 160 * 1024 && RAWB % 16 == 0, "LDS map");

__global__ __launch_bounds__(256, 1) void conv3x3_wino24sx(const Wino24Args p) {
    extern __shared__ __attribute__((aligned(16))) char sx_smem[];
    w24_tile<2, true>(p, sx_smem);
}

// OIHW fp32 [K, Cin, 3, 3] -> the three bf16 planes of U = G2 g G4t in fragment order [K/32][C/16][24][3][64][8]
__global__ void wino24sx_pack_kernel(const float* __restrict__ w, unsigned short* __restrict__ out, int K, int Cin, int Cstore, int mode) {
    const int nks = Cstore / 16;
    const size_t total = (size_t)(K / 32) * nks * 64;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
        seam_pack::wino24sx_item(w, out, i, K, Cin, nks, mode);
}

// what conv3x3_wino24pc takes today: C a multiple of 64 from 64 on, K a multiple of 64, stride 1, pad 0 | 1
inline bool wino24sx_ok(int C, int K, int stride, int pad) {
    return stride == 1 && (pad == 0 || pad == 1) && C >= 64 && C % 64 == 0 && K >= 64 && K % 64 == 0 && (long long)K * C * 144 < (1ll << 31);
}

// XCD groups the n-tiles are split over (w24_tile's decode; every value gives the same bits).  seam_conv3x3_wino24sx_set_nsplit(1 |
// 2 | 4 | 8) forces one (a process-wide int of this launcher, like the selectors of seam_opts.h; it is not one of them because their
// number is pinned); wino24_plan reduces it until it divides the n-tiles.  The rule is 1 everywhere: measured with 1 / 2 / 4 on the ten
// shapes of a step at 80 and 40 frames and on one and two images, no shape wins beyond its spreads (80 x 200^2 x 256 -> 256: 9544 ->
// 9557 -> 9517 us), although two groups take a fifth of the L2 misses and of the fetched bytes away: seven of eight requests hit
// already (profiles/w24sx_l2_layer_ab.txt, profiles/w24sx_l2_pmc.txt).
std::atomic<int> g_force_nsplit{0};          // 0: the rule
int wino24sx_nsplit(int C, int K, long patch_blocks) {
    const int force = g_force_nsplit.load(std::memory_order_relaxed);
    if (force > 0) return force;
    (void)C; (void)K; (void)patch_blocks;
    return 1;
}

// blocks: the grid (with the padding blocks of an n-tile split); tiles: patch blocks x n-tiles, whatever the split
int wino24sx_plan(Wino24Args& a, int N, int H, int W, int C, int K, int pad, int stride, long& blocks, long* tiles = nullptr) {
    if (!wino24sx_ok(C, K, stride, pad)) return (int)hipErrorInvalidValue;
    return wino24_plan(a, N, H, W, C, K, pad, blocks, 2, wino24sx_nsplit, tiles);
}

}  // namespace

extern "C" {

long long seam_wino24sx_weight_bytes(int K, int C) { return (long long)K * C * 144; }

int seam_pack_conv_weight_wino24_sx(const float* w, void* u_packed, int K, int Cin, int Cstore, int mode, void* stream) {
    if (!wino24sx_ok(Cstore, K, 1, 1) || Cin > Cstore || Cin <= 0) return (int)hipErrorInvalidValue;
    const size_t total = (size_t)(K / 32) * (Cstore / 16) * 64;
    hipLaunchKernelGGL(wino24sx_pack_kernel, dim3(seam_launch::grid256(total)), dim3(256), 0, (hipStream_t)stream, w,
                       (unsigned short*)u_packed, K, Cin, Cstore, mode);
    return (int)hipGetLastError();
}

int seam_conv3x3_wino24sx_supported(int N, int H, int W, int C, int K, int pad, int stride) {
    Wino24Args a;
    long blocks;
    return wino24sx_plan(a, N, H, W, C, K, pad, stride, blocks) == 0 ? 1 : 0;
}

/* XCD groups of the n-tile split: 0 = the launcher's rule (default), 1 | 2 | 4 | 8 forced; any other value is refused */
int seam_conv3x3_wino24sx_set_nsplit(int nsplit) {
    if (nsplit != 0 && nsplit != 1 && nsplit != 2 && nsplit != 4 && nsplit != 8) return (int)hipErrorInvalidValue;
    g_force_nsplit.store(nsplit, std::memory_order_relaxed);
    return 0;
}

int seam_conv3x3_wino24sx_get_nsplit(void) { return g_force_nsplit.load(std::memory_order_relaxed); }

/* tiles of the launch (one block each, one per CU at a time; the padding blocks of an n-tile split are not counted, so the number
   does not depend on the forced split); 0 = unsupported.  ops.w24sx_map_ok asks it for ONE image. */
long long seam_conv3x3_wino24sx_blocks(int N, int H, int W, int C, int K, int pad) {
    Wino24Args a;
    long blocks, work = 0;
    return wino24sx_plan(a, N, H, W, C, K, pad, 1, blocks, &work) == 0 ? (long long)work : 0;
}

/* The block layout of a launch, read from the Wino24Args the launcher would launch with (sx = 0: seam_conv3x3_wino24_f32's plan,
   sx = 1: this file's, under the currently forced split).  out[24]: nreg, stack, G, PH, nt, tiles_n, nsplit, per_img, TX[3], TY[3],
   bx[3], by[3], patch blocks (all images, per n-tile), grid blocks (patch blocks x n-tiles plus the padding blocks of an n-tile
   split; the producer / consumer form walks that many tiles with a persistent grid).  Regions past nreg are 0.  Returns
   hipErrorInvalidValue, writing nothing, for a shape the launcher refuses. */
int seam_wino24_layout(int N, int H, int W, int C, int K, int pad, int sx, int* out) {
    Wino24Args a;
    long blocks;
    if (!out || (sx != 0 && sx != 1)) return (int)hipErrorInvalidValue;
    const int rc = sx ? wino24sx_plan(a, N, H, W, C, K, pad, 1, blocks) : wino24_plan(a, N, H, W, C, K, pad, blocks);
    if (rc) return rc;
    const int head[8] = {a.nreg, a.stack, a.G, a.PH, a.nt, a.tiles_n, a.nsplit, a.per_img};
    for (int i = 0; i < 8; ++i) out[i] = head[i];
    for (int r = 0; r < 3; ++r) {
        const bool used = r < a.nreg;
        out[8 + r] = used ? a.TX[r] : 0;
        out[11 + r] = used ? a.TY[r] : 0;
        out[14 + r] = used ? a.bx[r] : 0;
        out[17 + r] = used ? a.by[r] : 0;
    }
    out[20] = (int)patch_blocks(a);
    out[21] = (int)blocks;
    out[22] = out[23] = 0;
    return 0;
}

int seam_conv3x3_wino24sx_f32(const float* x, const void* u_packed, const float* scale, const float* shift, const float* residual,
                              float* y, int N, int H, int W, int C, int K, int pad, int stride, int relu, void* stream) {
    Wino24Args a;
    long blocks;
    const int rc = wino24sx_plan(a, N, H, W, C, K, pad, stride, blocks);
    if (rc) return rc;
    a.x = x; a.u = (const float*)u_packed; a.scale = scale; a.shift = shift; a.res = residual; a.y = y;
    a.relu = relu;
    a.trace = nullptr;
    a.total_tiles = 0;
    const hipError_t e = seam_launch::prepare<conv3x3_wino24sx>(SX_LDS);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(conv3x3_wino24sx, dim3((unsigned)blocks), dim3(256), SX_LDS, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // extern "C"
