// seam_pwsx.hip -- pointwise (1x1, stride 1, pad 0) convolution, fp32 in / fp32 out, as six-term three-plane split-bf16 products
// (the arithmetic of conv_igemm_sx<.., 6>, seam_conv.hip) on a PRODUCER / CONSUMER block persistent over its XCD's tiles: the
// structure of conv1x1_f16pc (seam_pwhpc.hip) with the fp32 16-byte epilogue of conv1x1_pc (seam_pwpc.hip).  It serves the long
// 1x1 layers of the fp32 path's split classes: the bottleneck reductions (512 / 1024 / 2048 -> 128 / 256 / 512) and the plain
// expansions with their residual (256 -> 1024, 512 -> 2048).
//
// Why.  conv_igemm_sx is bound by exposed load latency (profiles/split_f32_tile_and_ablation.txt: 333-389 us shipped, 229 us without
// global loads, 162 us MFMAs + epilogue on 40 x 50^2, 1024 -> 256): all four waves of its block gather, split, store to LDS, meet at
// a barrier and multiply in turn, one wave per SIMD.  Here
//   * a block owns 128 pixels (consecutive rows of the [M, C] activation matrix) x 128 output channels per tile;
//   * waves 4..7 (producers) copy the tile's rows, 64 channels (one 256-byte run per pixel, 16 adjacent lanes per run) per chunk,
//     global -> registers -> split3_bf16 -> LDS (two LDS buffers, two more chunks in registers), across tile boundaries; their
//     per-lane offsets are launch invariants, a tile changes one descriptor; every interval issues the same 8 loads (without a chunk:
//     an empty descriptor), so hipcc's vmcnt bookkeeping is exact;
//   * waves 0..3 (consumers, one per SIMD) only multiply: wave w owns channels 32 w .. 32 w + 31 of the tile for all 128 pixels (4
//     accumulator tiles).  Per k-step of 16: twelve `ds_read_b128` (three planes x four 32-pixel groups: lane = pixel, 16 bytes = 8
//     consecutive k, the upper lanes 8 k further) and three 1-KiB global loads (the wave's three weight planes in fragment order, a
//     register ring four k-steps deep) feed 24 MFMAs; addresses are per-lane bases + immediates: no VALU in the k-steps (the chunk
//     loop swaps its two buffer pointers, three v_mov per 96 MFMAs).  One barrier
//     per chunk (96 MFMAs per wave), inside the chunk's LAST k-step: that step's fragments were read a step earlier, so behind the
//     barrier the consumers read the next chunk's first fragments under their own MFMAs and run from chunk to chunk -- and from a
//     tile's epilogue into the next tile -- without a stop, while the producers put chunk c + 2 over chunk c;
//   * the MFMA's operand roles are swapped (rows = channels, columns = pixels), so a lane ends with four consecutive channels of one
//     pixel per register quad; the epilogue is conv1x1_pc's: a wave-private LDS transpose into rows (8 lanes per pixel), scale /
//     shift, plain residual, ReLU, 16-byte stores of full 128-byte lines, no barrier.  The epilogue vectors and the residual pieces of three
//     of the four pixel groups are requested before the tile's last chunk, the fourth group's at the epilogue's start (all four
//     ahead spill registers).  Store offsets stay in the vector register (the SGPR-offset hazard).
// Arithmetic: bit for bit conv_igemm_sx<.., 6>: the same 16 k-values per MFMA in the same element positions, k-steps ascending,
// within a k-step the six piece products of an accumulator tile in its order (activation piece, weight piece) = (2,0) (1,1) (0,2)
// (1,0) (0,1) (0,0), every accumulator tile starts from zero; the products are exact, so which operand is the MFMA's A is immaterial.
//
// The two-source form conv1x1_sxpc_dual (sxpc_body<true>) runs the projection-shortcut blocks, bn3(conv3(h)) + bn_d(conv_d(x)), as one
// reduction over [x1 | x2 sampled at stride2]: only the producers differ.  A tile's first C1 / 64 chunks are its rows of x1 as above;
// the others are the pixels (n, stride2 ho, stride2 wo) of x2 through a second descriptor, rebased per tile at the first image the
// tile touches, and eight per-lane offsets recomputed once per tile; per chunk a scalar branch picks the source, the same eight loads
// on either side.  Weights, consumers and epilogue are the plain kernel's on the [K, C1 + C2] matrix; the bits are those of the plain
// kernel on the concatenated rows.
//
// The upsampled-residual form conv1x1_sxpc_up (sxpc_body<false, true>) runs the FPN's lateral 1x1 with its nearest top-down merge:
// conv(x) * scale + shift, + top[n, nearest_src(ho), nearest_src(wo), :], ReLU.  Only the source of the epilogue's 16 residual pieces
// per lane differs from the plain kernel.  The PRODUCERS compute the byte offset of each of the tile's 128 pixels in the coarse map
// (one pixel per thread pair: the image by the two-source form's multiply-high rules, ho / wo by multiply-high, two
// seam_fpn::nearest_src) and put them into a 512-byte LDS table with the store of the tile's first chunk; the consumers read it at
// the tile's last chunk, which any chunk barrier in between orders; two tables by tile parity (a table is rewritten two tiles later,
// behind a barrier the consumers reach only in the next tile).  The table's layout is [pixel & 7][pixel group][i], so the row-layout
// lane fetches one pixel group's four offsets with one ds_read_b128 right before that group's four loads.  The coarse map's
// descriptor is rebased per tile at the first image the tile touches (its index travels behind the table), so lane offsets stay 32-bit.
// The bits are those of the plain kernel (scale, shift) followed by seam_upsample_add_f32 and ReLU.
//
// K = 64 (sxpc_body<.., NG = 2>): conv1x1_sxpc64 is the same block on tiles of 128 pixels x 64 output channels.  The consumers map two
// by two so that all four SIMDs multiply: wave w owns channels 32 (w & 1) of pixels 64 (w >> 1), two accumulator tiles; per k-step six
// ds_read_b128, three 1-KiB weight loads, twelve MFMAs in the same term order; the pack is the same fragment order with two n-tiles
// (6 K C bytes); the epilogue is the same, per wave over its two pixel groups.  C is a multiple of 64 from 128 on.  stem_sxpc
// (sxpc_body<true, false, 2, true>) is its gather form for the ResNet stem, the 4x4 / stride-1 convolution over the 12-channel
// space-to-depth frame with its zero cells, [N, Hs + 3, Ws + 3, 12]: an output pixel's reduction is 192 = 4 tap rows x 48 contiguous
// floats, three chunks of 64.  Only the producers differ: every chunk comes through the two-source form's second descriptor (no first
// source); the thread's eight pixel offsets are computed once per tile as there; piece q = 16 j + (ptid & 15) of chunk j adds
// (q / 12) row_step + (q % 12) 16, three launch invariants per lane.  The bits are those of conv1x1_sxpc64 on the gathered [M, 192] rows.
//
// The `short` entries launch conv1x1_sxpc / conv1x1_sxpc_dual on two chunks per tile (C = 128; C1 = C2 = 64): see sxpc_plan.
//
// LDS map (139264 bytes, one block per CU; the upsampled-residual form: + 1056):
//   [0, 102400)        two chunk buffers of 128 pixel rows x 400 bytes: plane 0 | plane 1 | plane 2 (64 bf16 = 128 bytes each) | 16
//                      bytes of padding -- 25 slots of 16 bytes, odd, so the 16 lanes of a ds_read_b128 cycle (16 consecutive
//                      pixels) meet 16 different bank groups
//   [102400, 139264)   per consumer wave two transpose buffers of 32 pixels x (32 channels + 16 bytes)
//   [139264, 140320)   (conv1x1_sxpc_up) two tables of 128 coarse-map byte offsets + the tile's first image (16 bytes)
#include <hip/hip_runtime.h>
#include "seam_device.h"
#include <stdint.h>
#include <algorithm>
#include <type_traits>
#include "seam_fastdiv.h"
#include "seam_fpn_common.h"
#include "seam_launch.h"
#include "seam_pack_items.h"
#include "seam_split.h"

namespace {

constexpr int BM = 128;                     // pixels per tile
constexpr int CK = 64;                      // channels per chunk
constexpr int KS = CK / 16;                 // k-steps (one MFMA depth) per chunk
constexpr int PLB = CK * 2;                 // bytes of one plane of a pixel's chunk
constexpr int ROWB = 3 * PLB + 16;          // LDS bytes per pixel and chunk: 25 slots
constexpr int ABUF = BM * ROWB;             // 51200
constexpr int NP = BM * (CK / 4) / 256;     // 16-byte fp32 pieces per producer thread and chunk: 8
constexpr int TROW = 128 + 16;              // wave-private transpose rows: 32 pixels x (32 channels + 16 bytes)
constexpr int TBUF = 32 * TROW;             // 4608 bytes
constexpr int TR0 = 2 * ABUF;
constexpr int LDS_BYTES = TR0 + 4 * 2 * TBUF;
static_assert(LDS_BYTES <= 160 * 1024 && ABUF + 3 * PLB < 65536 && 4 * 32 * ROWB < 65536, "LDS map / ds immediates");
constexpr int TBLB = BM * 4 + 16;           // conv1x1_sxpc_up: one offset table (128 pixels) + the index of the tile's first image
constexpr int TBL0 = LDS_BYTES;
constexpr int LDS_UP_BYTES = LDS_BYTES + 2 * TBLB;
static_assert(LDS_UP_BYTES <= 160 * 1024, "LDS map of the upsampled-residual form");
constexpr int RB = 4;                       // k-steps of weight fragments in flight per consumer wave (= KS: the ring slot of a k-step is its index in the chunk)
static_assert(RB == KS, "ring slot = k-step of the chunk");
constexpr int RVA = 3;                      // pixel groups whose residual pieces are requested before the tile's last chunk (the fourth: at the
                                            // epilogue's start; 4 spills 6 registers, 3 leaves 242 VGPRs and no scratch)

#ifndef SEAM_SXPC_ABL
#define SEAM_SXPC_ABL 0     // timing-only experiments: 1 no row staging, 2 no in-loop weight loads, 4 no split VALU, 8 no in-loop A reads
#endif

struct SxpcArgs {
    const float* x;        // [M, C]
    const void* w;         // packed: [K/128][4 n-tiles][C/16 k-steps][3 planes][64 lanes][8 bf16]
    const float* scale;    // [K] or null
    const float* shift;    // [K] or null
    const float* res;      // [M, K] or null
    float* y;              // [M, K]
    int M, C, K, relu;
    int tiles_n, nchunks, total_tiles;
    unsigned m_tiles_n;
};

// The second source of the dual form (conv1x1_sxpc_dual): chunks [0, n1) of a tile are its 128 consecutive rows of x = x1 [M, C1],
// chunks [n1, nchunks) the pixels (n, stride2 ho, stride2 wo) of x2 [N, H2, W2, C2]; SxpcArgs::C = C1 + C2 (the consumers' reduction).
// A second source is addressed per output pixel (n, ho, wo) of the [N, Ho, Wo] grid; its fields but the pointer, C1 and n1 are filled
// by sxpc_src_plan and read by sxpc_pixel, for SxpcUp under the same names.
struct SxpcDual {
    const float* x2;
    unsigned long long img_bytes;       // H2 * W2 * C2 * 4
    int N, C1, n1;
    unsigned HoWo, Wo;
    // row rl of the first image's output grid (rl < BM + HoWo) -> image rl / HoWo = umulhi(rl, m_howo) + rl * one_howo + (rl >= thr):
    // HoWo = 1: (0, 1, never); 2 <= HoWo < BM: (magic, 0, never); HoWo >= BM (at most two images): (0, 0, HoWo).  No branch, any map.
    unsigned m_howo, one_howo, thr;
    unsigned m_wo, one_wo;              // the remainder by Wo: umulhi(rem, m_wo) + rem * one_wo
    unsigned img_step, row_step, px_step;      // byte steps of x2 per image / per output row (stride2 W2 C2 4) / per output pixel (stride2 C2 4)
};

// The coarse map of the upsampled-residual form (conv1x1_sxpc_up): output pixel (n, ho, wo) adds top[n, nearest_src(ho), nearest_src(wo), :]
struct SxpcUp {
    const float* top;                   // [N, rH, rW, K]
    unsigned long long img_bytes;       // rH * rW * K * 4
    int N, Ho, Wo, rH, rW;
    unsigned HoWo;
    unsigned m_howo, one_howo, thr;     // a row of the tile's image span -> its image: SxpcDual's rules
    unsigned m_wo, one_wo;              // the remainder by Wo
    unsigned img_step, row_step, px_step;      // byte steps of top per image / per coarse row (rW K 4) / per coarse pixel (K 4)
};

// row rl (< BM + HoWo) of the output grid of the first image a tile touches -> (image, ho, wo), by the multiply-high rules above
template <class Src>
__device__ __forceinline__ void sxpc_pixel(const Src& s, const unsigned rl, unsigned& nl, unsigned& ho, unsigned& wo) {
    nl = __umulhi(rl, s.m_howo) + rl * s.one_howo + (rl >= s.thr ? 1u : 0u);
    const unsigned rem = rl - nl * s.HoWo;
    ho = __umulhi(rem, s.m_wo) + rem * s.one_wo;
    wo = rem - ho * s.Wo;
}

// NG: 32-pixel groups (accumulator tiles) per consumer wave.  4: the forms above, 128 output channels per tile, wave w = channels
// 32 w of all 128 pixels.  2: the 64-output-channel forms (see "K = 64" below), wave w = channels 32 (w & 1) of pixels 64 (w >> 1).
// STEM (with DUAL, NG = 2): every chunk comes from the second source, a 4 x 4 window of the padded space-to-depth frame.
template <bool DUAL, bool UP = false, int NG = 4, bool STEM = false>
__device__ __forceinline__ void sxpc_body(const SxpcArgs& p, const SxpcDual& d, const SxpcUp& u = SxpcUp{}) {
    static_assert((NG == 4 || NG == 2) && (!STEM || (DUAL && NG == 2)) && !(UP && NG != 4), "forms of sxpc_body");
    constexpr int BN = 32 * (NG == 4 ? 4 : 2);          // output channels per tile
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool consumer = wave < 4;
    const int n = p.nchunks;

    // ---- the block's tiles (tile = m-tile * tiles_n + n-tile: the n-tiles of a row block are neighbours -- the second one finds the
    // rows in the L2) ----
    const XcdTiles xt = xcd_tiles(p.total_tiles);
    const int ntiles = xt.ntiles, S = xt.stride;
    if (ntiles == 0) return;
    const int tile0 = xt.tile0();
    const int c1 = STEM ? 0 : DUAL ? d.C1 : p.C;     // channels of a row of x
    const size_t row_bytes = (size_t)c1 * 4, out_row = (size_t)p.K * 4;
    const int total_chunks = ntiles * n;

    if (!consumer) {
        // =================================================== producer ===================================================
        const int ptid = tid - 256;
        unsigned goff[NP];                      // byte offset of piece (ptid & 15) of tile row (ptid >> 4) + 16 r: launch invariants
        LDSQ char* lp[NP];                      // LDS address of the piece's plane 0 in chunk buffer 0
#pragma unroll
        for (int r = 0; r < NP; ++r) {
            const int row = (ptid >> 4) + 16 * r;
            goff[r] = (unsigned)(row * c1 * 4 + (ptid & 15) * 16);
            lp[r] = (LDSQ char*)smem + row * ROWB + (ptid & 15) * 8;
        }
        f32x4 rq[2][NP];                        // two chunks in registers (chunk parity)
        // the REQUEST stage: chunk ck of tile `tile`; rows past M have no records in the tile's descriptor and read as zeros; past the
        // block's last tile the descriptor is empty (the loads are issued all the same: see the header)
        int tile = tile0, ck = 0, tiles_left = ntiles;
        auto x_desc = [&](const int tl) {
            const int tm = fdivu(tl, p.tiles_n, p.m_tiles_n);
            const int row0 = tm * BM;
            const int rows = tiles_left > 0 ? min(BM, p.M - row0) : 0;
            return __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)p.x + (size_t)(tiles_left > 0 ? row0 : 0) * row_bytes), 0,
                                                     (int)(rows * row_bytes), 0x00020000);
        };
        __amdgpu_buffer_rsrc_t rs = x_desc(tile);
        // DUAL: the second source of tile tl -- its descriptor, rebased at the first image the tile touches (32-bit lane offsets for
        // any x2; the plan has checked that the images of one tile fit the descriptor), and this thread's eight pixel offsets: once
        // per tile, nothing per chunk.  Rows past M get kOob; past the block's last tile the descriptor is empty.
        unsigned goff2[DUAL ? NP : 1];
        __amdgpu_buffer_rsrc_t rs2;
        auto x2_tile = [&](const int tl) {
            const bool live = tiles_left > 0;
            const unsigned row0 = live ? (unsigned)fdivu(tl, p.tiles_n, p.m_tiles_n) * BM : 0u;
            const unsigned n_first = __builtin_amdgcn_readfirstlane(row0 / d.HoWo);       // (a true division: once per tile, any M)
            const unsigned long long left = (unsigned long long)((unsigned)d.N - n_first) * d.img_bytes;
            rs2 = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)d.x2 + (size_t)n_first * d.img_bytes), 0,
                                                    live ? (int)(left > kOob ? kOob : (unsigned)left) : 0, 0x00020000);
            const unsigned rl0 = row0 - n_first * d.HoWo + (unsigned)(ptid >> 4);      // row inside that image's output grid
#pragma unroll
            for (int r = 0; r < NP; ++r) {
                unsigned nl, ho, wo;
                sxpc_pixel(d, rl0 + 16 * r, nl, ho, wo);
                const unsigned off = nl * d.img_step + ho * d.row_step + wo * d.px_step + (STEM ? 0u : (unsigned)((ptid & 15) * 16));
                goff2[r] = row0 + (unsigned)(ptid >> 4) + 16 * r < (unsigned)p.M ? off : kOob;
            }
        };
        if (DUAL) x2_tile(tile);
        // STEM: piece q = 16 ck + (ptid & 15) of a pixel's 192-float window lies (q / 12) frame rows down, 16 (q % 12) bytes in:
        // three launch invariants per lane
        unsigned tap[STEM ? 3 : 1] = {};
        if constexpr (STEM) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const unsigned q = 16u * j + (unsigned)(ptid & 15);
                tap[j] = (q / 12u) * d.row_step + (q % 12u) * 16u;
            }
        }
        auto request = [&](f32x4 (&dst)[NP]) {
            if constexpr (STEM) {
                const unsigned tj = ck == 0 ? tap[0] : ck == 1 ? tap[1] : tap[2];
#pragma unroll
                for (int r = 0; r < NP; ++r)        // (a row past M: kOob + tj stays out of every descriptor)
                    dst[r] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs2, (SEAM_SXPC_ABL & 1) ? kOob : goff2[r] + tj, 0, 0));
            } else if (!DUAL || ck < d.n1) {
#pragma unroll
                for (int r = 0; r < NP; ++r)
                    dst[r] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (SEAM_SXPC_ABL & 1) ? kOob : goff[r], ck * (CK * 4), 0));
            } else {                            // (a scalar branch: the same eight loads on either side)
#pragma unroll
                for (int r = 0; r < NP; ++r)
                    dst[r] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs2, (SEAM_SXPC_ABL & 1) ? kOob : goff2[r], (ck - d.n1) * (CK * 4), 0));
            }
            if (++ck == n) {                    // the next request belongs to the next tile
                ck = 0;
                tile += S;
                --tiles_left;
                rs = x_desc(tile);
                if (DUAL) x2_tile(tile);
            }
        };
        // UP: the offset table of tile tl (see the header): pixel ptid >> 1 of the tile, written by the even thread of the pair
        int st_tile = tile0, st_ck = 0, st_left = ntiles, st_par = 0;      // the STORE stage's tile / chunk (the request stage runs ahead)
        const float fh = UP ? (float)u.rH / (float)u.Ho : 0.f, fw = UP ? (float)u.rW / (float)u.Wo : 0.f;
        auto up_table = [&](const int tl, const int par) {
            const unsigned row0 = (unsigned)fdivu(tl, p.tiles_n, p.m_tiles_n) * BM;
            const unsigned n_first = __builtin_amdgcn_readfirstlane(row0 / u.HoWo);       // (a true division: once per tile, any M)
            const unsigned r = (unsigned)ptid >> 1;
            unsigned nl, ho, wo;
            sxpc_pixel(u, row0 - n_first * u.HoWo + r, nl, ho, wo);       // row inside that image's output grid: < BM + HoWo
            const unsigned hs = (unsigned)seam_fpn::nearest_src((int)ho, fh, u.rH), ws = (unsigned)seam_fpn::nearest_src((int)wo, fw, u.rW);
            const unsigned off = nl * u.img_step + hs * u.row_step + ws * u.px_step;
            LDSQ char* const tb = (LDSQ char*)smem + TBL0 + par * TBLB;
            if (!(ptid & 1))
                *reinterpret_cast<unsigned LDSQ*>(tb + ((r & 7) * 16 + (r >> 5) * 4 + ((r >> 3) & 3)) * 4) = row0 + r < (unsigned)p.M ? off : kOob;
            if (ptid == 0) *reinterpret_cast<unsigned LDSQ*>(tb + BM * 4) = n_first;
        };
        auto store_chunk = [&](const f32x4 (&src)[NP], const int buf) {
            if constexpr (UP) {                 // with a tile's first chunk: its table (past the block's last tile: none)
                if (st_ck == 0 && st_left > 0) up_table(st_tile, st_par);
                if (++st_ck == n) {
                    st_ck = 0;
                    st_tile += S;
                    --st_left;
                    st_par ^= 1;
                }
            }
            if (SEAM_SXPC_ABL & 1) return;
#pragma unroll
            for (int r = 0; r < NP; ++r) {
                u32x2 q0, q1, q2;
                if (SEAM_SXPC_ABL & 4) {
                    q0[0] = __builtin_bit_cast(unsigned, src[r][0]); q0[1] = __builtin_bit_cast(unsigned, src[r][1]);
                    q1[0] = __builtin_bit_cast(unsigned, src[r][2]); q1[1] = __builtin_bit_cast(unsigned, src[r][3]); q2 = q0;
                } else {
                    split3_bf16_single(src[r], q0, q1, q2);    // producer waves beside the consumers' MFMAs: nothing packed
                }
                *reinterpret_cast<u32x2 LDSQ*>(lp[r] + buf * ABUF) = q0;
                *reinterpret_cast<u32x2 LDSQ*>(lp[r] + buf * ABUF + PLB) = q1;
                *reinterpret_cast<u32x2 LDSQ*>(lp[r] + buf * ABUF + 2 * PLB) = q2;
            }
        };
        // chunk c (counted over the block's tiles) lives in LDS buffer c & 1 and travels through register set c & 1.  The consumers
        // pass the barrier of chunk c (B_c) in its last k-step: before it the producers have stored chunk c + 1, behind it nobody
        // reads chunk c's buffer any more and it takes chunk c + 2.
        request(rq[0]);                         // chunk 0
        request(rq[1]);                         // chunk 1
        store_chunk(rq[0], 0);
        request(rq[0]);                         // chunk 2
        LDS_BAR();                              // P: chunk 0 visible
        for (int c = 0; c < total_chunks; c += 2) {
            store_chunk(rq[1], 1);              // chunk c + 1
            request(rq[1]);                     // chunk c + 3
            LDS_BAR();                          // B_c
            if (c + 1 >= total_chunks) break;
            store_chunk(rq[0], 0);              // chunk c + 2
            request(rq[0]);                     // chunk c + 4
            LDS_BAR();                          // B_{c+1}
        }
    } else {
        // =================================================== consumer ===================================================
        const int wn = NG == 4 ? wave : wave & 1;       // this wave's 32-channel n-tile of the block's BN
        const int pg = NG == 4 ? 0 : wave >> 1;         // ... and (NG = 2) its half of the tile's pixels
        f32x16 acc[NG];
        f32x4 af[3][NG];                        // [plane][pixel group]: the A fragments of the current k-step
        f32x4 bf[RB][3];                        // [ring slot][plane]: the wave's weight fragments
        // the lane's pixel (group 0) at k-half lane >> 5, plane 0, in the chunk buffer ...; groups, planes and k-steps are immediates
        const LDSQ char* ac = (const LDSQ char*)smem + (lane & 31) * ROWB + (lane >> 5) * 16 + pg * (NG * 32 * ROWB);      // ... of the current chunk
        const LDSQ char* an = ac + ABUF;                                                            // ... of the next one
        const int nsteps = p.C >> 4;
        const int wtile_bytes = nsteps * 3072;  // one n-tile's weights: C / 16 k-steps x three 1-KiB planes
        const int blane = lane * 16;
        __amdgpu_buffer_rsrc_t w_rsrc;
        int tm_n = 0, tn_n = 0;                 // m-tile / n-tile of the tile whose weights are in the ring
        auto load_b = [&](const int slot, const int step) {
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
                bf[slot][pl] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(w_rsrc, blane, (step * 3 + pl) * 1024, 0));
        };
        auto ring_preload = [&](const int tl) {
            tm_n = fdivu(tl, p.tiles_n, p.m_tiles_n);
            tn_n = __builtin_amdgcn_readfirstlane(tl - tm_n * p.tiles_n);
            tm_n = __builtin_amdgcn_readfirstlane(tm_n);
            w_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)p.w + (size_t)(tn_n * (BN / 32) + wn) * wtile_bytes), 0, wtile_bytes, 0x00020000);
#pragma unroll
            for (int s = 0; s < RB; ++s) { SB(); load_b(s, s); }
            SB();
        };
        // The epilogue's row layout (after the wave-private transpose): lane -> pixel (lane >> 3) + 8 i of a 32-pixel group, 16-byte piece
        // (lane & 7) of the wave's 32 channels: eight lanes write one pixel's 128 bytes -- a full line per pixel.
        const unsigned ooff = (unsigned)(((lane >> 3) + pg * (NG * 32)) * p.K * 4 + (32 * wn + 4 * (lane & 7)) * 4);
        LDSQ char* const tw = (LDSQ char*)smem + TR0 + wave * (2 * TBUF) + (lane & 31) * TROW + (lane >> 5) * 16;   // accumulator layout: piece 2 qd + h
        const LDSQ char* const tr = (const LDSQ char*)smem + TR0 + wave * (2 * TBUF) + (lane >> 3) * TROW + (lane & 7) * 16;
        const int K32 = 32 * p.K * 4, K8 = 8 * p.K * 4;        // byte steps of a 32-pixel group / of 8 pixels
        const LDSQ char* const tbr = (const LDSQ char*)smem + TBL0 + (lane >> 3) * 64;       // UP: this lane's pixel row of the offset table
        int tpar = 0;                           // ... of the current tile (tile parity)
        int tile = tile0;
        ring_preload(tile);
        constexpr int RV = RVA < NG ? RVA : NG;      // pixel groups whose residual pieces travel under the tile's last chunk
        f32x4 rv[NG][4], sc, sh;
        LDS_BAR();                              // P: chunk 0 is in LDS
        for (int k = 0; k < ntiles; ++k) {
            const int tm_k = tm_n, tn_k = tn_n;             // (wave-uniform by construction)
            const int rows = min(BM, p.M - tm_k * BM);
            const __amdgpu_buffer_rsrc_t y_rsrc = __builtin_amdgcn_make_buffer_rsrc(
                (void*)((char*)p.y + (size_t)tm_k * BM * out_row), 0, (int)(rows * out_row), 0x00020000);
            const __amdgpu_buffer_rsrc_t r_rsrc = __builtin_amdgcn_make_buffer_rsrc(
                (void*)((const char*)(p.res ? p.res : p.y) + (size_t)tm_k * BM * out_row), 0, (int)(rows * out_row), 0x00020000);
            const unsigned ocol = ooff + (unsigned)(tn_k * (BN * 4));
            const unsigned ccol = (unsigned)(tn_k * (BN * 4) + 128 * wn) + (unsigned)((lane & 7) * 16);      // UP: the lane's piece inside a coarse pixel
            __amdgpu_buffer_rsrc_t t_rsrc = y_rsrc;         // UP: the coarse map from the tile's first image on (set at the last chunk)
            // UP: pixel group m's residual pieces through the tile's offset table (rows past M: kOob, zeros)
            auto up_request = [&](const int m) {
                const u32x4 to = *reinterpret_cast<const u32x4 LDSQ*>(tbr + tpar * TBLB + m * 16);
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    rv[m][i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(t_rsrc, to[i] + ccol, 0, 0));
            };
            // the tile's first fragments (a tile's last chunk reads them ahead like every chunk, but they are not kept across the
            // epilogue, which needs the registers)
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
#pragma unroll
                for (int m = 0; m < NG; ++m) af[pl][m] = *reinterpret_cast<const f32x4 LDSQ*>(ac + m * (32 * ROWB) + pl * PLB);
            for (int t = 0; t < n; ++t) {
                const bool last = t == n - 1;
                if (last) {
                    // the tile's epilogue vectors (this lane's four channels in the row layout) without a branch of their own (a
                    // missing vector reads the weights instead and is replaced by 1 / 0), and the residual pieces of the first RVA
                    // pixel groups (row layout): in flight under the tile's last chunk
                    const int ch = tn_k * BN + 32 * wn + 4 * (lane & 7);
                    const f32x4 a = *reinterpret_cast<const f32x4*>((p.scale ? p.scale : (const float*)p.w) + ch);
                    const f32x4 b = *reinterpret_cast<const f32x4*>((p.shift ? p.shift : (const float*)p.w) + ch);
                    sc = a;                     // (replaced in the epilogue: a select here would wait for the loads at once)
                    sh = b;
                    if constexpr (UP) {
                        const unsigned n_first = __builtin_amdgcn_readfirstlane(*reinterpret_cast<const unsigned LDSQ*>((const LDSQ char*)smem + TBL0 + tpar * TBLB + BM * 4));
                        const unsigned long long left = (unsigned long long)((unsigned)u.N - n_first) * u.img_bytes;
                        t_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)u.top + (size_t)n_first * u.img_bytes), 0,
                                                                   (int)(left > kOob ? kOob : (unsigned)left), 0x00020000);
#pragma unroll
                        for (int m = 0; m < RV; ++m) up_request(m);
                    } else if (p.res) {
#pragma unroll
                        for (int m = 0; m < RV; ++m)
#pragma unroll
                            for (int i = 0; i < 4; ++i)
                                rv[m][i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r_rsrc, ocol + m * K32 + i * K8, 0, 0));
                    }
                }
                auto read_a = [&](const int pl, const int m, const int ks) -> f32x4 {       // ks = KS: the next chunk's first fragments
                    return *reinterpret_cast<const f32x4 LDSQ*>((ks == KS ? an : ac + ks * 32) + m * (32 * ROWB) + pl * PLB);
                };
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    // (activation piece, weight piece) by descending i + j: entries 3..8 of conv_igemm_sx's T9
                    constexpr int TA[6] = {2, 1, 0, 1, 0, 0}, TB[6] = {0, 1, 2, 0, 1, 0};
                    constexpr int LAST[3] = {5, 3, 0};      // the term after which plane pa's fragments of this k-step are history
#pragma unroll
                    for (int tq = 0; tq < 6; ++tq) {
                        const int pa = TA[tq], pb = TB[tq];
                        if (ks == KS - 1 && tq == 1) {
                            // B_c: the next chunk is in the other buffer; this one (read to its end a k-step ago) may be overwritten
                            SB();
                            LDS_BAR();
                            SB();
#if !(SEAM_SXPC_ABL & 8)
#pragma unroll
                            for (int m = 0; m < NG; ++m) af[2][m] = read_a(2, m, KS);
#endif
                        }
#pragma unroll
                        for (int m = 0; m < NG; ++m) {
                            SB();
                            // roles swapped: rows = output channels (the weight fragment), columns = pixels (the activation fragment)
                            if (ks == 0 && tq == 0 && t == 0) {     // the tile's first step multiplies into a constant zero: no accumulator clears
                                const f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                                acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, bf[ks][pb]), __builtin_bit_cast(bf16x8, af[pa][m]), z, 0, 0, 0);
                            } else {
                                acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, bf[ks][pb]), __builtin_bit_cast(bf16x8, af[pa][m]), acc[m], 0, 0, 0);
                            }
                            SB();
#if !(SEAM_SXPC_ABL & 8)
                            // the next k-step's fragment of this plane and group, behind the plane's last product of this k-step
                            if (tq == LAST[pa] && !(ks == KS - 1 && tq == 0)) af[pa][m] = read_a(pa, m, ks + 1);
#endif
                        }
                    }
                    SB();
#if !(SEAM_SXPC_ABL & 2)
                    load_b(ks, min(t * KS + ks + RB, nsteps - 1));      // (past the tile's end: its last step again, never used)
#endif
                }
                SB();
                // the buffers change roles (three v_mov per chunk of 96 MFMAs; the k-steps themselves have no vector-ALU instruction)
                const LDSQ char* const sw = ac;
                ac = an;
                an = sw;
            }
            // ---- epilogue, in registers ----
            tile += S;
            ring_preload(tile);                 // the next tile's first weight fragments: in flight under the arithmetic (past the
                                                // block's last tile: a tile that is never multiplied -- inside the pack, or dropped)
            if (!p.scale) sc = f32x4{1.f, 1.f, 1.f, 1.f};
            if (!p.shift) sh = f32x4{0.f, 0.f, 0.f, 0.f};
            auto finish_tile = [&](auto res_c, auto relu_c) {    // flags as compile-time constants: four straight-line copies
                constexpr bool RES = decltype(res_c)::value, RELU = decltype(relu_c)::value;
                if (RES) {
#pragma unroll
                    for (int m = RV; m < NG; ++m)   // the pixel groups the last chunk had no registers for
                        if constexpr (UP) {
                            up_request(m);
                        } else {
#pragma unroll
                            for (int i = 0; i < 4; ++i)
                                rv[m][i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r_rsrc, ocol + m * K32 + i * K8, 0, 0));
                        }
                    // (one wait for everything that came from memory, before the first store)
#pragma unroll
                    for (int m = 0; m < NG; ++m) asm volatile("" :: "v"(rv[m][0]), "v"(rv[m][1]), "v"(rv[m][2]), "v"(rv[m][3]));
                }
                // accumulator layout (lane = pixel, register quad = 4 consecutive channels) -> this wave's private [32 pixels][32 channels]
                // rows (two buffers: group m + 1 is written before group m is read back) -> row layout: 8 lanes per pixel
                auto put = [&](const int m) {
#pragma unroll
                    for (int qd = 0; qd < 4; ++qd)
                        *reinterpret_cast<f32x4 LDSQ*>(tw + (m & 1) * TBUF + qd * 32) =
                            f32x4{acc[m][4 * qd], acc[m][4 * qd + 1], acc[m][4 * qd + 2], acc[m][4 * qd + 3]};
                };
                put(0);
#pragma unroll
                for (int m = 0; m < NG; ++m) {
                    if (m + 1 < NG) put(m + 1);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        f32x4 v = *reinterpret_cast<const f32x4 LDSQ*>(tr + (m & 1) * TBUF + i * (8 * TROW));
                        v = v * sc + sh;                    // (no scale: sc = 1 -- the same value as v + sh)
                        if (RES) v += rv[m][i];
                        if (RELU) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
                        }
                        // (vector offset + immediate only: with a SCALAR offset hipcc puts the next piece's arithmetic right behind a
                        // 16-byte store without the wait state its data registers need)
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), y_rsrc, ocol + m * K32 + i * K8, 0, 0);
                    }
                }
            };
            if (UP || p.res) {
                if (p.relu) finish_tile(std::true_type{}, std::true_type{}); else finish_tile(std::true_type{}, std::false_type{});
                if constexpr (UP) tpar ^= 1;
            } else {
                if (p.relu) finish_tile(std::false_type{}, std::true_type{}); else finish_tile(std::false_type{}, std::false_type{});
            }
        }
    }
}

__global__ __launch_bounds__(512, 2) void conv1x1_sxpc(const SxpcArgs p) { sxpc_body<false>(p, SxpcDual{}); }
__global__ __launch_bounds__(512, 2) void conv1x1_sxpc_dual(const SxpcArgs p, const SxpcDual d) { sxpc_body<true>(p, d); }

// [K, C] fp32 (row-major) -> three bf16 planes in fragment order [K/128][4][C/16][3][64][8]
__global__ void sxpc_pack_kernel(const float* __restrict__ w, unsigned short* __restrict__ out, int K, int C) {
    const size_t total = (size_t)K * C / 8;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
        seam_pack::sxpc_item(w, out, i, C);
}

// (behind the pack kernel: the existing kernels keep their place in the module)
__global__ __launch_bounds__(512, 2) void conv1x1_sxpc_up(const SxpcArgs p, const SxpcUp u) { sxpc_body<false, true>(p, SxpcDual{}, u); }

// (behind the existing kernels, like conv1x1_sxpc_up)  K = 64: the 64-output-channel form and the stem as its gather form
__global__ __launch_bounds__(512, 2) void conv1x1_sxpc64(const SxpcArgs p) { sxpc_body<false, false, 2>(p, SxpcDual{}); }
__global__ __launch_bounds__(512, 2) void stem_sxpc(const SxpcArgs p, const SxpcDual d) { sxpc_body<true, false, 2, true>(p, d); }

// min_c: 256 for the entries above; 128 for the `short` entries (two chunks per tile: the body's pipeline is counted in chunks
// over the block's tiles, the weight ring's look-ahead is clamped to the tile, the residual requests go out in the last chunk
// whichever it is -- nothing in it needs a third chunk)
int sxpc_plan(SxpcArgs& a, long long M, int C, int K, int min_c = 256) {
    if (M <= 0 || C < min_c || (C % CK) || K < 128 || (K % 128)) return 1;
    if ((unsigned long long)BM * C * 4 >= kOob || (unsigned long long)BM * K * 4 >= kOob) return 1;
    if ((unsigned long long)(C / 16) * 3072 >= kOob) return 1;
    const long long tiles_m = (M + BM - 1) / BM;
    const long long total = tiles_m * (K / 128);
    if (total >= (1LL << 24) || M >= (1LL << 31)) return 1;
    a.M = (int)M; a.C = C; a.K = K;
    a.tiles_n = K / 128; a.nchunks = C / CK; a.total_tiles = (int)total;
    // (the producers and the ring preload run one grid stride past the block's last tile: numerators below 2 * total + 2^16)
    if (!seam_fastdiv::exact(a.tiles_n, 2ull * total + (1ull << 16))) return 1;
    a.m_tiles_n = seam_fastdiv::magic(a.tiles_n);
    return 0;
}

// The geometry of a second source (Src: SxpcDual or SxpcUp) under the [N, Ho, Wo] output grid: one image of it is `pixels` x px_bytes
// bytes; output pixel (n, ho, wo) lies img_bytes n + row_step ho + px_step wo bytes in (the upsampled-residual form: ho, wo through
// nearest_src first).
template <class Src>
int sxpc_src_plan(Src& s, long long N, long long Ho, long long Wo, unsigned long long pixels, unsigned long long px_bytes,
                  unsigned long long row_step, unsigned long long px_step) {
    const long long HoWo = Ho * Wo;
    if (pixels >= (1ull << 31) / px_bytes) return 1;        // one image of the source inside a descriptor
    const unsigned long long img = pixels * px_bytes;
    // a tile's 128 rows touch at most this many images; their pixels are addressed from the first one's start with 32-bit offsets
    const unsigned long long imgs = std::min<unsigned long long>((unsigned long long)N, (unsigned long long)((BM - 2) / HoWo + 2));
    if (imgs * img > kOob) return 1;
    // divisions of the producers: a row of the tile's image span by HoWo (by multiply-high for 2 <= HoWo < BM only: numerators
    // below BM + HoWo), its remainder by Wo
    const bool mid = HoWo >= 2 && HoWo < BM;
    if (mid && !seam_fastdiv::exact((unsigned long long)HoWo, (unsigned long long)(BM + HoWo))) return 1;
    if (!seam_fastdiv::exact((unsigned long long)Wo, (unsigned long long)HoWo)) return 1;
    s.img_bytes = img;
    s.N = (int)N; s.HoWo = (unsigned)HoWo; s.Wo = (decltype(s.Wo))Wo;
    s.m_howo = mid ? seam_fastdiv::magic((unsigned long long)HoWo) : 0u;
    s.one_howo = HoWo == 1 ? 1u : 0u;
    s.thr = HoWo >= BM ? (unsigned)HoWo : 0xffffffffu;
    s.m_wo = seam_fastdiv::magic((unsigned long long)Wo);       // (0 for Wo = 1)
    s.one_wo = Wo == 1 ? 1u : 0u;
    // (a step that exceeds 32 bits multiplies an index that is always 0: Ho = 1 / Wo = 1 with a large stride)
    s.img_step = (unsigned)img; s.row_step = (unsigned)row_step; s.px_step = (unsigned)px_step;
    return 0;
}

// the dual form: the plain plan of (M, C1 + C2, K) and x2's pixels (n, stride2 ho, stride2 wo) as the second source
int sxpc_dual_plan(SxpcArgs& a, SxpcDual& d, long long N, long long Ho, long long Wo, int C1, long long H2, long long W2, int C2, int stride2, int K,
                   int min_c = 256) {
    if (N <= 0 || Ho <= 0 || Wo <= 0 || H2 <= 0 || W2 <= 0 || C1 < CK || C2 < CK || (C1 % CK) || (C2 % CK) || stride2 < 1) return 1;
    if (N >= (1LL << 31) || Ho >= (1LL << 31) || Wo >= (1LL << 31) || H2 >= (1LL << 31) || W2 >= (1LL << 31)) return 1;
    if ((Ho - 1) * stride2 >= H2 || (Wo - 1) * stride2 >= W2) return 1;
    if (Ho * Wo >= (1LL << 31) || N * (Ho * Wo) >= (1LL << 31)) return 1;
    if (sxpc_plan(a, N * Ho * Wo, C1 + C2, K, min_c)) return 1;
    d.C1 = C1; d.n1 = C1 / CK;
    return sxpc_src_plan(d, N, Ho, Wo, (unsigned long long)H2 * W2, (unsigned long long)C2 * 4,
                         (unsigned long long)stride2 * W2 * C2 * 4, (unsigned long long)stride2 * C2 * 4);
}

// the upsampled-residual form: the plain plan of (N Ho Wo, C, K) and the coarse map as the second source
int sxpc_up_plan(SxpcArgs& a, SxpcUp& u, long long N, long long Ho, long long Wo, int C, int K, long long rH, long long rW) {
    if (N <= 0 || Ho <= 0 || Wo <= 0 || rH <= 0 || rW <= 0) return 1;
    if (N >= (1LL << 31) || Ho >= (1LL << 24) || Wo >= (1LL << 24) || rH >= (1LL << 24) || rW >= (1LL << 24)) return 1;     // (nearest_src: indices exact in fp32)
    if (Ho * Wo >= (1LL << 31) || N * (Ho * Wo) >= (1LL << 31)) return 1;
    if (sxpc_plan(a, N * Ho * Wo, C, K)) return 1;
    u.Ho = (int)Ho; u.rH = (int)rH; u.rW = (int)rW;
    return sxpc_src_plan(u, N, Ho, Wo, (unsigned long long)rH * rW, (unsigned long long)K * 4, (unsigned long long)rW * K * 4, (unsigned long long)K * 4);
}

// the 64-output-channel form: one n-tile of 64 channels, two chunks per tile at the least (one chunk is refused: untested, unused)
int sxpc64_plan(SxpcArgs& a, long long M, int C, int K) {
    if (M <= 0 || K != 64 || C < 2 * CK || (C % CK)) return 1;
    if ((unsigned long long)BM * C * 4 >= kOob || (unsigned long long)(C / 16) * 3072 >= kOob) return 1;
    const long long total = (M + BM - 1) / BM;
    if (total >= (1LL << 24) || M >= (1LL << 31)) return 1;
    a.M = (int)M; a.C = C; a.K = K;
    a.tiles_n = 1; a.nchunks = C / CK; a.total_tiles = (int)total;
    a.m_tiles_n = 0;        // (fdivu's d == 1 branch)
    return 0;
}

// the stem: sxpc64_plan of (N Hs Ws, 192, 64) and the padded frame [N, Hs + 3, Ws + 3, 12] as SxpcDual's second source (no first one)
int stem_sxpc_plan(SxpcArgs& a, SxpcDual& d, long long N, long long Hs, long long Ws) {
    if (N <= 0 || Hs <= 0 || Ws <= 0 || N >= (1LL << 31) || Hs >= (1LL << 31) - 3 || Ws >= (1LL << 31) - 3) return 1;
    if (Hs * Ws >= (1LL << 31) || N * (Hs * Ws) >= (1LL << 31)) return 1;
    if (sxpc64_plan(a, N * Hs * Ws, 192, 64)) return 1;
    d.C1 = 0; d.n1 = 0;
    return sxpc_src_plan(d, N, Hs, Ws, (unsigned long long)(Hs + 3) * (Ws + 3), 48, (unsigned long long)((Ws + 3) * 48), 48);
}

// the launch entries' common tail: the I/O fields of a planned SxpcArgs ...
void sxpc_io(SxpcArgs& a, const float* x, const void* w_packed, const float* scale, const float* shift, const float* res, float* y, int relu) {
    a.x = x; a.w = w_packed; a.scale = scale; a.shift = shift; a.res = res; a.y = y; a.relu = relu;
}

// ... and the launch: one persistent block per CU, at most one per tile
template <auto Kernel, class... Extra>
int sxpc_launch(int lds_bytes, void* stream, const SxpcArgs& a, const Extra&... extra) {
    int ncu;
    const hipError_t e = seam_launch::prepare<Kernel>(lds_bytes, &ncu);
    if (e != hipSuccess) return (int)e;
    const unsigned grid = (unsigned)(a.total_tiles > ncu ? ncu : a.total_tiles);
    hipLaunchKernelGGL(Kernel, dim3(grid), dim3(512), lds_bytes, (hipStream_t)stream, a, extra...);
    return (int)hipGetLastError();
}

// the pack entries' launch, behind each entry's own rule for (C, K)
int sxpc_pack(const float* w, void* w_packed, int K, int C, void* stream) {
    const size_t total = (size_t)K * C / 8;
    hipLaunchKernelGGL(sxpc_pack_kernel, dim3(seam_launch::grid256(total)), dim3(256), 0, (hipStream_t)stream, w, (unsigned short*)w_packed, K, C);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

/* 1 when seam_conv1x1_sxpc takes this layer (1x1 / stride 1 / pad 0; C >= 256 and a multiple of 64; K a multiple of 128; M >= 1), else 0 */
int seam_conv1x1_sxpc_supported(long long M, int C, int K) {
    SxpcArgs a;
    return sxpc_plan(a, M, C, K) == 0 ? 1 : 0;
}

long long seam_conv1x1_sxpc_weight_bytes(int K, int C) { return (long long)K * C * 6; }

/* w: [K, C] fp32 row-major (a 1x1 OIHW weight) -> the kernel's three bf16 planes in fragment order */
int seam_pack_conv1x1_weight_sxpc(const float* w, void* w_packed, int K, int C, void* stream) {
    SxpcArgs a;
    if (sxpc_plan(a, 1, C, K)) return (int)hipErrorInvalidValue;      // the kernel's own rule for (C, K)
    return sxpc_pack(w, w_packed, K, C, stream);
}

/* y[M, K] = act(scale * (x[M, C] . w^T) + shift + residual), fp32 in / out, six-term split-bf16 products: the bits of seam_conv2d_sx
 * with terms = 6 on the same 1x1 layer; relu 0 | 1 */
int seam_conv1x1_sxpc(const float* x, const void* w_packed, const float* scale, const float* shift, const float* residual, float* y,
                      long long M, int C, int K, int relu, void* stream) {
    SxpcArgs a;
    if ((relu != 0 && relu != 1) || sxpc_plan(a, M, C, K)) return (int)hipErrorInvalidValue;
    sxpc_io(a, x, w_packed, scale, shift, residual, y, relu);
    return sxpc_launch<conv1x1_sxpc>(LDS_BYTES, stream, a);
}

/* 1 when the channel counts and M of a two-source layer suit seam_conv1x1_sxpc_dual (C1, C2 multiples of 64; the plain rule for
 * (M, C1 + C2, K)), else 0; the launch checks the geometry as well */
int seam_conv1x1_sxpc_dual_supported(long long M, int C1, int C2, int K) {
    SxpcArgs a;
    if (C1 < CK || C2 < CK || (C1 % CK) || (C2 % CK) || (long long)C1 + C2 >= (1LL << 30)) return 0;
    return sxpc_plan(a, M, C1 + C2, K) == 0 ? 1 : 0;
}

/* y[N, Ho, Wo, K] = act(scale * ([x1 | x2 at (stride2 ho, stride2 wo)] . w^T) + shift): the bits of seam_conv1x1_sxpc on the
 * concatenated rows, which are never written; w_packed: seam_pack_conv1x1_weight_sxpc of [K, C1 + C2]; relu 0 | 1 */
int seam_conv1x1_sxpc_dual(const float* x1, const float* x2, const void* w_packed, const float* scale, const float* shift, float* y,
                           int N, int Ho, int Wo, int C1, int H2, int W2, int C2, int stride2, int K, int relu, void* stream) {
    SxpcArgs a;
    SxpcDual d;
    if ((relu != 0 && relu != 1) || !x2 || sxpc_dual_plan(a, d, N, Ho, Wo, C1, H2, W2, C2, stride2, K)) return (int)hipErrorInvalidValue;
    sxpc_io(a, x1, w_packed, scale, shift, nullptr, y, relu);
    d.x2 = x2;
    return sxpc_launch<conv1x1_sxpc_dual>(LDS_BYTES, stream, a, d);
}

/* 1 when seam_conv1x1_sxpc_up takes this lateral: the plain rule for (M, C, K), M == N Ho Wo, rH, rW >= 1 and the geometry rules of
 * the launch (the coarse images one tile touches within 2 GiB, exact multiply-high divisions); else 0.  Wo == 1 and 1 x 1 maps are served. */
int seam_conv1x1_sxpc_up_supported(long long M, int N, int Ho, int Wo, int C, int K, int rH, int rW) {
    SxpcArgs a;
    SxpcUp u;
    if (N <= 0 || Ho <= 0 || Wo <= 0 || M != (long long)N * Ho * Wo) return 0;
    return sxpc_up_plan(a, u, N, Ho, Wo, C, K, rH, rW) == 0 ? 1 : 0;
}

/* y[N, Ho, Wo, K] = act(scale * (x[N Ho Wo, C] . w^T) + shift + top[n, nearest(ho), nearest(wo), :]): the bits of seam_conv1x1_sxpc
 * (scale, shift) followed by seam_upsample_add_f32 and ReLU; top [N, rH, rW, K]; relu 0 | 1 */
int seam_conv1x1_sxpc_up(const float* x, const void* w_packed, const float* scale, const float* shift, const float* top, float* y,
                         int N, int Ho, int Wo, int C, int K, int rH, int rW, int relu, void* stream) {
    SxpcArgs a;
    SxpcUp u;
    if ((relu != 0 && relu != 1) || !top || sxpc_up_plan(a, u, N, Ho, Wo, C, K, rH, rW)) return (int)hipErrorInvalidValue;
    sxpc_io(a, x, w_packed, scale, shift, nullptr, y, relu);
    u.top = top;
    return sxpc_launch<conv1x1_sxpc_up>(LDS_UP_BYTES, stream, a, u);
}

/* The `short` entries: conv1x1_sxpc / conv1x1_sxpc_dual on two-chunk reductions, C == 128 / C1 == C2 == 64 with stride2 == 1 */
int seam_conv1x1_sxpc_short_supported(long long M, int C, int K) {
    SxpcArgs a;
    return C == 2 * CK && sxpc_plan(a, M, C, K, 2 * CK) == 0 ? 1 : 0;
}

int seam_pack_conv1x1_weight_sxpc_short(const float* w, void* w_packed, int K, int C, void* stream) {
    if (!seam_conv1x1_sxpc_short_supported(1, C, K)) return (int)hipErrorInvalidValue;
    return sxpc_pack(w, w_packed, K, C, stream);
}

int seam_conv1x1_sxpc_short(const float* x, const void* w_packed, const float* scale, const float* shift, const float* residual, float* y,
                            long long M, int C, int K, int relu, void* stream) {
    SxpcArgs a;
    if ((relu != 0 && relu != 1) || C != 2 * CK || sxpc_plan(a, M, C, K, 2 * CK)) return (int)hipErrorInvalidValue;
    sxpc_io(a, x, w_packed, scale, shift, residual, y, relu);
    return sxpc_launch<conv1x1_sxpc>(LDS_BYTES, stream, a);
}

int seam_conv1x1_sxpc_dual_short_supported(long long M, int C1, int C2, int K) {
    SxpcArgs a;
    return C1 == CK && C2 == CK && sxpc_plan(a, M, C1 + C2, K, 2 * CK) == 0 ? 1 : 0;
}

int seam_conv1x1_sxpc_dual_short(const float* x1, const float* x2, const void* w_packed, const float* scale, const float* shift, float* y,
                                 int N, int Ho, int Wo, int C1, int H2, int W2, int C2, int K, int relu, void* stream) {
    SxpcArgs a;
    SxpcDual d;
    if ((relu != 0 && relu != 1) || !x2 || C1 != CK || C2 != CK || sxpc_dual_plan(a, d, N, Ho, Wo, C1, H2, W2, C2, 1, K, 2 * CK))
        return (int)hipErrorInvalidValue;
    sxpc_io(a, x1, w_packed, scale, shift, nullptr, y, relu);
    d.x2 = x2;
    return sxpc_launch<conv1x1_sxpc_dual>(LDS_BYTES, stream, a, d);
}

/* 1 when seam_conv1x1_sxpc64 takes this layer (1x1 / stride 1 / pad 0; K == 64; C >= 128 and a multiple of 64; M >= 1), else 0 */
int seam_conv1x1_sxpc64_supported(long long M, int C, int K) {
    SxpcArgs a;
    return sxpc64_plan(a, M, C, K) == 0 ? 1 : 0;
}

/* w: [64, C] fp32 row-major -> the three bf16 planes in seam_conv1x1_sxpc's fragment order with two 32-channel n-tiles: 6 K C bytes */
int seam_pack_conv1x1_weight_sxpc64(const float* w, void* w_packed, int K, int C, void* stream) {
    SxpcArgs a;
    if (sxpc64_plan(a, 1, C, K)) return (int)hipErrorInvalidValue;
    return sxpc_pack(w, w_packed, K, C, stream);
}

/* y[M, 64] = act(scale * (x[M, C] . w^T) + shift + residual): seam_conv1x1_sxpc's arithmetic (the bits of seam_conv2d_sx with
 * terms = 6) for 64 output channels; w_packed: seam_pack_conv1x1_weight_sxpc64; relu 0 | 1 */
int seam_conv1x1_sxpc64(const float* x, const void* w_packed, const float* scale, const float* shift, const float* residual, float* y,
                        long long M, int C, int K, int relu, void* stream) {
    SxpcArgs a;
    if ((relu != 0 && relu != 1) || sxpc64_plan(a, M, C, K)) return (int)hipErrorInvalidValue;
    sxpc_io(a, x, w_packed, scale, shift, residual, y, relu);
    return sxpc_launch<conv1x1_sxpc64>(LDS_BYTES, stream, a);
}

/* 1 when seam_stem_sxpc takes the frame geometry (N frames of Hs x Ws space-to-depth cells), else 0 */
int seam_stem_sxpc_supported(int N, int Hs, int Ws) {
    SxpcArgs a;
    SxpcDual d;
    return stem_sxpc_plan(a, d, N, Hs, Ws) == 0 ? 1 : 0;
}

/* The ResNet stem as the 4x4 / stride-1 convolution over the space-to-depth frame: xp [N, Hs + 3, Ws + 3, 12] fp32 is the frame
 * with its zero cells (2 before, 1 after, both directions), y [N, Hs, Ws, 64] = act(scale * (window . w^T) + shift) with the window
 * of an output pixel its 4 x 4 cells in (r, s, c) order: the bits of seam_conv1x1_sxpc64 on the gathered [N Hs Ws, 192] rows.
 * w_packed: seam_pack_conv1x1_weight_sxpc64 of the [64, 192] rows; relu 0 | 1 */
int seam_stem_sxpc(const float* xp, const void* w_packed, const float* scale, const float* shift, float* y, int N, int Hs, int Ws,
                   int relu, void* stream) {
    SxpcArgs a;
    SxpcDual d;
    if ((relu != 0 && relu != 1) || !xp || stem_sxpc_plan(a, d, N, Hs, Ws)) return (int)hipErrorInvalidValue;
    sxpc_io(a, xp, w_packed, scale, shift, nullptr, y, relu);
    d.x2 = xp;
    return sxpc_launch<stem_sxpc>(LDS_BYTES, stream, a, d);
}

}  // extern "C"
