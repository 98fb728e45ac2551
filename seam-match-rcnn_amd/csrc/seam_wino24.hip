// seam_wino24.hip -- Winograd F(2x4,3x3) convolution on the gfx950 fp32 matrix cores.
//
// The second Winograd kernel of the path: output tiles of 2 rows x 4 columns from 4 x 6 input tiles, i.e. F(2,3) down
// the rows (as seam_wino.hip) and F(4,3) along the columns: 24 multiplies per 8 outputs = 3 per output instead of
// 4 (F(2x2,3x3)) or 9 (direct) -- 3x fewer MFMA issues than the implicit GEMM, 1.33x fewer than seam_wino.hip.
//   Y = A2t [ (G2 g G4t) (.) (B2t d B4) ] A4   per tile, summed over input channels = 24 independent GEMMs
//   M_p[tile, n] = sum_c V_p[tile, c] * U_p[n, c],  p = (xi in 0..3, nu in 0..5), all fp32 (v_mfma_f32_32x32x2_f32).
// The F(4,3) half uses the points {0, +-1, +-2, inf}; its transforms multiply by 2, 4, 5, 8 (input / output side) and
// 1/4, 1/6, 1/12, 1/24 (weights, computed in fp64 at pack time and rounded once): measured rounding ~2x that of
// F(2x2,3x3), ~1e-6 of the output scale (tools/wino_bench.py).
//
// Mapping (same ideas as seam_wino.hip -- no operand goes through LDS):
//   block = 4 waves; wave xi owns the six positions (xi, nu = 0..5) for 32 tiles x 32 output channels: 6 accumulator
//   tiles of 32x32 (96 VGPRs), two blocks per CU.
//   A operand: each wave computes ITS row of B2t d (two input rows per column) and the six column combinations in
//     registers, directly in MFMA A-fragment layout, from the block's raw input patch -- the only LDS resident:
//     (2*TY+2) x (4*TX+2) pixels x 8 channels per chunk, split by channel half and by x mod 4 so that the tile-strided
//     ds_read_b128s are conflict free, double buffered, one barrier per 8-channel chunk.
//   B operand: U packed in fragment order [n_tile][chunk][p][lane][4]; a wave streams its 6 KiB per chunk with coalesced
//     buffer loads straight into registers.
//   Registers are the scarce resource (96 accumulators): A and B fragments are SINGLE sets that roll -- the positions are
//     walked in pairs (0,5), (1,2), (3,4) (the pairs that share sub-expressions of B4t); as soon as the 8 MFMAs of a
//     pair are issued, its A fragments are overwritten with those of the next chunk and its weight loads for the next
//     chunk are issued (16 MFMA slots ahead of their use).
//   Epilogue: the nu half of the output transform (A4t: 6 -> 4) in registers, the xi half (A2t: 4 -> 2) through a
//     32 KiB LDS exchange in two passes, scale / shift (+ residual, ReLU), 16-byte NHWC stores.
#include <hip/hip_runtime.h>
#include "seam_device.h"
#include <stdint.h>
#include <stdlib.h>
#include "seam_fastdiv.h"
#include "seam_launch.h"
#include "seam_opts.h"
#include "seam_pack_items.h"
#include "seam_wino24_common.h"
#if defined(SEAM_W24PC_TRACE)
#include "dev/seam_trace_host.h"      // -DSEAM_DEV_BUILD experiment builds only (tools/experiments/w24pc_abl.sh)
#endif
#include <type_traits>

namespace {

template <int NT>
__global__ __launch_bounds__(256, NT == 1 ? 2 : 1) void conv3x3_wino24(const Wino24Args p) {
    // two raw patch buffers; the epilogue's exchange array ex[xi][b][tile][n] (64 KiB, all four output columns of a tile in one
    // pass) reuses the same memory after the K loop
    constexpr int EXB = 4 * 4 * 32 * 32 * 4;
    static_assert(2 * RAWB <= EXB, "the raw buffers live inside the exchange array's 64 KiB");
    __shared__ __attribute__((aligned(16))) char smem[EXB];

    w24_tile<NT, false>(p, smem);
}

// =====================================================================================================================
// conv3x3_wino24pc (round 5): the NT = 2 block as a PRODUCER / CONSUMER pair of wave groups, two waves per SIMD, persistent.
//
// What round 4 measured on conv3x3_wino24<2>: the block is alone on its CU (one wave per SIMD, 490 registers), so everything that
// is not an MFMA is exposed -- the input transform, the patch loads / LDS stores, the waits behind them: ~17 % of every chunk plus a
// fixed 5.3 us per block.  What tools/probes/pc_probe.hip measured this round: beside a wave that streams fp32 MFMAs back to back,
// its SIMD partner's LDS, vector-memory and scalar instructions are free, but its VECTOR-ALU instructions do not issue at all until
// the matrix pipe idles (fp32 MFMA and fp32 VALU share the SIMD's FMA lanes).  So the work is split by role, and the one thing
// that has to share the pipe -- the 36 packed ops of a chunk's input transform -- is placed where the consumer yields anyway:
//   waves 0..3 (consumers, one per SIMD): MFMAs only.  Wave xi owns the positions (xi, nu = 0..5) x 32 tiles x 64 channels
//     (192 accumulators, all arch VGPRs: with 512 threads per block the budget is 256 registers and hipcc selects the VGPR
//     form of the MFMA).  A fragments come from LDS (`ds_read_b128`, one position ahead), B fragments straight from global
//     memory through a register ring (RING positions x 8 registers, refilled right behind the MFMAs that read them); the K loop
//     holds no vector-ALU instruction; the first k-step of a tile multiplies into a zero constant (no accumulator clears).
//   waves 4..7 (producers, the SIMD partners): a software pipeline over the block's chunk stream, one interval per consumer
//     chunk -- fragments of chunk t + 2 registers -> LDS V[t & 1]; raw patch of chunk t + 4 registers -> LDS raw[t & 1]; global
//     loads of chunk t + 6; LDS reads of chunk t + 3's raw patch (all free beside the MFMAs); then the 36 packed ops of chunk
//     t + 3, which run while the consumer waits at the chunk's barrier; then the barrier.  The pipeline runs ACROSS tiles: a block
//     is persistent (grid = CUs, XCD-contiguous tile ranges), the next tile's address set-up is computed nine intervals before
//     the current tile ends and the load / store / read stages switch over one by one, so a tile's prologue (first patch
//     latency, two transforms) disappears behind the previous tile's last chunks and epilogue.
//   One s_barrier per chunk, in the consumer between positions 4 and 5: it then holds the chunk's last fragment in registers
//     and requests the next chunk's first one under the eight MFMAs of position 5.
//   Epilogue: consumers run the nu half of the output transform into the exchange array (its own 64 KiB: the raw / V buffers hold
//     the next tile's data by then), all 512 threads finish (xi half, scale / shift / residual / ReLU, 16-byte stores).
// The arithmetic (transform expressions, accumulation order, epilogue) is that of conv3x3_wino24<2>: results are bit-identical.
// =====================================================================================================================
#ifndef SEAM_W24PC_ABL
#define SEAM_W24PC_ABL 0    // experiments: 1 no in-loop patch loads / stores (64: no stores only, 128: no requests only), 2 no in-loop weight loads, 8 no in-loop transforms, 16 no epilogue arithmetic,
                            // 256 (round 6, TIMING ONLY -- results are garbage): the weight fragments travel through LDS -- the producers issue
                            // them as LDS-DMA loads (buffer_load_dwordx4 ... lds) into the exchange region, the consumers read them with ds_read_b128
#endif
#ifndef SEAM_W24PC_RING
#define SEAM_W24PC_RING 4
#endif
#ifndef SEAM_W24PC_AD
#define SEAM_W24PC_AD 1
#endif
constexpr int PC_VB = 4 * 6 * 64 * 16;                 // bytes per V buffer
constexpr int PC_RAW = 0, PC_V = 2 * RAWB, PC_EX = 2 * RAWB + 2 * PC_VB;      // LDS map: raw[2] | V[2] | ex
constexpr int PC_EXB = 4 * 4 * 32 * 32 * 4;
constexpr int PC_LDS = PC_EX + PC_EXB;
static_assert((2 * RAWB) % 16 == 0 && PC_LDS <= 160 * 1024, "LDS map");

#ifdef SEAM_W24PC_TRACE      // debug: stamp (tag << 56 | s_memtime) into p.trace[wave * 4096 + k++] from lane 0 of the traced block
#define PC_TR(tag) SEAM_STAMP(4096, tag)
#else
#define PC_TR(tag) do { } while (0)
#endif

// wave-uniform geometry of one tile (SGPRs; recomputed from the tile index where it is needed rather than kept alive)
struct PcGeo {
    int tn, reg, n_img, n_here, R0, prow0, ty0, tx0, iy0, ix0, TX, PW, NPIX, HS, PR, NENT, nslots, tye, txe;
    unsigned m_TX, m_PW;
};
__device__ __forceinline__ PcGeo pc_geo(const Wino24Args& p, const int tile) {
    PcGeo g;
    const int tm = fdivu(tile, p.tiles_n, p.m_tiles_n);
    g.tn = tile - tm * p.tiles_n;
    const int tm_img = fdivu(tm, p.per_img, p.m_per_img);
    int rb = tm - tm_img * p.per_img;
    int reg = 0;
    const int c0 = p.rg[0].bx * p.rg[0].by, c1 = p.rg[1].bx * p.rg[1].by;
    if (p.nreg > 1 && rb >= c0) {
        rb -= c0;
        reg = 1;
        if (p.nreg > 2 && rb >= c1) { rb -= c1; reg = 2; }
    }
    g.reg = reg;
    const Wino24Args::Rg R = p.rg[reg];         // one 64-byte scalar load
    const int TX = R.TX, TY = R.TY;
    const int byi = fdivu(rb, R.bx, R.m_bx);
    const int bxi = rb - byi * R.bx;
    g.R0 = tm * TY;
    g.n_img = p.stack ? fdivu(g.R0, p.tiles_y, p.m_tys) : tm_img;
    g.prow0 = p.stack ? 2 * (g.R0 - g.n_img * p.tiles_y) : 0;
    g.n_here = min(p.G, p.N - g.n_img);
    g.ty0 = p.stack ? 0 : R.ry0 + byi * TY;
    g.tx0 = p.stack ? 0 : R.rx0 + bxi * TX;
    g.iy0 = 2 * g.ty0 - p.pad;
    g.ix0 = 4 * g.tx0 - p.pad;
    g.TX = TX;
    g.PW = 4 * TX + 2;
    const int PH = p.stack ? p.PH : 2 * TY + 2;
    g.NPIX = g.PW * PH;
    g.HS = (TX + 1) | 1;
    g.PR = 8 * g.HS + (TX & 7);
    const int NENT0 = g.PR * ((PH + 1) >> 1);
    g.NENT = NENT0 + ((4 - NENT0) & 7);
    g.nslots = TX * TY;
    g.m_TX = R.m_TX; g.m_PW = R.m_PW; g.tye = R.rye; g.txe = R.rxe;
    return g;
}
// tile slot id (0..31) of a block patch -> image-in-group g, tile row / column, first patch row; false for idle slots
__device__ __forceinline__ bool pc_slot(const Wino24Args& p, const PcGeo& q, int id, int& g, int& ty, int& tx, int& prow) {
    const int r = fdivu(id, q.TX, q.m_TX);
    tx = q.tx0 + (id - __mul24(r, q.TX));
    if (p.stack) {
        const int R = q.R0 + r;
        const int n = fdivu(R, p.tiles_y, p.m_tys);
        g = n - q.n_img;
        ty = R - __mul24(n, p.tiles_y);
        prow = __mul24(2 * p.tiles_y + 2, g) + 2 * ty - q.prow0;
        return id < q.nslots && n < p.N;
    }
    g = 0;
    ty = q.ty0 + r;
    prow = 2 * r;
    return id < q.nslots && ty < q.tye && tx < q.txe;
}

// second half of the epilogue for one n-tile (all 512 threads; consumers take the output columns 0, 1 of a tile, producers 2, 3).
// sc / sh: this thread's four channels of the epilogue vectors, requested by the caller ahead of the barrier in front of this call.
struct PcEpi { f32x4 sc[2], sh[2]; };
__device__ __forceinline__ void pc_epi_vectors(const Wino24Args& p, const PcGeo& q, const int tid, PcEpi& e) {
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int ncol = (q.tn * 2 + nt) * 32 + (tid & 7) * 4;
        e.sc[nt] = f32x4{1.f, 1.f, 1.f, 1.f};
        e.sh[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (p.scale) e.sc[nt] = *reinterpret_cast<const f32x4*>(p.scale + ncol);
        if (p.shift) e.sh[nt] = *reinterpret_cast<const f32x4*>(p.shift + ncol);
    }
}
__device__ __forceinline__ void pc_finish(const Wino24Args& p, const PcGeo& q, const float* ex, const int nt, const int tid, const bool consumer,
                                          const PcEpi& epi) {
    const int et = (tid & 255) >> 3;
    const int n4 = tid & 7;
    int g, tyt, txt, prow_unused;
    const bool tile_ok = pc_slot(p, q, et, g, tyt, txt, prow_unused) && g < q.n_here;
    const int oy = 2 * tyt, ox = 4 * txt;
    const int cstep = p.K * 4, rstep = p.Wo * cstep;
    const size_t out_img = (size_t)p.Ho * p.Wo * p.K * 4;
    const __amdgpu_buffer_rsrc_t y_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void*)((char*)p.y + (size_t)q.n_img * out_img), 0, (int)(out_img * q.n_here), 0x00020000);
    const __amdgpu_buffer_rsrc_t r_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void*)((const char*)(p.res ? p.res : p.y) + (size_t)q.n_img * out_img), 0, (int)(out_img * q.n_here), 0x00020000);
    const int ncol = (q.tn * 2 + nt) * 32 + n4 * 4;
    const f32x4 sc = epi.sc[nt], sh = epi.sh[nt];
    // (operands below 2^24: the launcher caps an image group's output at 2^31 bytes and K >= 64 -- the full-rate 24-bit multiply)
    const unsigned obase = (unsigned)(__mul24(__mul24(__mul24(g, p.Ho) + oy, p.Wo) + ox, p.K) + ncol) * 4u;
    unsigned off[2][2];
    f32x4 rv[2][2];
#pragma unroll
    for (int bc = 0; bc < 2; ++bc)
#pragma unroll
        for (int aa = 0; aa < 2; ++aa) {
            const int bcol = (consumer ? 0 : 2) + bc;
            const bool ok = tile_ok && (oy + aa) < p.Ho && (ox + bcol) < p.Wo;
            off[bc][aa] = ok ? obase + (unsigned)(aa * rstep + bcol * cstep) : kOob;
            if (p.res) rv[bc][aa] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r_rsrc, off[bc][aa], 0, 0));   // all four ahead of the LDS reads
        }
#pragma unroll
    for (int bc = 0; bc < 2; ++bc) {
        const int bcol = (consumer ? 0 : 2) + bc;
        const f32x4 q0 = *reinterpret_cast<const f32x4*>(&ex[((0 * 4 + bcol) * 32 + et) * 32 + (n4 ^ (et & 7)) * 4]);
        const f32x4 q1 = *reinterpret_cast<const f32x4*>(&ex[((1 * 4 + bcol) * 32 + et) * 32 + (n4 ^ (et & 7)) * 4]);
        const f32x4 q2 = *reinterpret_cast<const f32x4*>(&ex[((2 * 4 + bcol) * 32 + et) * 32 + (n4 ^ (et & 7)) * 4]);
        const f32x4 q3 = *reinterpret_cast<const f32x4*>(&ex[((3 * 4 + bcol) * 32 + et) * 32 + (n4 ^ (et & 7)) * 4]);
        f32x4 yv[2];
        yv[0] = q0 + q1 + q2;
        yv[1] = q1 - q2 - q3;
#pragma unroll
        for (int aa = 0; aa < 2; ++aa) {
            f32x4 v = yv[aa] * sc + sh;
            if (p.res) {
                if (p.relu == 2) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = rv[bc][aa][e] > 0.f ? v[e] : 0.f;
                } else {
                    v += rv[bc][aa];
                }
            }
            if (p.relu == 1) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
            }
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), y_rsrc, off[bc][aa], 0, 0);
        }
    }
}

template <int RING>
__global__ __launch_bounds__(512, 2) void conv3x3_wino24pc(const Wino24Args p) {
    constexpr int NT = 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char (*raw)[RAWB] = reinterpret_cast<char (*)[RAWB]>(smem + PC_RAW);
    float* const ex = reinterpret_cast<float*>(smem + PC_EX);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool consumer = wave < 4;
    const int xi = wave & 3;
    const int n = p.nchunks;

    const XcdTiles xt = xcd_tiles(p.total_tiles);
    const int ntiles = xt.ntiles, S = xt.stride;
    if (ntiles == 0) return;
    const int tile0 = xt.tile0();

    const int vlane = PC_V + (xi * 6 * 64 + lane) * 16;        // this wave pair's row of V[0]: + buf * PC_VB + nu * 1024
#ifdef SEAM_W24PC_TRACE
    const bool tr_on = p.trace && blockIdx.x == SEAM_W24PC_TRACE && (wave & 3) == 0;
    int tr_k = 0;
#endif

#ifdef SEAM_W24PC_TRACE
    const unsigned long long blk_t0 = __builtin_amdgcn_s_memtime();
#endif
    if (!consumer) {
        // =================================================== producer ===================================================
        const int ptid = tid - 256;
        const size_t img_bytes = (size_t)p.H * p.W * p.C * 4;
        constexpr int NP = 12;                  // 16-byte patch pieces per thread and GROUP of four chunks (one 128-byte line per pixel)
        // Address state of the three stages that touch a tile's geometry.  Each piece is recomputed for the next tile (vector ALU,
        // in a burst window) right after its stage has used it for the last time, so one set serves the whole pipeline.
        //   A patch pixel's 32 channels of a group are ONE 128-byte line: eight adjacent lanes fetch it with one 16-byte piece each
        //   (round 5: the per-chunk form -- two lanes per line, four visits per line -- missed the 32 KiB L1 every time: 4 x the
        //   L2 requests, and the vector-memory queue it kept busy held back the consumers' weight loads).
        unsigned goff[NP];                      // load stage: global byte offset of piece (ptid & 7) of pixel (ptid >> 3) + 32 r; kOob outside
        LDSQ char* lp[NP];                      // store stage: LDS address of that piece inside raw[0] (its chunk = piece >> 1, half = piece & 1)
        LDSQ char* ra[4];                       // read stage: LDS addresses (raw[0]) of the transform's two patch rows at x phases 0..3
        LDSQ char* rb[4];
        LDSQ char* lpn[NP];                     // the next tile's lp, computed together with its goff (same pixel arithmetic)
        // (this runs in a burst window, i.e. with the consumers idle: ~440 vector instructions = 3100 cycles in its general form --
        //  2.5 % of a C = 256 tile, measured with stamps.  Products have operands below 2^24 -- launcher-checked: 2^31 bytes per
        //  image group, C >= 64 -- and use the full-rate 24-bit multiply.  Consecutive tiles of a block mostly lie in the same
        //  region of a non-stacked map: their patch has the same shape, so each piece's patch coordinates (kept packed in `vp`)
        //  and LDS address are unchanged and only the image offset and the border tests are redone -- ~150 instructions.)
        int vp[NP];                             // piece r's patch row | column << 16 in the region `vp_reg` (row 0x7fff: no pixel)
        int vp_reg = -1;                        // -1: nothing cached
        auto setup_patch = [&](const PcGeo& q, LDSQ char* (&lp_)[NP]) {
            const int pitch = 2 * p.tiles_y + 2;
            if (q.reg == vp_reg) {
                if (p.stack) {
                    // stacked maps (round 6): the patch shape is the same for every tile, only the row at which the images wrap moves
                    // (prow0) -- the piece's patch coordinates and LDS address stay, the image index and its row are redone
#pragma unroll
                    for (int r = 0; r < NP; ++r) {
                        const int v = vp[r] & 0xffff, px = vp[r] >> 16;
                        const int vr = q.prow0 + v;                 // v = 0x7fff (no pixel): an image index far outside the group
                        const int g = fdivu(vr, pitch, p.m_pitch);
                        const int gy = vr - __mul24(g, pitch) - p.pad, gx = q.ix0 + px;
                        const bool inb = g < q.n_here && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
                        goff[r] = inb ? (unsigned)((__mul24(__mul24(__mul24(g, p.H) + gy, p.W) + gx, p.C) + (ptid & 7) * 4) * 4) : kOob;
                    }
                    return;
                }
#pragma unroll
                for (int r = 0; r < NP; ++r) {
                    const int v = vp[r] & 0xffff, px = vp[r] >> 16;
                    const int gy = q.iy0 + v, gx = q.ix0 + px;
                    const bool inb = (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;      // v = 0x7fff fails the row test
                    goff[r] = inb ? (unsigned)((__mul24(__mul24(gy, p.W) + gx, p.C) + (ptid & 7) * 4) * 4) : kOob;
                }
                return;                         // lp_ (= lpn): this region's addresses already
            }
#pragma unroll
            for (int r = 0; r < NP; ++r) {
                const int pix = (ptid >> 3) + 32 * r;
                const int v = fdivu(pix, q.PW, q.m_PW);
                const int px = pix - __mul24(v, q.PW);
                int g = 0, gy = q.iy0 + v;
                if (p.stack) {
                    const int vr = q.prow0 + v;
                    g = fdivu(vr, pitch, p.m_pitch);
                    gy = vr - __mul24(g, pitch) - p.pad;
                }
                const int gx = q.ix0 + px;
                const bool inb = pix < q.NPIX && g < q.n_here && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
                goff[r] = inb ? (unsigned)((__mul24(__mul24(__mul24(g, p.H) + gy, p.W) + gx, p.C) + (ptid & 7) * 4) * 4) : kOob;
                const int half = ptid & 1;
                lp_[r] = (LDSQ char*)smem + PC_RAW +
                         (pix < q.NPIX ? (__mul24(half, q.NENT) + __mul24(v >> 1, q.PR) + __mul24((v & 1) * 4 + (px & 3), q.HS) + (px >> 2)) * 16
                                       : 2 * ENTMAX * 16);
                vp[r] = pix < q.NPIX ? (v | (px << 16)) : 0x7fff;
            }
            vp_reg = q.reg;
        };
        auto setup_read = [&](const PcGeo& q) {
            // input transform of row xi: T_j = d[ra][j] + cb * d[rb][j]  (rows: xi0: d0 - d2, xi1: d1 + d2, xi2: d2 - d1, xi3: d1 - d3)
            const int rwa = xi == 0 ? 0 : xi == 2 ? 2 : 1;
            const int rwb = xi == 0 ? 2 : xi == 1 ? 2 : xi == 2 ? 1 : 3;
            int g, ty, tx, prow;
            if (!pc_slot(p, q, lane & 31, g, ty, tx, prow)) pc_slot(p, q, 0, g, ty, tx, prow);     // idle slots read tile 0 (never stored)
            const int rbase = (__mul24(lane >> 5, q.NENT) + __mul24(prow >> 1, q.PR) + (tx - q.tx0)) * 16;
            const int oa = ((rwa >> 1) * q.PR + (rwa & 1) * 4 * q.HS) * 16, ob = ((rwb >> 1) * q.PR + (rwb & 1) * 4 * q.HS) * 16;
#pragma unroll
            for (int j = 0; j < 4; ++j) {       // column j: x phase (j & 3) at entry (j >> 2)
                ra[j] = (LDSQ char*)smem + PC_RAW + rbase + oa + j * q.HS * 16;
                rb[j] = (LDSQ char*)smem + PC_RAW + rbase + ob + j * q.HS * 16;
            }
        };
        auto x_desc = [&](const PcGeo& q) {
            return __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)p.x + (size_t)q.n_img * img_bytes), 0, (int)(img_bytes * q.n_here), 0x00020000);
        };
        const float cb = xi == 1 ? 1.f : -1.f;
        const f32x2 cb2 = {cb, cb};
        const f32x2 k4 = {4.f, 4.f}, km5 = {-5.f, -5.f}, km4 = {-4.f, -4.f}, k2 = {2.f, 2.f}, km2 = {-2.f, -2.f};

        __amdgpu_buffer_rsrc_t rsrcL;
        int gL = 0;                             // next group (of its tile) the load stage requests
        // The request stage runs two groups (eight chunks) ahead of the store stage: with n = 8 chunks per tile (the C = 64 layers) it
        // works one whole tile ahead of the others (LEAD = 1), otherwise it moves to the next tile eight intervals before the end.
        const int LEAD = n == 8 ? 1 : 0;
        const int i_setup = n == 8 ? 6 : n - 9; // the interval in whose burst window the request stage's next address set is computed
        {
            const PcGeo q0 = pc_geo(p, tile0);
            setup_patch(q0, lp);
#pragma unroll
            for (int r = 0; r < NP; ++r) lpn[r] = lp[r];        // the fast path above leaves lpn alone
            setup_read(q0);
            rsrcL = x_desc(q0);
        }
        f32x4 rq[2][NP];                        // the pieces of two groups (group parity)
        f32x4 xa[3], xb[3], ya[3], yb[3], va[6];
        auto load_group = [&](f32x4 (&dst)[NP]) {      // request group gL of the load stage's tile
            const int so = min(gL, (n >> 2) - 1) * 128;     // (never past a tile's last group)
#pragma unroll
            for (int r = 0; r < NP; ++r)
                dst[r] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrcL, goff[r], so, 0));
            ++gL;
        };
        // chunk (cq = 0..3 of its group) -> LDS raw[buf]: the sixteen lanes per instruction that hold this chunk's pieces store them
        // (exec mask by immediate; scalar + LDS instructions only -- a v_cmp in front of the stores would not issue before the consumer yields)
#define PC_ST1(i) "ds_write_b128 %" #i ", %[d" #i "] offset:%[off]\n\t"
#define PC_STORE12(MASK, src, buf)                                                                                                          \
        asm volatile("s_mov_b32 exec_lo, " MASK "\n\ts_mov_b32 exec_hi, " MASK "\n\t"                                                        \
                     PC_ST1(0) PC_ST1(1) PC_ST1(2) PC_ST1(3) PC_ST1(4) PC_ST1(5) PC_ST1(6) PC_ST1(7) PC_ST1(8) PC_ST1(9) PC_ST1(10) PC_ST1(11)  \
                     "s_mov_b64 exec, -1"                                                                                                    \
                     :: "v"(lp[0]), "v"(lp[1]), "v"(lp[2]), "v"(lp[3]), "v"(lp[4]), "v"(lp[5]), "v"(lp[6]), "v"(lp[7]), "v"(lp[8]), "v"(lp[9]),  \
                        "v"(lp[10]), "v"(lp[11]), [d0] "v"(src[0]), [d1] "v"(src[1]), [d2] "v"(src[2]), [d3] "v"(src[3]), [d4] "v"(src[4]),    \
                        [d5] "v"(src[5]), [d6] "v"(src[6]), [d7] "v"(src[7]), [d8] "v"(src[8]), [d9] "v"(src[9]), [d10] "v"(src[10]),          \
                        [d11] "v"(src[11]), [off] "n"((buf) * RAWB) : "memory")
        auto store_chunk = [&](const f32x4 (&src)[NP], const int cq, const int buf) {
            if (cq == 0) { if (buf) PC_STORE12("0x03030303", src, 1); else PC_STORE12("0x03030303", src, 0); }
            if (cq == 1) { if (buf) PC_STORE12("0x0c0c0c0c", src, 1); else PC_STORE12("0x0c0c0c0c", src, 0); }
            if (cq == 2) { if (buf) PC_STORE12("0x30303030", src, 1); else PC_STORE12("0x30303030", src, 0); }
            if (cq == 3) { if (buf) PC_STORE12("0xc0c0c0c0", src, 1); else PC_STORE12("0xc0c0c0c0", src, 0); }
        };
        // The transform in three steps that the pipeline places apart: twelve patch reads (LDS), 36 packed ops (vector ALU: they
        // only run while the matrix pipe is idle, so they sit in front of the barrier the consumer is about to wait at), six
        // fragment stores (LDS again: behind the barrier, under the next chunk's MFMAs).
        auto tr_read = [&](int buf) {
            const int bo = buf * RAWB;
            xa[0] = *reinterpret_cast<const f32x4 LDSQ*>(ra[0] + bo);
            xb[0] = *reinterpret_cast<const f32x4 LDSQ*>(rb[0] + bo);
            xa[1] = *reinterpret_cast<const f32x4 LDSQ*>(ra[2] + bo);
            xb[1] = *reinterpret_cast<const f32x4 LDSQ*>(rb[2] + bo);
            xa[2] = *reinterpret_cast<const f32x4 LDSQ*>(ra[0] + bo + 16);
            xb[2] = *reinterpret_cast<const f32x4 LDSQ*>(rb[0] + bo + 16);
            ya[0] = *reinterpret_cast<const f32x4 LDSQ*>(ra[1] + bo);
            yb[0] = *reinterpret_cast<const f32x4 LDSQ*>(rb[1] + bo);
            ya[1] = *reinterpret_cast<const f32x4 LDSQ*>(ra[3] + bo);
            yb[1] = *reinterpret_cast<const f32x4 LDSQ*>(rb[3] + bo);
            ya[2] = *reinterpret_cast<const f32x4 LDSQ*>(ra[1] + bo + 16);
            yb[2] = *reinterpret_cast<const f32x4 LDSQ*>(rb[1] + bo + 16);
        };
        auto tr_math = [&]() {
            const f32x4 T0 = fma4s(cb2, xb[0], xa[0]), T2 = fma4s(cb2, xb[1], xa[1]), T4 = fma4s(cb2, xb[2], xa[2]);
            const f32x4 T1 = fma4s(cb2, yb[0], ya[0]), T3 = fma4s(cb2, yb[1], ya[1]), T5 = fma4s(cb2, yb[2], ya[2]);
            va[0] = fma4s(km5, T2, fma4s(k4, T0, T4));
            va[5] = fma4s(km5, T3, fma4s(k4, T1, T5));
            {
                const f32x4 a = fma4s(km4, T2, T4), bq = fma4s(km4, T1, T3);
                va[1] = add4(a, bq);
                va[2] = sub4(a, bq);
            }
            {
                const f32x4 c = sub4(T4, T2), d = sub4(T3, T1);
                va[3] = fma4s(k2, d, c);
                va[4] = fma4s(km2, d, c);
            }
        };
        LDSQ char* const vrow0 = (LDSQ char*)smem + vlane;
        auto tr_write = [&](int buf) {
#pragma unroll
            for (int nu = 0; nu < 6; ++nu) *reinterpret_cast<f32x4 LDSQ*>(vrow0 + buf * PC_VB + nu * 1024) = va[nu];
        };
#define PC_PIN_VA() asm volatile("" ::"v"(va[0]), "v"(va[1]), "v"(va[2]), "v"(va[3]), "v"(va[4]), "v"(va[5]))
        // ---- prologue of the block's first tile: V(0) in LDS, V(1) in registers, raw(2) in LDS, chunk 3 in registers, group 1 in flight
        load_group(rq[0]);
        load_group(rq[1]);
        if (LEAD) {                             // n = 8: both groups of the first tile are requested; the stage moves on to the block's second tile
            if (ntiles > 1) {
                const PcGeo q1 = pc_geo(p, tile0 + S);
                setup_patch(q1, lpn);
                rsrcL = x_desc(q1);
            } else {
#pragma unroll
                for (int r = 0; r < NP; ++r) goff[r] = kOob;
            }
            gL = 0;
        }
        store_chunk(rq[0], 0, 0);
        store_chunk(rq[0], 1, 1);
        LDS_BAR();                              // P1: raw(0), raw(1) visible (the patch is shared by the four producer waves)
        tr_read(0);
        tr_math();
        tr_write(0);
        tr_read(1);
        LDS_BAR();                              // P2: every wave has read raw[0] and raw[1]
        tr_math();                              // va = V(1)
        PC_PIN_VA();
        store_chunk(rq[0], 2, 0);               // raw(2)
        LDS_BAR();                              // P3: V(0), raw(2) visible

        // ---- interval i of a tile (i = 0 .. n - 1), closed by the barrier inside the consumers' chunk i:
        //        fragments of chunk i + 1: registers -> V[(i + 1) & 1];   patch of chunk i + 3: registers -> raw[(i + 3) & 1];
        //        every fourth interval (chunk i + 3 was its group's last): request group (i + 3) / 4 + 2 into the freed registers;
        //        patch of chunk i + 2: raw[i & 1] -> registers, then its 36 packed ops; barrier.
        //      Chunks >= n of a tile ARE the next tile's first chunks: the request stage moves to the next tile after interval
        //      n - 12 (its addresses are recomputed in the burst window of interval n - 9), the store stage after n - 4, the read
        //      stage after n - 3 -- each piece of address state right behind its last use, so nothing is selected at run time.
        //      The tile's epilogue (second halves) follows its last interval; the next tile's interval 0 starts behind it.
        auto finish_prev = [&](const int tile_prev) {   // a finished tile's epilogue, second halves (barriers E1, E2, E3)
            const PcGeo qp = pc_geo(p, tile_prev);
            PcEpi epi;
            pc_epi_vectors(p, qp, tid, epi);    // requested here, used behind the barrier
            PC_TR(30);
            LDS_BAR();                          // E1: ex holds n-tile 0
            PC_TR(31);
            if (!(SEAM_W24PC_ABL & 16)) pc_finish(p, qp, ex, 0, tid, false, epi);
            PC_TR(32);
            LDS_BAR();                          // E2: ex is free again
            PC_TR(33);
            LDS_BAR();                          // E3: ex holds n-tile 1
            PC_TR(34);
            if (!(SEAM_W24PC_ABL & 16)) pc_finish(p, qp, ex, 1, tid, false, epi);
            PC_TR(35);
        };
        int tile = tile0;
        for (int k = 0; k < ntiles; ++k) {
            const bool has_next = k + 1 < ntiles, has_lead = k + 1 + LEAD < ntiles;
            for (int i0 = 0; i0 < n; i0 += 8) {
                // interval i = i0 + j; i0 is a multiple of 8: every index below is a compile-time constant of j (a template argument,
                // not an unrolled loop variable: the register sets must be split into registers before any loop pass runs)
                auto ivl = [&](auto jt) {
                    constexpr int j = decltype(jt)::value;
                    PC_TR(1);
#ifdef SEAM_W24PC_PSLEEP
                    __builtin_amdgcn_s_sleep(SEAM_W24PC_PSLEEP);
#endif
                    tr_write((j + 1) & 1);
#if SEAM_W24PC_ABL & 256
                    {       // this wave pair's twelve fragments of a chunk two ahead: global -> LDS, no registers (never waited for: timing only)
                        const int nb = n * 24576;
                        const __amdgpu_buffer_rsrc_t ur = __builtin_amdgcn_make_buffer_rsrc(
                            (void*)((const char*)p.u + (size_t)pc_geo(p, tile).tn * NT * nb), 0, NT * nb, 0x00020000);
                        const int ck = min(i0 + j + 2, n - 1) * 24576;
#pragma unroll
                        for (int r = 0; r < 12; ++r)
                            __builtin_amdgcn_raw_ptr_buffer_load_lds(ur, (LDSQ void*)((LDSQ char*)smem + PC_EX + (xi * 12 + r) * 1024), 16,
                                                                     (xi * 6 * 64 + lane) * 16 + (r % 6 & 3) * 1024, ck + ((r % 6) >> 2) * 4096 + (r / 6) * nb, 0, 0);
                    }
#endif
#ifdef SEAM_W24PC_PSLEEP
                    __builtin_amdgcn_s_sleep(SEAM_W24PC_PSLEEP);
#endif
                    if (!(SEAM_W24PC_ABL & 1)) {
                        if (!(SEAM_W24PC_ABL & 64)) store_chunk(rq[((j + 3) >> 2) & 1], (j + 3) & 3, (j + 3) & 1);     // 64: requests only
                        if ((j & 3) == 0 && !(SEAM_W24PC_ABL & 128)) load_group(rq[((j + 3) >> 2) & 1]);           // 128: LDS stores only
                    }
                    tr_read(j & 1);
                    PC_TR(2);
                    if (!(SEAM_W24PC_ABL & 8)) tr_math();
                    PC_PIN_VA();
                    // address state for the next tile, recomputed in this burst window right behind its last use
                    if ((j == 7 || j == 6) && i0 + j == i_setup) {      // the request stage (n >= 16: its last request for this tile was at i = n - 12)
                        if (has_lead) {
                            const PcGeo qn = pc_geo(p, tile + (1 + LEAD) * S);
                            setup_patch(qn, lpn);
                            rsrcL = x_desc(qn);
                        } else {                            // no next tile: the requests fall outside every image
#pragma unroll
                            for (int r = 0; r < NP; ++r) goff[r] = kOob;
                        }
                        gL = 0;
                    }
                    if (j == 4 && i0 == n - 8 && has_next) {                                    // i = n - 4: the store stage
#pragma unroll
                        for (int r = 0; r < NP; ++r) lp[r] = lpn[r];
                    }
                    if (j == 5 && i0 == n - 8 && has_next) setup_read(pc_geo(p, tile + S));     // i = n - 3
                    PC_TR(6);
                    // the fragments are inputs of the barrier statement: hipcc otherwise sinks the packed ops below it
                    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::"v"(va[0]), "v"(va[1]), "v"(va[2]), "v"(va[3]), "v"(va[4]), "v"(va[5]) : "memory");
                    SB();
                };
                ivl(std::integral_constant<int, 0>{});
                ivl(std::integral_constant<int, 1>{});
                ivl(std::integral_constant<int, 2>{});
                ivl(std::integral_constant<int, 3>{});
                ivl(std::integral_constant<int, 4>{});
                ivl(std::integral_constant<int, 5>{});
                ivl(std::integral_constant<int, 6>{});
                ivl(std::integral_constant<int, 7>{});
            }
            finish_prev(tile);                  // this tile's epilogue (the consumers are past their last chunk's barrier)
            tile += S;
        }
#undef PC_PIN_VA
#undef PC_STORE12
#undef PC_ST1
    } else {
        // =================================================== consumer ===================================================
        f32x16 acc[6][NT];
        const int ntile_bytes = n * 24576;
        int uoff0 = (xi * 6 * 64 + lane) * 16;
        f32x4 bq[RING][NT];                     // B fragments: slot j % RING holds position instance j = 6 * chunk + nu
        constexpr int AD = SEAM_W24PC_AD;       // A fragments are requested AD positions ahead of their MFMAs
        f32x4 aq[AD + 1];                       // A fragments: position nu in aq[nu % (AD + 1)]
        static_assert(6 % (AD + 1) == 0 && AD >= 1 && AD <= 2, "the fragment ring's phase repeats every chunk");
        auto read_a = [&](int buf, int nu) -> f32x4 { return *reinterpret_cast<const f32x4*>(smem + vlane + buf * PC_VB + nu * 1024); };
        LDS_BAR();                              // P1
        LDS_BAR();                              // P2
        LDS_BAR();                              // P3
        int tile = tile0;
        auto u_desc = [&](const int tn) {
            return __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)p.u + (size_t)tn * NT * ntile_bytes), 0, NT * ntile_bytes, 0x00020000);
        };
        __amdgpu_buffer_rsrc_t u_rsrc = u_desc(pc_geo(p, tile0).tn);
        for (int k = 0; k < ntiles; ++k) {
            const PcGeo q = pc_geo(p, tile);
            auto load_b = [&](int slot_, int nu, int chunk) {
                const int so = min(chunk, n - 1) * 24576 + (nu >> 2) * 4096;     // (chunks past the end: the last one again)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
#if SEAM_W24PC_ABL & 256
                    (void)so;
                    bq[slot_][nt] = *reinterpret_cast<const f32x4*>(smem + PC_EX + ((xi * 6 + nu) * 2 + nt) * 1024 + lane * 16);
#else
                    bq[slot_][nt] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(u_rsrc, uoff0 + (nu & 3) * 1024, so + nt * ntile_bytes, 0));
#endif
                    SB();
                }
            };
            auto ring_preload = [&]() {         // the tile's first RING position instances, in ring order, pinned: the K loop's vmcnt
#pragma unroll                                  // waits count on that order
                for (int j = 0; j < RING; ++j) {
                    SB();
                    load_b(j, j % 6, j / 6);
                }
                SB();
            };
            if (k == 0) ring_preload();         // later tiles: requested in the previous tile's epilogue
#pragma unroll
            for (int a = 0; a < AD; ++a) aq[a] = read_a(0, a);
            // one chunk: positions 0..5 in order; c = chunk parity (V buffer), t = chunk index; FIRST: the tile's first chunk
            // multiplies its first k-step into a zero constant instead of clearing 192 accumulators
            auto chunk = [&](const int t, const int c, const bool first) {
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    const int jl = 6 * c + i, sl = jl % RING;
                    SB();
#ifdef SEAM_W24PC_TRACE_POS
                    PC_TR(10 + i);
#endif
                    // the fragment AD positions ahead (the next chunk's first ones come from the other V buffer, behind the barrier)
                    aq[(i + AD) % (AD + 1)] = i + AD < 6 ? read_a(c, i + AD) : read_a(c ^ 1, i + AD - 6);
                    SB();
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) {
                            if (first && kk == 0) {
                                const f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                                acc[i][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(bq[sl][nt][kk], aq[i % (AD + 1)][kk], z, 0, 0, 0);
                            } else {
                                acc[i][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(bq[sl][nt][kk], aq[i % (AD + 1)][kk], acc[i][nt], 0, 0, 0);
                            }
                            SB();
                        }
                    if (!(SEAM_W24PC_ABL & 2)) {
                        const int j2 = jl + RING;                   // the instance that takes over this slot (chunks past the end
                        load_b(sl, j2 % 6, t - c + j2 / 6);         // re-read the last chunk, never used)
                    }
                    SB();
                    if (i == 5 - AD) {          // every fragment of this chunk is in registers (or on its way, waited for by the barrier
                        PC_TR(8);               // statement): the producers may overwrite V[c]
                        LDS_BAR();
                        PC_TR(9);
                    }
                }
            };
            static_assert(12 % RING == 0, "the ring's phase repeats every two chunks");
            chunk(0, 0, true);
            chunk(1, 1, false);
            for (int t = 2; t < n; t += 2) {
                asm volatile("" : "+v"(uoff0));
                chunk(t, 0, false);
                chunk(t + 1, 1, false);         // nchunks is even (wino24_pc): one straight two-chunk body, exact vmcnt waits
            }
            // ---- epilogue: the nu half of the output transform (A4t: 6 -> 4) on register pairs into the exchange array ----
            //   columns (A4t over nu): Y0 = m0+m1+m2+m3+m4, Y1 = (m1-m2) + 2(m3-m4), Y2 = (m1+m2) + 4(m3+m4), Y3 = (m1-m2) + 8(m3-m4) + m5
            //   rows (A2t over xi, across the waves, in pc_finish): y0 = q0+q1+q2, y1 = q1-q2-q3
            PcEpi epi;
            pc_epi_vectors(p, q, tid, epi);     // requested here, used behind the first epilogue barrier
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                PC_TR(20 + 4 * nt);
                if (nt == 1) LDS_BAR();         // E2: the finishers of n-tile 0 are done with ex
                PC_TR(21 + 4 * nt);
                if (!(SEAM_W24PC_ABL & 16)) {
                    const f32x2 c2 = {2.f, 2.f}, c4 = {4.f, 4.f}, c8 = {8.f, 8.f};
                    // The MFMAs ran with the operand roles swapped (rows = channels, columns = tiles; the products and their order are
                    // the same, so are the results): a lane holds ONE tile (lane & 31) and, in registers 4m..4m+3, the four consecutive
                    // channels 8m + 4 (lane >> 5) + 0..3 -- the exchange rows [tile][32 channels] take 16-byte stores (16 per n-tile
                    // instead of 64 4-byte ones).  16-byte channel group g of a row sits at slot g ^ (tile & 7): conflict-free for the
                    // stores (eight consecutive tiles per LDS phase) and for pc_finish's reads (eight groups of one row).
                    const int tl = lane & 31;
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        f32x2 yy[4][2];
#pragma unroll
                        for (int hh = 0; hh < 2; ++hh) {
                            const int h = 2 * m + hh;
                            auto rd = [&](int nu) -> f32x2 { return f32x2{acc[nu][nt][2 * h], acc[nu][nt][2 * h + 1]}; };
                            const f32x2 m0 = rd(0), m1 = rd(1), m2 = rd(2), m3 = rd(3), m4 = rd(4), m5 = rd(5);
                            const f32x2 s12 = pk_add(m1, m2), d12 = pk_sub(m1, m2), s34 = pk_add(m3, m4), d34 = pk_sub(m3, m4);
                            yy[0][hh] = pk_add(pk_add(m0, s12), s34);
                            yy[1][hh] = pk_fma_s(c2, d34, d12);
                            yy[2][hh] = pk_fma_s(c4, s34, s12);
                            yy[3][hh] = pk_add(pk_fma_s(c8, d34, d12), m5);
                        }
                        const int grp = (2 * m + (lane >> 5)) ^ (tl & 7);
#pragma unroll
                        for (int b = 0; b < 4; ++b)
                            *reinterpret_cast<f32x4*>(&ex[((xi * 4 + b) * 32 + tl) * 32 + grp * 4]) =
                                __builtin_shufflevector(yy[b][0], yy[b][1], 0, 1, 2, 3);
                    }
                } else if (nt == 1) {
                    float sum = 0.f;
#pragma unroll
                    for (int nu = 0; nu < 6; ++nu)
#pragma unroll
                        for (int m = 0; m < NT; ++m)
#pragma unroll
                            for (int r = 0; r < 16; ++r) sum += acc[nu][m][r];
                    if (sum == 123456.789f) p.y[tid] = sum;
                }
                if (nt == NT - 1 && k + 1 < ntiles) {   // the accumulators are dead: the next tile's first weight fragments travel under
                    u_rsrc = u_desc(pc_geo(p, tile + S).tn);    // the rest of the epilogue
                    ring_preload();
                }
                PC_TR(22 + 4 * nt);
                LDS_BAR();                      // E1 / E3: ex holds this n-tile
                PC_TR(23 + 4 * nt);
                if (!(SEAM_W24PC_ABL & 16)) pc_finish(p, q, ex, nt, tid, true, epi);
            }
            tile += S;
        }
#ifdef SEAM_W24PC_TRACE
        if (p.trace && tid == 0) {      // per-block span (cycles) and tile count, behind the two traced waves' stamp areas
            p.trace[8 * 4096 + 2 * blockIdx.x] = __builtin_amdgcn_s_memtime() - blk_t0;
            p.trace[8 * 4096 + 2 * blockIdx.x + 1] = (unsigned long long)ntiles;
        }
#endif
    }
}

// OIHW fp32 [K, Cin, 3, 3] -> U = G2 g G4t in MFMA fragment order: [K/32][Cstore/8][24][64][4]
//   element (tn, chunk, p = 6*xi + nu, lane, e) = U_p[n = 32*tn + (lane & 31)][c = 8*chunk + 4*(lane >> 5) + e]
// mode 0: forward weights; mode 2: input-gradient weights (taps rotated 180 degrees, channels swapped), as in
// seam_pack_conv_weight_f32.  fp64 arithmetic, one rounding.
__global__ void wino24_pack_kernel(const float* __restrict__ w, float* __restrict__ out, int K, int Cin, int Cstore, int mode) {
    const int nch = Cstore / 8;
    const size_t total = (size_t)(K / 32) * nch * 64;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
        seam_pack::wino24_item(w, out, i, K, Cin, nch, mode);
}

}  // namespace

extern "C" {

long long seam_wino24_weight_floats(int K, int Cstore) { return (long long)K * Cstore * 24; }

int seam_pack_conv_weight_wino24_f32(const float* w, float* u_packed, int K, int Cin, int Cstore, int mode, void* stream) {
    if (!wino_ok(Cstore, K, 3, 3, 1) || Cin > Cstore) return (int)hipErrorInvalidValue;
    const size_t total = (size_t)(K / 32) * (Cstore / 8) * 64;
    const unsigned grid = seam_launch::grid256(total);
    hipLaunchKernelGGL(wino24_pack_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, w, u_packed, K, Cin, Cstore, mode);
    return (int)hipGetLastError();
}

/* MFMA issues of the launch in units of 32x32x8-channel position GEMMs (blocks x 32 tile slots x 24 positions; 0 = unsupported):
 * the figure ops.conv2d compares with seam_wino_issue_slots to pick the cheaper Winograd form for a layer shape. */
long long seam_wino24_issue_slots(int N, int H, int W, int C, int K, int pad) {
    Wino24Args a;
    long blocks;
    if (wino24_plan(a, N, H, W, C, K, pad, blocks)) return 0;
    const long work = patch_blocks(a) * a.tiles_n;     // without the padding blocks of an n-tile split
    return (long long)work * a.nt * 32 * 24;
}

/* 1 when the launcher runs this layer shape on the producer / consumer kernel conv3x3_wino24pc (NT = 2 work split over two wave
 * groups), 0 for conv3x3_wino24<NT>; -1 = unsupported shape */
int seam_wino24_form(int N, int H, int W, int C, int K, int pad) {
    Wino24Args a;
    long blocks;
    if (wino24_plan(a, N, H, W, C, K, pad, blocks)) return -1;
    return wino24_pc(a) ? 1 : 0;
}

/* n-tiles per block (the kernel's template argument NT = 1 | 2) the launcher picks for this layer shape; 0 = unsupported */
int seam_wino24_variant(int N, int H, int W, int C, int K, int pad) {
    Wino24Args a;
    long blocks;
    if (wino24_plan(a, N, H, W, C, K, pad, blocks)) return 0;
    return a.nt;
}

int seam_conv3x3_wino24_f32(const float* x, const float* u_packed, const float* scale, const float* shift, const float* residual,
                            float* y, int N, int H, int W, int C, int K, int pad, int relu, void* stream) {
    Wino24Args a;
    long blocks;
    const int rc = wino24_plan(a, N, H, W, C, K, pad, blocks);
    if (rc) return rc;
    a.x = x; a.u = u_packed; a.scale = scale; a.shift = shift; a.res = residual; a.y = y;
    a.relu = relu;
    a.trace = nullptr;
    a.total_tiles = 0;
    if (wino24_pc(a)) {
        int ncu;
        const hipError_t e = seam_launch::prepare<conv3x3_wino24pc<SEAM_W24PC_RING>>(PC_LDS, &ncu);
        if (e != hipSuccess) return (int)e;
        // persistent grid: one block per CU walks its XCD's tile range (SEAM_W24_PERSIST=0: one tile per block)
        const int persist = seam_opt::get(seam_opt::W24_PERSIST);
        a.total_tiles = (int)blocks;
        for (int r = 0; r < 3; ++r) {
            a.rg[r].TX = a.TX[r]; a.rg[r].TY = a.TY[r]; a.rg[r].bx = a.bx[r]; a.rg[r].by = a.by[r];
            a.rg[r].rx0 = a.rx0[r]; a.rg[r].ry0 = a.ry0[r]; a.rg[r].rxe = a.rxe[r]; a.rg[r].rye = a.rye[r];
            a.rg[r].m_bx = a.m_bx[r]; a.rg[r].m_TX = a.m_TX[r]; a.rg[r].m_PW = a.m_PW[r];
            for (int e = 0; e < 5; ++e) a.rg[r].pad_[e] = 0;
        }
        const unsigned grid = (unsigned)(persist && blocks > ncu ? ncu : blocks);
#ifdef SEAM_W24PC_TRACE
        static seam_dev::TraceBuf tb;
        a.trace = seam_dev::trace_begin(tb, 8 * 4096 + 2 * 1024);
#endif
        hipLaunchKernelGGL(conv3x3_wino24pc<SEAM_W24PC_RING>, dim3(grid), dim3(512), PC_LDS, (hipStream_t)stream, a);
#ifdef SEAM_W24PC_TRACE
        seam_dev::trace_end(tb, 3, 4096, true, grid < 1024 ? grid : 1024);
#endif
        return (int)hipGetLastError();
    }
    if (a.nt == 2) hipLaunchKernelGGL(conv3x3_wino24<2>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(conv3x3_wino24<1>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // extern "C"
