// seam_wino_layout.h -- which blocks a Winograd launch consists of: the block-layout chooser of the F(2x2,3x3) kernels
// (seam_wino.hip) and the F(2x4,3x3) kernels (seam_wino24_common.h), and the part of their launch planners that does not depend on
// the kernel.  Host code in plain C++ (no HIP include): a host compiler builds it alone, tests/wino_layout_check.cpp does.
//
// Small maps: the whole tile grid of G images per block (stacked form).  Otherwise up to three regions per image: a main region
// tiled exactly by TX x TY patches, and the right / bottom strips that remain, each tiled by the best patch for ITS shape -- a
// 100 x 100 tile map of F(2x2) takes 157 blocks of 64 instead of 169.
#pragma once
#include <stddef.h>

namespace seam_wino_layout {

struct Layout {
    int nreg, G, stack, PH;
    int rx0[3], ry0[3], rxe[3], rye[3], TX[3], TY[3], bx[3], by[3];
    long per_img, blocks;      // blocks: per n-tile, for N images
};

// The kernel form a layout is chosen for: output columns per tile (a tile is 2 rows high; the raw patch of TX x TY tiles is
// tile_w * TX + 2 pixels wide, 2 * TY + 2 high), tile slots per block, raw-patch pixels per LDS buffer, 16-byte LDS entries per
// channel half (0: the form has no such rule).  The kernels size their buffers from these very numbers.
struct Form { int tile_w, slots, npixmax, entmax; };
constexpr Form F22_MT1{2, 32, 208, 0};     // conv3x3_wino<1>
constexpr Form F22_MT2{2, 64, 384, 0};     // conv3x3_wino<2>
constexpr Form F24{4, 32, 384, 672};       // conv3x3_wino24<NT>, conv3x3_wino24pc, conv3x3_wino24sx

// F(2x4): LDS entries per channel half for a patch of tx tiles x ph rows (the kernel's HS / PR / NENT)
inline int lds_entries(int tx, int ph) {
    const int hs = (tx + 1) | 1, pr = 8 * hs + (tx & 7), n0 = pr * ((ph + 1) / 2);
    return n0 + ((4 - n0) & 7);
}

// a raw patch of tx tiles x ph pixel rows fits the block's buffers
inline bool fits(const Form& f, int tx, int ph) {
    return (f.tile_w * tx + 2) * ph <= f.npixmax && (!f.entmax || lds_entries(tx, ph) <= f.entmax);
}

inline bool patch_ok(const Form& f, int tx, int ty) { return tx >= 1 && ty >= 1 && tx * ty <= f.slots && fits(f, tx, 2 * ty + 2); }

// best uniform tiling of a w x h tile rectangle: fewest blocks, then the smallest raw patch
inline long best_uniform(const Form& f, int w, int h, int& TX, int& TY) {
    long best = -1, best_cost = -1;
    for (int ty = 1; ty <= f.slots && ty <= h; ++ty)
        for (int tx = 1; tx * ty <= f.slots && tx <= w; ++tx) {
            if (!patch_ok(f, tx, ty)) continue;
            const long nb = (long)((w + tx - 1) / tx) * ((h + ty - 1) / ty);
            const long cost = nb * 4096 + (f.tile_w * tx + 2) * (2 * ty + 2);
            if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = nb; TX = tx; TY = ty; }
        }
    return best;
}

// appends the tile rectangle [x0, xe) x [y0, ye) to C as a region of its own best uniform tiling; adds its blocks to nb
inline void add_region(const Form& f, Layout& C, int x0, int y0, int xe, int ye, long& nb) {
    const int r = C.nreg++;
    nb += best_uniform(f, xe - x0, ye - y0, C.TX[r], C.TY[r]);
    C.rx0[r] = x0; C.ry0[r] = y0; C.rxe[r] = xe; C.rye[r] = ye;
    C.bx[r] = (xe - x0 + C.TX[r] - 1) / C.TX[r]; C.by[r] = (ye - y0 + C.TY[r] - 1) / C.TY[r];
}

// oob: the stacked form addresses the G images of a block through ONE buffer descriptor, so G images must stay below the byte
// offset the kernels use as "out of range" (seam_device.h kOob)
inline Layout choose_layout(const Form& f, int N, int tiles_x, int tiles_y, size_t in_img_bytes, size_t out_img_bytes, size_t oob) {
    // Stacked candidate (maps narrower than a block): TY consecutive tile rows of the batch at full width per block.  The tile
    // rows of ALL images form one tall list; a block's raw patch lives in "padded row" space, image n owning rows
    // [n * pitch, (n + 1) * pitch), pitch = 2 * tiles_y + 2.
    Layout S{};
    S.blocks = -1;
    if (tiles_x <= f.slots) {
        const int t = tiles_y, pitch = 2 * t + 2;
        for (int ty = f.slots / tiles_x; ty >= 1; --ty) {
            int phmax = 0, gmax = 0;
            for (int b = 0; b < t; ++b) {                                // block starts repeat with period <= tiles_y
                const int tyf = (int)(((long)b * ty) % t);
                const int last = tyf + ty - 1;
                const int gl = last / t, tyl = last - gl * t;
                const int span = pitch * gl + 2 * tyl + 4 - 2 * tyf;
                if (span > phmax) phmax = span;
                if (gl + 1 > gmax) gmax = gl + 1;
            }
            if (!fits(f, tiles_x, phmax)) continue;
            if ((size_t)gmax * in_img_bytes >= oob || (size_t)gmax * out_img_bytes >= oob) continue;
            S.nreg = 1; S.stack = 1; S.PH = phmax; S.G = gmax;
            S.rxe[0] = tiles_x; S.rye[0] = tiles_y; S.TX[0] = tiles_x; S.TY[0] = ty; S.bx[0] = S.by[0] = 1;
            S.per_img = 1;
            S.blocks = ((long)N * t + ty - 1) / ty;
            break;
        }
    }
    // one region (uniform tiling) is the baseline
    Layout L{};
    L.G = 1;
    long best_blocks = 0;
    add_region(f, L, 0, 0, tiles_x, tiles_y, best_blocks);
    // main region + strips
    for (int ty = 1; ty <= f.slots && ty <= tiles_y; ++ty)
        for (int tx = 1; tx * ty <= f.slots && tx <= tiles_x; ++tx) {
            if (!patch_ok(f, tx, ty)) continue;
            const int mx = tiles_x / tx, my = tiles_y / ty;              // exact blocks of the main region
            const int wm = mx * tx, hm = my * ty;
            if (wm == 0 || hm == 0) continue;
            Layout C;                                                    // (regions past nreg stay unset: ~100 candidates per call)
            C.G = 1; C.nreg = 1; C.stack = 0; C.PH = 0;
            C.rx0[0] = 0; C.ry0[0] = 0; C.rxe[0] = wm; C.rye[0] = hm; C.TX[0] = tx; C.TY[0] = ty; C.bx[0] = mx; C.by[0] = my;
            long nb = (long)mx * my;
            if (wm < tiles_x) add_region(f, C, wm, 0, tiles_x, tiles_y, nb);     // right strip: full height
            if (hm < tiles_y) add_region(f, C, 0, hm, wm, tiles_y, nb);          // bottom strip: under the main region only
            if (nb < best_blocks) {
                best_blocks = nb;
                L = C;
            }
        }
    L.per_img = 0;
    for (int r = 0; r < L.nreg; ++r) L.per_img += (long)L.bx[r] * L.by[r];
    L.blocks = L.per_img * N;
    if (S.blocks > 0 && S.blocks < L.blocks) return S;
    return L;
}

inline bool wino_ok(int C, int K, int R, int S, int stride) { return R == 3 && S == 3 && stride == 1 && C % 8 == 0 && K % 32 == 0 && C >= 8; }

// ---- the planners' shared tail (WinoArgs and Wino24Args name these fields alike) --------------------------------------------

// the layout into the launch arguments; regions past nreg repeat region 0, so the kernel may read all three
template <class Args>
inline void set_layout(Args& a, const Layout& L, int tiles_y) {
    a.nreg = L.nreg; a.G = L.G; a.per_img = (int)L.per_img;
    a.stack = L.stack; a.PH = L.PH; a.tiles_y = tiles_y;
    for (int r = 0; r < 3; ++r) {
        const int q = r < L.nreg ? r : 0;
        a.rx0[r] = L.rx0[q]; a.ry0[r] = L.ry0[q]; a.rxe[r] = L.rxe[q]; a.rye[r] = L.rye[q];
        a.TX[r] = L.TX[q]; a.TY[r] = L.TY[q]; a.bx[r] = L.bx[q]; a.by[r] = L.by[q];
    }
}

// n-tile split (see the kernels' tile decode): `want` XCD groups, reduced until the number divides the a.tiles_n n-tiles and the 8
// XCDs; the patch blocks are cut into 8 / nsplit partitions of part_q (+1 for the first part_r) each.  Returns the grid: patch
// blocks x n-tiles, with a split padded to the longest partition.
// (wino_plan runs a floor loop of its own before this one and relies on `8 % ns` being tested here: see there.)
template <class Args>
inline long split_ntiles(Args& a, long patch_blocks, int want) {
    int ns = want;
    while (ns > 1 && (a.tiles_n % ns || 8 % ns)) ns >>= 1;
    a.nsplit = ns < 1 ? 1 : ns;
    a.tns = a.tiles_n / a.nsplit;
    const int parts = 8 / a.nsplit;
    a.part_q = (int)(patch_blocks / parts); a.part_r = (int)(patch_blocks % parts);
    return a.nsplit > 1 ? 8L * (a.part_q + (a.part_r ? 1 : 0)) * a.tns : patch_blocks * a.tiles_n;
}

// the patch blocks of a planned launch (all images, per n-tile): what the grid holds without the padding blocks of a split
template <class Args>
inline long patch_blocks(const Args& a) { return (long)(8 / a.nsplit) * a.part_q + a.part_r; }

}  // namespace seam_wino_layout
