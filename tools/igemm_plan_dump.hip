// Prints what the launchers of the implicit-GEMM conv family (csrc/seam_conv.hip) decide over a sweep of geometries: per call the
// return code and, when accepted, the kernel named in the launch (the expression as written), grid, block and every field of ConvArgs
// by name.  The launch itself is replaced by a recorder (hipLaunchKernelGGL and hipGetLastError are redefined below, after the HIP
// header is in), so only host code runs and no GPU is needed.  Two builds of the kernel file are compared by diffing the two outputs
// (profiles/igemm_split_fold.txt); <csrc> is the directory of the build under test:
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude -I<csrc> tools/igemm_plan_dump.hip
//         -o igemm_plan_dump && ./igemm_plan_dump > plans.txt
#include <hip/hip_runtime.h>
#include <cstdio>

namespace rec {
template <class... A>
void launch(const char* kern, dim3 grid, dim3 block, const A&... args);
}
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kern, grid, block, shmem, stream, ...) rec::launch(#kern, grid, block, __VA_ARGS__)
#define hipGetLastError() hipSuccess

#include "seam_abi.hip"
#include "seam_conv.hip"

namespace {

long accepted = 0, refused = 0, launches = 0;
char dummy[8 * 64];      // never dereferenced: a pointer field prints as its offset in here, or -1 for null
const float* fp(int i) { return i < 0 ? nullptr : (const float*)(dummy + 64 * i); }
long off(const void* q) { return q ? (long)((const char*)q - dummy) : -1; }

void show(const ConvArgs& a) {
    printf(" x=%ld w=%ld scale=%ld shift=%ld res=%ld y=%ld N=%d H=%d W=%d C=%d Ho=%d Wo=%d K=%d R=%d S=%d stride=%d pad=%d kred=%d M=%d relu=%d"
           " y_f32=%d vec_epi=%d slab_bn=%d tiles_m=%d tiles_n=%d x2=%ld H2=%d W2=%d C2=%d stride2=%d m_HoWo=%u m_Wo=%u div_fast=%d"
           " epi_prio=%d rH=%d rW=%d", off(a.x), off(a.w), off(a.scale), off(a.shift), off(a.res), off(a.y), a.N, a.H, a.W, a.C, a.Ho,
           a.Wo, a.K, a.R, a.S, a.stride, a.pad, a.kred, a.M, a.relu, a.y_f32, a.vec_epi, a.slab_bn, a.tiles_m, a.tiles_n, off(a.x2),
           a.H2, a.W2, a.C2, a.stride2, a.m_HoWo, a.m_Wo, a.div_fast, a.epi_prio, a.rH, a.rW);
}
template <class... A>
void show(const A&...) {}      // the pack kernels' arguments: not part of the sweep

void done(int rc) {
    ++(rc ? refused : accepted);
    printf(" rc=%d\n", rc);
}

void* const ST = nullptr;

// one geometry through every entry; dual only where the entry's own shape (1x1, pad 0) is the geometry
void geometry(int N, int H, int W, int C, int C_other, int K, int R, int stride, int pad, int relu) {
    const float *x = fp(0), *w = fp(1), *sc = fp(2), *sh = fp(3), *res = fp(4), *x2 = fp(6);
    float* y = (float*)fp(5);
    const bool fits = H + 2 * pad >= R && W + 2 * pad >= R;
    const int Ho = fits ? (H + 2 * pad - R) / stride + 1 : 1, Wo = fits ? (W + 2 * pad - R) / stride + 1 : 1;
#define CALL(name, ...)                                                                              \
    do {                                                                                             \
        printf(#name " %d %d %d %d %d %d %d %d %d:", N, H, W, C, K, R, stride, pad, relu);           \
        done(name(__VA_ARGS__));                                                                     \
    } while (0)
    CALL(seam_conv2d_f32, x, w, sc, sh, res, y, N, H, W, C, K, R, R, stride, pad, relu, ST);
    CALL(seam_conv2d_f16, x, w, sc, sh, res, y, N, H, W, C, K, R, R, stride, pad, relu, relu == 1, ST);
    CALL(seam_conv2d_upres_f32, x, w, sc, sh, res, y, N, H, W, C, K, R, R, stride, pad, (Ho + 1) / 2, (Wo + 1) / 2, relu, ST);
    CALL(seam_conv2d_crop_f32, x, w, sc, sh, y, N, H, W, C, K, R, R, stride, pad, Ho > 1 ? Ho - 1 : 1, Wo, relu, ST);
    CALL(seam_conv2d_crop_f16, x, w, sc, sh, y, N, H, W, C, K, R, R, stride, pad, Ho, Wo > 1 ? Wo - 1 : 1, relu, ST);
    if (R == 1 && pad == 0) {      // x is the output grid, x2 the strided second source
        CALL(seam_conv2d_dual_f32, x, x2, w, sc, sh, y, N, H, W, C, (H - 1) * stride + 1, (W - 1) * stride + 1, C_other, stride, K, relu, ST);
        CALL(seam_conv2d_dual_f16, x, x2, w, sc, sh, y, N, H, W, C, (H - 1) * stride + 1, (W - 1) * stride + 1, C_other, stride, K, relu, ST);
    }
    CALL(seam_conv2d_bx3, x, w, sc, sh, res, y, N, H, W, C, K, R, R, stride, pad, relu, ST);
    for (int terms : {3, 5, 6, 9}) CALL(seam_conv2d_sx, x, w, sc, sh, res, y, N, H, W, C, K, R, R, stride, pad, relu, terms, ST);
}

// the refusals of tests/test_gpu_stress_igemm.py (and what each shares its line with)
void refusals() {
    const float* p = fp(0);
    float* q = (float*)fp(5);
    int N = 0, H = 0, W = 0, C = 0, K = 0, R = 0, stride = 0, pad = 0, relu = 0;      // CALL's line header: the case's ordinal instead
#define REFUSED(name, ...) do { ++N; CALL(name, __VA_ARGS__); } while (0)
    for (int cc : {6, 36}) {
        REFUSED(seam_conv2d_f32, p, p, nullptr, nullptr, nullptr, q, 1, 8, 8, cc, 64, 3, 3, 1, 1, 0, ST);
        REFUSED(seam_conv2d_bx3, p, p, nullptr, nullptr, nullptr, q, 1, 8, 8, cc, 64, 3, 3, 1, 1, 0, ST);
        REFUSED(seam_conv2d_sx, p, p, nullptr, nullptr, nullptr, q, 1, 8, 8, cc, 64, 3, 3, 1, 1, 0, 6, ST);
        REFUSED(seam_pack_conv_weight_f32, p, q, 64, cc, 3, 3, cc, 0, ST);
    }
    for (int cc : {4, 72}) {
        REFUSED(seam_conv2d_f16, p, p, nullptr, nullptr, nullptr, q, 1, 8, 8, cc, 64, 3, 3, 1, 1, 0, 0, ST);
        REFUSED(seam_pack_conv_weight_f16, p, q, 64, cc, 3, 3, cc, 0, ST);
    }
    REFUSED(seam_conv2d_f32, p, p, nullptr, nullptr, nullptr, q, 1, 8, 8, 32, 0, 3, 3, 1, 1, 0, ST);
    REFUSED(seam_conv2d_f16, p, p, nullptr, nullptr, nullptr, q, 1, 8, 8, 64, 0, 3, 3, 1, 1, 0, 0, ST);
    REFUSED(seam_conv2d_bx3, p, p, nullptr, nullptr, nullptr, q, 1, 8, 8, 32, 0, 3, 3, 1, 1, 0, ST);
    REFUSED(seam_conv2d_sx, p, p, nullptr, nullptr, nullptr, q, 1, 8, 8, 32, 0, 3, 3, 1, 1, 0, 9, ST);
    REFUSED(seam_conv2d_f32, p, p, nullptr, nullptr, nullptr, q, 1, 2, 8, 32, 64, 5, 5, 1, 1, 0, ST);
    REFUSED(seam_conv2d_f32, p, p, nullptr, nullptr, nullptr, q, 1, 2, 8, 32, 64, 5, 5, 2, 1, 0, ST);
    REFUSED(seam_conv2d_f32, p, p, nullptr, nullptr, nullptr, q, 1, 8, 1, 32, 64, 5, 5, 3, 1, 0, ST);
    REFUSED(seam_conv2d_f16, p, p, nullptr, nullptr, nullptr, q, 1, 2, 8, 64, 64, 5, 5, 2, 1, 0, 0, ST);
    REFUSED(seam_conv2d_bx3, p, p, nullptr, nullptr, nullptr, q, 1, 2, 8, 32, 64, 5, 5, 2, 1, 0, ST);
    REFUSED(seam_conv2d_sx, p, p, nullptr, nullptr, nullptr, q, 1, 8, 1, 32, 64, 5, 5, 3, 1, 0, 9, ST);
    REFUSED(seam_conv2d_crop_f32, p, p, nullptr, nullptr, q, 1, 2, 8, 32, 64, 5, 5, 2, 1, 1, 1, 0, ST);
    REFUSED(seam_conv2d_f32, p, p, nullptr, nullptr, nullptr, q, 1, 8, 2, 32, 64, 5, 5, 1, 1, 0, ST);
    REFUSED(seam_conv2d_f16, p, p, nullptr, nullptr, nullptr, q, 1, 2, 8, 64, 64, 5, 5, 1, 1, 0, 0, ST);
    REFUSED(seam_conv2d_bx3, p, p, nullptr, nullptr, nullptr, q, 1, 2, 8, 32, 64, 5, 5, 1, 1, 0, ST);
    REFUSED(seam_conv2d_sx, p, p, nullptr, nullptr, nullptr, q, 1, 2, 8, 32, 64, 5, 5, 1, 1, 0, 6, ST);
    REFUSED(seam_conv2d_crop_f32, p, p, nullptr, nullptr, q, 1, 8, 8, 32, 64, 3, 3, 1, 1, 9, 8, 0, ST);
    REFUSED(seam_conv2d_crop_f32, p, p, nullptr, nullptr, q, 1, 8, 8, 32, 64, 3, 3, 2, 1, 4, 5, 0, ST);
    REFUSED(seam_conv2d_crop_f16, p, p, nullptr, nullptr, q, 1, 8, 8, 64, 64, 3, 3, 1, 1, 8, 9, 0, ST);
    REFUSED(seam_conv2d_upres_f32, p, p, nullptr, nullptr, p, q, 1, 8, 8, 32, 6, 1, 1, 1, 0, 4, 4, 0, ST);
    REFUSED(seam_conv2d_upres_f32, p, p, nullptr, nullptr, p, q, 1, 8, 8, 32, 64, 1, 1, 1, 0, 4, 4, 2, ST);
    REFUSED(seam_conv2d_upres_f32, p, p, nullptr, nullptr, nullptr, q, 1, 8, 8, 32, 64, 1, 1, 1, 0, 4, 4, 0, ST);
    REFUSED(seam_conv2d_upres_f32, p, p, nullptr, nullptr, p, q, 1, 8, 8, 32, 64, 1, 1, 1, 0, 0, 4, 0, ST);
    REFUSED(seam_conv2d_dual_f32, p, p, p, nullptr, nullptr, q, 1, 5, 5, 32, 8, 9, 64, 2, 64, 0, ST);
    REFUSED(seam_conv2d_dual_f32, p, p, p, nullptr, nullptr, q, 1, 5, 5, 32, 9, 8, 64, 2, 64, 0, ST);
    REFUSED(seam_conv2d_dual_f32, p, p, p, nullptr, nullptr, q, 1, 5, 5, 32, 9, 9, 48, 2, 64, 0, ST);
    REFUSED(seam_conv2d_dual_f32, p, p, p, nullptr, nullptr, q, 1, 5, 5, 16, 9, 9, 64, 2, 64, 0, ST);
    REFUSED(seam_conv2d_dual_f16, p, p, p, nullptr, nullptr, q, 1, 5, 5, 64, 8, 9, 64, 2, 64, 0, ST);
    REFUSED(seam_conv2d_dual_f16, p, p, p, nullptr, nullptr, q, 1, 5, 5, 64, 9, 9, 48, 2, 64, 0, ST);
    REFUSED(seam_conv2d_dual_f16, p, p, p, nullptr, nullptr, q, 1, 5, 5, 64, 9, 9, 96, 2, 64, 0, ST);
#undef REFUSED
#undef CALL
}

}  // namespace

template <class... A>
void rec::launch(const char* kern, dim3 grid, dim3 block, const A&... args) {
    ++launches;
    printf(" %s grid=%u,%u,%u block=%u,%u,%u", kern, grid.x, grid.y, grid.z, block.x, block.y, block.z);
    show(args...);
}

int main() {
    const int Ns[] = {1, 2, 3, 40, 70000}, HW[] = {1, 2, 3, 7, 8, 14, 25, 127, 128, 129, 200};
    const int Cs[] = {3, 4, 8, 12, 16, 32, 64, 96, 256}, Ks[] = {0, 1, 14, 63, 64, 65, 128, 192, 256};
    const int G[][3] = {{1, 1, 0}, {1, 2, 0}, {3, 1, 1}, {3, 2, 1}, {5, 2, 1}, {7, 2, 3}};
    const int tiles[] = {0, 256128, 128128, 128064, 64128, 64064};
    int relu = 0;
    for (int tile : tiles) {
        if (seam_set_option("SEAM_CONV_TILE", tile)) return 2;
        printf("SEAM_CONV_TILE %d\n", tile);
        // the launchers' own choice: every H with itself and with its neighbour in the list as W; a forced tile: square maps, and
        // the batch sizes 1, 40 and 70000
        for (int ni = 0; ni < 5; ++ni) {
            if (tile && (ni == 1 || ni == 2)) continue;
            for (int hi = 0; hi < 11; ++hi) for (int wj = 0; wj < (tile ? 1 : 2); ++wj)
                for (int ci = 0; ci < 9; ++ci) for (int K : Ks) for (const auto& g : G) {
                    geometry(Ns[ni], HW[hi], HW[(hi + wj) % 11], Cs[ci], Cs[(ci + 1) % 9], K, g[0], g[1], g[2], relu);
                    relu = (relu + 1) % 3;
                }
        }
    }
    if (seam_set_option("SEAM_CONV_TILE", 0)) return 2;
    refusals();
    fprintf(stderr, "%ld cases (accepted %ld, refused %ld), %ld launches recorded\n", accepted + refused, accepted, refused, launches);
    return 0;
}
