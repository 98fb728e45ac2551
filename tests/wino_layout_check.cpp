// Invariants of csrc/seam_wino_layout.h, checked on the host alone: the header and nothing else of the library.  For each of the
// three kernel forms, every tile grid up to BOUND x BOUND and N in {1, 3, 8}, whatever choose_layout returns must describe blocks
// that compute every tile exactly once within the form's budgets -- with 4 KiB images and, on the grids up to BOUND / 2, with images
// of 900 MiB in / 700 MiB out, of which a stacked block may span two and no more.  tests/test_wino_layout_host.py builds this with
// -fsanitize=address,undefined and runs it.  usage: wino_layout_check [BOUND]; exit code 1 and one line per broken case.
#include "seam_wino_layout.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace seam_wino_layout;

namespace {

constexpr size_t OOB = 0x80000000u;       // the kernels' out-of-range byte offset
long failures = 0;

struct Case { const char* form; int n, tx, ty; size_t in_bytes, out_bytes; };
long g_limited = 0;                       // stacked layouts of small images whose G the large images do not allow

void fail(const Case& c, const char* what) {
    if (++failures <= 20) printf("%s N=%d tiles %d x %d, %zu B images: %s\n", c.form, c.n, c.tx, c.ty, c.in_bytes, what);
}
#define CHECK(cond) do { if (!(cond)) fail(c, #cond); } while (0)

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// regions: every tile of the grid lies in exactly one block of one region
void check_regions(const Case& c, const Form& f, const Layout& L) {
    CHECK(L.stack == 0 && L.G == 1 && L.nreg >= 1 && L.nreg <= 3);
    std::vector<int> seen((size_t)c.tx * c.ty, 0);
    long per_img = 0;
    for (int r = 0; r < L.nreg; ++r) {
        CHECK(patch_ok(f, L.TX[r], L.TY[r]));
        CHECK(0 <= L.rx0[r] && L.rx0[r] < L.rxe[r] && L.rxe[r] <= c.tx && 0 <= L.ry0[r] && L.ry0[r] < L.rye[r] && L.rye[r] <= c.ty);
        CHECK(L.bx[r] == ceil_div(L.rxe[r] - L.rx0[r], L.TX[r]) && L.by[r] == ceil_div(L.rye[r] - L.ry0[r], L.TY[r]));
        per_img += (long)L.bx[r] * L.by[r];
        for (int byi = 0; byi < L.by[r]; ++byi)
            for (int bxi = 0; bxi < L.bx[r]; ++bxi)                        // the kernel's slots: tiles of the patch below the region's end
                for (int y = L.ry0[r] + byi * L.TY[r]; y < L.ry0[r] + (byi + 1) * L.TY[r] && y < L.rye[r]; ++y)
                    for (int x = L.rx0[r] + bxi * L.TX[r]; x < L.rx0[r] + (bxi + 1) * L.TX[r] && x < L.rxe[r]; ++x) ++seen[(size_t)y * c.tx + x];
    }
    bool once = true;
    for (int v : seen) once = once && v == 1;
    CHECK(once);
    CHECK(L.per_img == per_img && L.blocks == per_img * c.n);
    if (L.nreg > 1) {                                                      // a main region beside strips is an exact multiple of its patch
        CHECK(L.rx0[0] == 0 && L.ry0[0] == 0 && L.rxe[0] % L.TX[0] == 0 && L.rye[0] % L.TY[0] == 0);
        CHECK(L.bx[0] * L.TX[0] == L.rxe[0] && L.by[0] * L.TY[0] == L.rye[0]);
    }
}

// stacked: TY consecutive rows of the batch's N * tiles_y tile rows per block, at full width
void check_stacked(const Case& c, const Form& f, const Layout& L, const Layout& regions) {
    const int TY = L.TY[0], t = c.ty, pitch = 2 * t + 2;
    CHECK(L.stack == 1 && L.nreg == 1 && L.TX[0] == c.tx && TY >= 1 && L.TX[0] * TY <= f.slots);
    CHECK(fits(f, L.TX[0], L.PH));
    CHECK(L.blocks == ((long)c.n * t + TY - 1) / TY);
    CHECK(L.blocks < regions.blocks);
    int g_need = 0, ph_need = 0;
    for (long b = 0; b < L.blocks; ++b) {                                  // the images and the padded rows a block's real tile rows span
        const long R0 = b * TY, R1 = (R0 + TY < (long)c.n * t ? R0 + TY : (long)c.n * t) - 1;
        const int n0 = (int)(R0 / t), n1 = (int)(R1 / t);
        const int span = pitch * (n1 - n0) + 2 * (int)(R1 - (long)n1 * t) + 4 - 2 * (int)(R0 - (long)n0 * t);
        if (n1 - n0 + 1 > g_need) g_need = n1 - n0 + 1;
        if (span > ph_need) ph_need = span;
    }
    CHECK(L.G >= g_need && L.PH >= ph_need);
    CHECK((size_t)L.G * c.in_bytes < OOB && (size_t)L.G * c.out_bytes < OOB);      // one buffer descriptor spans the block's images
}

void sweep(const char* name, const Form& f, int bound, size_t in_bytes, size_t out_bytes) {
    static const int Ns[] = {1, 3, 8};
    for (int n : Ns)
        for (int ty = 1; ty <= bound; ++ty)
            for (int tx = 1; tx <= bound; ++tx) {
                const Case c{name, n, tx, ty, in_bytes, out_bytes};
                const Layout L = choose_layout(f, n, tx, ty, in_bytes, out_bytes, OOB);
                if (L.stack) check_stacked(c, f, L, choose_layout(f, n, tx, ty, in_bytes, out_bytes, 0));   // oob = 0: no image count passes, so regions
                else check_regions(c, f, L);
                if (in_bytes > 4096) {
                    const Layout small = choose_layout(f, n, tx, ty, 4096, 4096, OOB);
                    if (small.stack && ((size_t)small.G * in_bytes >= OOB || (size_t)small.G * out_bytes >= OOB)) ++g_limited;
                }
            }
}

}  // namespace

int main(int argc, char** argv) {
    const int bound = argc > 1 ? atoi(argv[1]) : 70;
    const struct { const char* name; const Form& f; } forms[] = {{"F(2x2) MT=1", F22_MT1}, {"F(2x2) MT=2", F22_MT2}, {"F(2x4)", F24}};
    for (const auto& fm : forms) {
        sweep(fm.name, fm.f, bound, 4096, 4096);
        sweep(fm.name, fm.f, bound / 2, (size_t)900 << 20, (size_t)700 << 20);
    }
    if (bound >= 8 && g_limited == 0) { printf("the large images limited no stacked layout: the G x image-bytes rule was not exercised\n"); ++failures; }
    printf("large images: %ld stacked layouts of the small images span more images than one descriptor holds\n", g_limited);
    printf("%d x %d tile grids, 3 forms, N in {1, 3, 8}: %ld failures\n", bound, bound, failures);
    return failures ? 1 : 0;
}
