// Prints what the host plans of the split 1x1 family (csrc/seam_pwsx.hip: sxpc_dual_plan, sxpc_up_plan, stem_sxpc_plan) decide over a
// sweep of geometries: per call the return code and, when accepted, every filled field by name.  Two builds of the kernel file are
// compared by diffing the two outputs (profiles/sxpc_fold.txt).  Only host code runs, no GPU is needed (the device code is compiled
// along: with --cuda-host-only the link misses the fat binary the host object refers to):
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude -Iseam-match-rcnn_amd/csrc
//         tools/sxpc_plan_dump.hip -o sxpc_plan_dump && ./sxpc_plan_dump > plans.txt
#include "seam_pwsx.hip"
#include <cstdio>

namespace {

long cases = 0;

template <class Src>
void show(int rc, const SxpcArgs& a, const Src& s) {
    ++cases;
    if (rc) { printf(" rc=%d\n", rc); return; }
    printf(" rc=0 M=%d C=%d K=%d tiles_n=%d nchunks=%d total_tiles=%d m_tiles_n=%u img_bytes=%llu N=%d HoWo=%u Wo=%u m_howo=%u one_howo=%u"
           " thr=%u m_wo=%u one_wo=%u img_step=%u row_step=%u px_step=%u", a.M, a.C, a.K, a.tiles_n, a.nchunks, a.total_tiles, a.m_tiles_n,
           s.img_bytes, s.N, s.HoWo, (unsigned)s.Wo, s.m_howo, s.one_howo, s.thr, s.m_wo, s.one_wo, s.img_step, s.row_step, s.px_step);
}

void dual(long long N, long long Ho, long long Wo, int C1, long long H2, long long W2, int C2, int st, int K, int min_c = 256) {
    SxpcArgs a{}; SxpcDual d{};
    printf("dual %lld %lld %lld %d %lld %lld %d %d %d %d:", N, Ho, Wo, C1, H2, W2, C2, st, K, min_c);
    const int rc = sxpc_dual_plan(a, d, N, Ho, Wo, C1, H2, W2, C2, st, K, min_c);
    show(rc, a, d);
    if (!rc) printf(" C1=%d n1=%d\n", d.C1, d.n1);
}

void up(long long N, long long Ho, long long Wo, int C, int K, long long rH, long long rW) {
    SxpcArgs a{}; SxpcUp u{};
    printf("up %lld %lld %lld %d %d %lld %lld:", N, Ho, Wo, C, K, rH, rW);
    const int rc = sxpc_up_plan(a, u, N, Ho, Wo, C, K, rH, rW);
    show(rc, a, u);
    if (!rc) printf(" Ho=%d rH=%d rW=%d\n", u.Ho, u.rH, u.rW);
}

void stem(long long N, long long Hs, long long Ws) {
    SxpcArgs a{}; SxpcDual d{};
    printf("stem %lld %lld %lld:", N, Hs, Ws);
    const int rc = stem_sxpc_plan(a, d, N, Hs, Ws);
    show(rc, a, d);
    if (!rc) printf(" C1=%d n1=%d\n", d.C1, d.n1);
}

}  // namespace

int main() {
    const long long Ns[] = {1, 2, 3, 40, 70000}, HW[] = {1, 2, 3, 7, 11, 25, 50, 127, 128, 129, 200};
    const int Cs[] = {32, 64, 128, 256}, Ks[] = {64, 96, 128, 256};
    for (long long N : Ns) for (long long Ho : HW) for (long long Wo : HW) {
        for (int st = 1; st <= 2; ++st) for (int less = 0; less <= 1; ++less) for (int C1 : Cs) for (int C2 : Cs) for (int K : Ks) {
            dual(N, Ho, Wo, C1, (Ho - 1) * st + 1 - less, (Wo - 1) * st + 1 - less, C2, st, K);
            if (C1 == 64 && C2 == 64 && st == 1) dual(N, Ho, Wo, C1, Ho - less, Wo - less, C2, 1, K, 128);      // the `short` entry
        }
        const long long rHs[] = {1, (Ho + 1) / 2, Ho}, rWs[] = {1, (Wo + 1) / 2, Wo};
        for (long long rH : rHs) for (long long rW : rWs) for (int C : Cs) for (int K : Ks) up(N, Ho, Wo, C, K, rH, rW);
        stem(N, Ho, Wo);
    }
    // the refusal rows (and their accepted neighbours) of tests/test_sxpc_dual_host.py, test_sxpc_up_host.py and test_sxpc64_host.py
    const long long D[][9] = {{2, 5, 7, 32, 10, 13, 256, 2, 128}, {2, 5, 7, 64, 10, 13, 128, 2, 128}, {2, 5, 7, 64, 10, 13, 192, 2, 96},
        {2, 5, 7, 64, 8, 13, 192, 2, 128}, {2, 5, 7, 64, 10, 12, 192, 2, 128}, {2, 5, 7, 64, 10, 13, 192, 0, 128}, {0, 5, 7, 64, 10, 13, 192, 2, 128},
        {2, 0, 7, 64, 10, 13, 192, 2, 128}, {2, 5, 7, 64, 0, 13, 192, 2, 128}, {2, 8, 8, 64, 724, 724, 1024, 2, 128}, {1, 8, 8, 64, 1024, 1024, 1024, 2, 128},
        {70000, 200, 200, 64, 200, 200, 192, 1, 128}, {2, 5, 7, 64, 10, 13, 192, 2, 128}, {80, 100, 100, 192, 200, 200, 256, 1, 128},
        {80, 25, 25, 192, 50, 50, 1024, 1, 128}, {18, 125, 125, 192, 250, 250, 1024, 1, 128}, {1, 8, 8, 192, 724, 724, 1024, 1, 128},
        {2, 8, 8, 192, 724, 724, 1024, 1, 128}, {1, 8, 8, 192, 1024, 1024, 1024, 1, 128}, {200, 1, 1, 192, 2048, 2048, 64, 1, 128}, {200, 1, 1, 192, 16, 16, 2048, 1, 128}};
    for (const auto& r : D) dual(r[0], r[1], r[2], (int)r[3], r[4], r[5], (int)r[6], (int)r[7], (int)r[8]);
    const long long U[][7] = {{1, 16, 16, 256, 128, 8, 8}, {3, 5, 7, 320, 256, 3, 4}, {2, 25, 25, 256, 128, 13, 13}, {1, 13, 9, 256, 128, 5, 4}, {300, 1, 1, 256, 128, 1, 1},
        {130, 3, 1, 256, 128, 2, 1}, {1, 43, 3, 256, 384, 22, 2}, {4, 100, 100, 256, 256, 50, 50}, {80, 200, 200, 256, 256, 100, 100}, {80, 100, 100, 512, 256, 50, 50},
        {80, 50, 50, 1024, 256, 25, 25}, {2, 5, 7, 192, 128, 3, 4}, {2, 5, 7, 256, 192, 3, 4}, {2, 5, 7, 288, 128, 3, 4}, {2, 5, 7, 256, 128, 0, 4}, {2, 5, 7, 256, 128, 3, 0},
        {0, 5, 7, 256, 128, 3, 4}, {2, 0, 7, 256, 128, 3, 4}, {3, 8, 8, 256, 128, 1200, 1200}, {1, 8, 8, 256, 128, 2048, 2048}, {2, 8, 8, 256, 128, 1200, 1200},
        {70000, 200, 200, 256, 128, 100, 100}};
    for (const auto& r : U) up(r[0], r[1], r[2], (int)r[3], (int)r[4], r[5], r[6]);
    const long long S[][3] = {{80, 400, 400}, {3, 3, 5}, {1, 7, 1}, {1, 1, 1}, {1, 16, 8}, {0, 8, 8}, {1, 0, 8}, {1, 8, -2}, {1, 1 << 16, 1 << 16}};
    for (const auto& r : S) stem(r[0], r[1], r[2]);
    fprintf(stderr, "%ld cases\n", cases);
    return 0;
}
