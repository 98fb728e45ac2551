// seam_tracklets.hip -- the greedy tracklet linking of evaluate_movingfashion.py:166-202 for all products / clips of a call, in two
// forms that take the same decisions: the evaluator's HOST helper (seam_host_build_tracklets, no device code) and its DEVICE twin
// (seam_build_tracklets_f32, one block per segment) for the inference path, where the blocks must not leave the stream.
//
// The linking is a chain of tiny data-dependent decisions over a product's <= a few dozen detections (seed with the most
// confident free detection; repeatedly take, among the free detections of frames that have no member yet, the one most similar to
// ANY current member; link it if that similarity exceeds the threshold, else close the tracklet) -- nothing for a GPU, but in
// Python / NumPy it was what the batched evaluator spent its time on (~0.2 ms per product of interpreter and array-call overhead
// against ~0.02 ms of device work).  Same decisions as the reference's loops, element for element: candidates in ascending
// detection order, rows (current members) in ascending detection order, the FIRST maximum in row-major order wins (np.argmax).
#include <stdint.h>
#include <limits.h>
#include <vector>
#include <algorithm>
#include "seam_hip.h"
#include "seam_device.h"

namespace {

constexpr int TRK_THREADS = 256;
constexpr int TRK_CAP = 2048;          // largest segment: 5 words of LDS per detection (40 KiB of the block's 64 KiB static limit)

// One entry of the two selections (seed: value = confidence, row = 0, col = detection; link: value = best similarity of the
// candidate to a member, row = the lowest member that reaches it, col = the candidate).  col == INT_MAX: no entry.
struct Pick {
    float v;
    int r, c;
};

// a wins over b: the larger value; among equal values the lower row, then the lower column -- the first maximum of the members x
// candidates matrix in row-major order.  Comparisons only; with a NaN neither side wins and the earlier entry stays.
__device__ __forceinline__ bool pick_wins(const Pick& a, const Pick& b) {
    if (a.c == INT_MAX) return false;
    if (b.c == INT_MAX) return true;
    return a.v > b.v || (a.v == b.v && (a.r < b.r || (a.r == b.r && a.c < b.c)));
}

// Block-wide winner, the same in every thread.  `red` holds two sets of one entry per wave, used alternately (`phase`): the
// barrier of the next call orders this call's reads before the writes of the call after it, so one barrier per call is enough.
__device__ __forceinline__ Pick block_pick(Pick p, Pick* red, int& phase) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Pick q;
        q.v = __shfl_xor(p.v, o, 64);
        q.r = __shfl_xor(p.r, o, 64);
        q.c = __shfl_xor(p.c, o, 64);
        if (pick_wins(q, p)) p = q;
    }
    Pick* slot = red + phase * (TRK_THREADS / 64);
    phase ^= 1;
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = p;
    __syncthreads();
    Pick w = slot[0];
#pragma unroll
    for (int i = 1; i < TRK_THREADS / 64; ++i)
        if (pick_wins(slot[i], w)) w = slot[i];
    return w;
}

// One block per segment.  Thread t owns the detections t, t + 256, ...: their state (retired, frame closed, running best) is read
// and written by the owner alone, so only the two selections synchronise the block.  Per link: one row of the similarity block is
// read (coalesced) to update the running best of every candidate -- members x candidates is never rescanned.
__global__ __launch_bounds__(TRK_THREADS) void build_tracklets_kernel(const float* __restrict__ blocks, const int64_t* __restrict__ block_off,
                                                                       const int* __restrict__ seg, const int* __restrict__ imgs,
                                                                       const float* __restrict__ scores, int max_rows, double threshold,
                                                                       int* __restrict__ members, int* __restrict__ track_len,
                                                                       int* __restrict__ n_tracks, int* __restrict__ track_of) {
    __shared__ int s_img[TRK_CAP];
    __shared__ float s_score[TRK_CAP];
    __shared__ float s_bestv[TRK_CAP];
    __shared__ int s_bestr[TRK_CAP];
    __shared__ int s_state[TRK_CAP];        // bit 0: retired (member of a tracklet), bit 1: its frame has a member of the open tracklet
    __shared__ Pick s_red[2 * (TRK_THREADS / 64)];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int o = seg[s];
    const int n = seg[s + 1] - o;
    if (n <= 0) {
        if (tid == 0) n_tracks[s] = 0;
        return;
    }
    if (n > max_rows || n > TRK_CAP) {
        if (tid == 0) n_tracks[s] = -1;
        return;
    }
    const float* sim = blocks + block_off[s];
    for (int j = tid; j < n; j += TRK_THREADS) {
        s_img[j] = imgs[o + j];
        s_score[j] = scores[o + j];
        s_state[j] = 0;
    }
    __syncthreads();                        // s_img is read across owners below
    int phase = 0, left = n, nt = 0, mo = 0;
    while (left > 0) {
        // ---- seed: the most confident free detection, the lowest index among equals
        Pick p = {0.f, 0, INT_MAX};
        for (int j = tid; j < n; j += TRK_THREADS)
            if (!(s_state[j] & 1)) {
                const Pick q = {s_score[j], 0, j};
                if (pick_wins(q, p)) p = q;
            }
        const Pick seed = block_pick(p, s_red, phase);
        if (seed.c == INT_MAX) break;       // cannot happen while left > 0; ends the loop rather than trusting that
        int m = seed.c, len = 0;
        for (;;) {
            // ---- m joins: it retires, closes its frame, and its row updates every candidate's running best
            const int fm = s_img[m];
            const float* row = sim + (size_t)m * n;
            if (tid == 0) {
                members[o + mo + len] = m;
                track_of[o + m] = nt;
            }
            Pick best = {0.f, 0, INT_MAX};
            for (int j = tid; j < n; j += TRK_THREADS) {
                int st = s_state[j];
                if (len == 0) st &= 1;                                  // a new tracklet: every frame is open again
                if (j == m) st |= 1;
                if (s_img[j] == fm) st |= 2;
                s_state[j] = st;
                if (st) continue;
                const float v = row[j];
                if (len == 0 || v > s_bestv[j] || (v == s_bestv[j] && m < s_bestr[j])) {
                    s_bestv[j] = v;
                    s_bestr[j] = m;
                }
                const Pick q = {s_bestv[j], s_bestr[j], j};
                if (pick_wins(q, best)) best = q;
            }
            ++len;
            const Pick w = block_pick(best, s_red, phase);
            // strictly above the threshold, compared in fp64: float(0.3) as a similarity links at the threshold 0.3
            if (w.c == INT_MAX || !((double)w.v > threshold) || len >= n) break;
            m = w.c;
        }
        if (tid == 0) track_len[o + nt] = len;
        ++nt;
        mo += len;
        left -= len;
    }
    for (int j = nt + tid; j < n; j += TRK_THREADS) track_len[o + j] = 0;
    if (tid == 0) n_tracks[s] = nt;
}

}  // namespace

extern "C" {

// blocks: the products' n_s x n_s self-similarity blocks, concatenated (offset of product s = sum of n_t^2, t < s);
// seg [n_seg + 1]: detection offsets; imgs / scores [seg[n_seg]]: frame index and confidence of every detection;
// members_out [seg[n_seg]]: per product (at seg[s]) its detections' LOCAL indices, tracklet after tracklet in creation order, members
// in link order; track_len_out [seg[n_seg]]: per product (at seg[s]) the lengths of its tracklets; n_tracks_out [n_seg].  Returns 0.
int seam_host_build_tracklets(const float* blocks, const int64_t* seg, const int64_t* imgs, const double* scores, int n_seg,
                              double threshold, int32_t* members_out, int32_t* track_len_out, int32_t* n_tracks_out) {
    std::vector<char> free_, open_, present;
    std::vector<int> members, sorted;
    size_t boff = 0;
    for (int s = 0; s < n_seg; ++s) {
        const int64_t o = seg[s];
        const int n = (int)(seg[s + 1] - o);
        const float* sim = blocks + boff;
        boff += (size_t)n * n;
        const int64_t* im = imgs + o;
        const double* sc = scores + o;
        int nfr = 0;
        for (int i = 0; i < n; ++i) nfr = std::max(nfr, (int)im[i] + 1);
        free_.assign(n, 1);
        present.assign(nfr, 0);
        for (int i = 0; i < n; ++i) present[im[i]] = 1;
        int left = n, nt = 0, mo = 0;
        while (left > 0) {
            int start = -1;
            for (int i = 0; i < n; ++i)
                if (free_[i] && (start < 0 || sc[i] > sc[start])) start = i;            // first maximum among the free detections
            members.assign(1, start);
            sorted.assign(1, start);
            open_ = present;
            open_[im[start]] = 0;
            for (;;) {
                float best = 0.f;
                int best_c = -1;
                for (int r : sorted)                                                     // rows in detection order
                    for (int j = 0; j < n; ++j)
                        if (free_[j] && open_[im[j]]) {
                            const float v = sim[(size_t)r * n + j];
                            if (best_c < 0 || v > best) { best = v; best_c = j; }      // strict: the first maximum in row-major order
                        }
                // (the comparison in fp32, as `sub[r, c] > threshold` is with a float32 matrix and a Python float under NumPy 2 promotion)
                if (best_c < 0 || !(best > (float)threshold)) break;
                members.push_back(best_c);
                sorted.insert(std::upper_bound(sorted.begin(), sorted.end(), best_c), best_c);
                open_[im[best_c]] = 0;
            }
            for (int m : members) { free_[m] = 0; members_out[o + mo++] = m; }
            left -= (int)members.size();
            track_len_out[o + nt++] = (int)members.size();
        }
        n_tracks_out[s] = nt;
    }
    return 0;
}

int seam_build_tracklets_max_rows(void) { return TRK_CAP; }

int seam_build_tracklets_f32(const float* blocks, const int64_t* block_off, const int* seg, const int* imgs, const float* scores,
                             int n_seg, int max_rows, double threshold, int32_t* members, int32_t* track_len, int32_t* n_tracks,
                             int32_t* track_of, void* stream) {
    if (n_seg == 0) return 0;
    if (n_seg < 0 || max_rows < 0 || max_rows > TRK_CAP) return (int)hipErrorInvalidValue;
    if (!block_off || !seg || !n_tracks) return (int)hipErrorInvalidValue;
    if (max_rows > 0 && (!blocks || !imgs || !scores || !members || !track_len || !track_of)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(build_tracklets_kernel, dim3((unsigned)n_seg), dim3(TRK_THREADS), 0, (hipStream_t)stream, blocks, block_off, seg,
                       imgs, scores, max_rows, threshold, members, track_len, n_tracks, track_of);
    return (int)hipGetLastError();
}

}  // extern "C"
