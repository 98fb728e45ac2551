// seam_optim.hip -- the optimizer step of the training loop (ref stuffs/engine.py:62-64: optimizer.step() of
// torch.optim.SGD(params, lr, momentum=0.9), train_matchrcnn.py:70-72) as ONE launch over every trainable parameter.
//
// Two device tables describe the work.  `tensors`: parameter, gradient and momentum-buffer pointer, element count and the slot of
// the tensor's hyper-parameters.  `chunks`: (tensor, offset, count) of every SEAM_SGD_CHUNK-element piece of every tensor.  A block
// walks chunks blockIdx.x, blockIdx.x + gridDim.x, ...: the 12.8 M-element fc6 weight and a 14-element bias are the same kind of
// work item, and the grid is sized by the bytes, not by the tensor count.  The hyper-parameters travel by value in the kernel
// arguments, so a learning-rate schedule costs no upload and no table rebuild.
//
// Arithmetic: torch.optim.SGD's, every multiply and every add rounded on its own (torch's add_(x, alpha=a) is a * x rounded, then
// the sum rounded, on the CPU's vector path).  Plain operators under FP_CONTRACT OFF give that; __fmul_rn / __fadd_rn do not under
// hipcc (csrc/seam_masks.hip says why).
//
// Pointers are only 4-byte aligned in general (the heads' gradients are row slices of one GEMM output).  A chunk whose three
// pointers are all 16-byte aligned moves 16 bytes per lane and finishes its last count % 4 elements one by one; any other chunk
// moves 4 bytes per lane.  Chunk offsets are multiples of SEAM_SGD_CHUNK, so a tensor's chunks share its alignment.  No byte
// outside [p, p + numel) / [buf, buf + numel) is written and none outside the three ranges is read.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "seam_device.h"
#include "seam_hip.h"

#pragma STDC FP_CONTRACT OFF

namespace {

constexpr int CHUNK = 8192;            // elements per chunk: 32 KiB per stream, 8 x 16 bytes per lane
constexpr int MAX_BLOCKS = 2048;       // 8 blocks per CU: the streaming-kernel grid of the guides

typedef __attribute__((address_space(1))) float GF;
typedef __attribute__((address_space(1))) f32x4 GF4;

struct Hyper {
    float lr, momentum, omd, wd;
    bool nesterov, maximize, first, has_buf;
};

__device__ __forceinline__ void update(float& p, float grad, float& buf, const Hyper& h) {
    float g = h.maximize ? -grad : grad;
    if (h.wd != 0.f) {
        const float t = h.wd * p;
        g = g + t;
    }
    if (h.has_buf) {
        if (h.first) {
            buf = g;
        } else {
            const float a = h.momentum * buf;
            const float b = h.omd * g;
            buf = a + b;
        }
        if (h.nesterov) {
            const float t = h.momentum * buf;
            g = g + t;
        } else {
            g = buf;
        }
    }
    const float s = h.lr * g;
    p = p - s;
}

// fingerprint term of element `pos` of tensor `tensor`: its bit pattern times an odd weight that depends on where it sits.  The
// terms are summed modulo 2^64, so the sum does not depend on which block or lane added what.
__device__ __forceinline__ unsigned long long fp_term(float v, int tensor, long long pos) {
    const unsigned w = (((unsigned)tensor * 0x9E3779B1u + (unsigned)pos) << 1) | 1u;
    return (unsigned long long)__builtin_bit_cast(unsigned, v) * (unsigned long long)w;
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// FP: also sum the fingerprint terms of every parameter element as read (fp[2 s]) and as written (fp[2 s + 1]) into slot
// s = blockIdx.x % SEAM_SGD_FP_SLOTS of `fp` (one 64-bit atomic pair per block): what the caller compares with the previous step's
// "as written" sum to learn whether anything but this kernel wrote the parameters in between.  No extra memory traffic.
template <bool FP>
__global__ __launch_bounds__(256) void sgd_step_kernel(const seam_sgd_tensor_t* __restrict__ tensors,
                                                       const seam_sgd_chunk_t* __restrict__ chunks, int n_chunks,
                                                       const seam_sgd_groups_t groups, unsigned long long* __restrict__ fp) {
    const int tid = threadIdx.x;
    unsigned long long fp_old = 0, fp_new = 0;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const seam_sgd_chunk_t ch = chunks[c];
        const seam_sgd_tensor_t t = tensors[ch.tensor];
        const seam_sgd_group_t gr = groups.g[t.group];
        Hyper h;
        h.lr = gr.lr; h.momentum = gr.momentum; h.omd = gr.one_minus_dampening; h.wd = gr.weight_decay;
        h.nesterov = gr.nesterov != 0; h.maximize = gr.maximize != 0; h.first = gr.first != 0;
        h.has_buf = gr.momentum != 0.f && t.buf != nullptr;
        // the table's pointers are generic to the compiler: say that they are global memory (global_load / global_store)
        GF* p = (GF*)(t.p + ch.offset);
        const GF* g = (const GF*)(t.g + ch.offset);
        GF* b = h.has_buf ? (GF*)(t.buf + ch.offset) : nullptr;
        const int n = ch.count;
        const bool read_buf = h.has_buf && !h.first;
        const uintptr_t bits = (uintptr_t)p | (uintptr_t)g | (uintptr_t)b;
        int done = 0;
        if ((bits & 15) == 0) {
            const int n4 = n >> 2;
            GF4* p4 = (GF4*)p;
            const GF4* g4 = (const GF4*)g;
            GF4* b4 = (GF4*)b;
#pragma unroll 2
            for (int i = tid; i < n4; i += 256) {
                f32x4 pv = p4[i];
                const f32x4 gv = __builtin_nontemporal_load(g4 + i);
                f32x4 bv = {0.f, 0.f, 0.f, 0.f};
                if (read_buf) bv = b4[i];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float pe = pv[e], be = bv[e];
                    if (FP) fp_old += fp_term(pe, ch.tensor, ch.offset + 4 * i + e);
                    update(pe, gv[e], be, h);
                    if (FP) fp_new += fp_term(pe, ch.tensor, ch.offset + 4 * i + e);
                    pv[e] = pe;
                    bv[e] = be;
                }
                p4[i] = pv;
                if (h.has_buf) b4[i] = bv;
            }
            done = n4 << 2;
        }
        for (int i = done + tid; i < n; i += 256) {
            float pv = p[i], bv = 0.f;
            if (read_buf) bv = b[i];
            if (FP) fp_old += fp_term(pv, ch.tensor, ch.offset + i);
            update(pv, g[i], bv, h);
            if (FP) fp_new += fp_term(pv, ch.tensor, ch.offset + i);
            p[i] = pv;
            if (h.has_buf) b[i] = bv;
        }
    }
    if (FP) {
        __shared__ unsigned long long red[8];
        fp_old = wave_sum_u64(fp_old);
        fp_new = wave_sum_u64(fp_new);
        if ((tid & 63) == 0) {
            red[2 * (tid >> 6)] = fp_old;
            red[2 * (tid >> 6) + 1] = fp_new;
        }
        __syncthreads();
        if (tid < 2) atomicAdd(fp + 2 * (blockIdx.x % SEAM_SGD_FP_SLOTS) + tid, red[tid] + red[2 + tid] + red[4 + tid] + red[6 + tid]);
    }
}

}  // namespace

extern "C" {

int seam_sgd_chunk_elems(void) { return CHUNK; }

int seam_sgd_step_f32(const seam_sgd_tensor_t* tensors, const seam_sgd_chunk_t* chunks, int n_chunks,
                      const seam_sgd_groups_t* groups, unsigned long long* fingerprint, void* stream) {
    if (n_chunks < 0 || !groups || groups->n < 0 || groups->n > SEAM_SGD_MAX_SLOTS) return (int)hipErrorInvalidValue;
    if (fingerprint) {
        const hipError_t e = hipMemsetAsync(fingerprint, 0, 2 * SEAM_SGD_FP_SLOTS * sizeof(unsigned long long), (hipStream_t)stream);
        if (e != hipSuccess) return (int)e;
    }
    if (n_chunks == 0) return 0;
    if (!tensors || !chunks) return (int)hipErrorInvalidValue;
    const unsigned grid = n_chunks < MAX_BLOCKS ? (unsigned)n_chunks : (unsigned)MAX_BLOCKS;
    if (fingerprint)
        hipLaunchKernelGGL(sgd_step_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, tensors, chunks, n_chunks, *groups,
                           fingerprint);
    else
        hipLaunchKernelGGL(sgd_step_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, tensors, chunks, n_chunks, *groups,
                           (unsigned long long*)nullptr);
    return (int)hipGetLastError();
}

}  // extern "C"
