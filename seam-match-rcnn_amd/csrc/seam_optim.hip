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
//
// Clipping by global norm (torch.nn.utils.clip_grad_norm_) and the non-finite guard of the reference loop (stuffs/engine.py:176-181)
// run over the same two tables: seam_grad_norm_f32 leaves the norm, torch's clip coefficient and a finite flag in a device record,
// seam_sgd_step_clip_f32 is the step on g * clip_coef that writes nothing when the record says non-finite and the caller asked to
// skip, seam_grad_scale_f32 is the stand-alone g *= clip_coef.  No float atomics; the norm's summation order is fixed.
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

// the block's two fingerprint sums into its slot of `fp`: one 64-bit atomic pair per block
__device__ __forceinline__ void fp_reduce(unsigned long long fp_old, unsigned long long fp_new, unsigned long long* __restrict__ fp, int tid) {
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
    if (FP) fp_reduce(fp_old, fp_new, fp, tid);
}

// The clipped step (seam_sgd_step_clip_f32): sgd_step_kernel's loop, kept as a kernel of its own so that the unclipped kernel's
// code stays what it was.  The gradient is first multiplied by the record's clip_coef (one rounded multiply: what
// g.mul_(clip_coef) stores); with `skip` and a record whose `finite` is 0 nothing is written but pending_out, and the fingerprint's
// "as written" sum is the "as read" one.  A tensor is "first" when its slot says so or pending_in[t.slot] is set; every chunk of a
// tensor writes the same pending_out[t.slot] (set: the buffer is still unwritten after this launch), so there is no race.
template <bool FP>
__global__ __launch_bounds__(256) void sgd_step_clip_kernel(const seam_sgd_tensor_t* __restrict__ tensors,
                                                            const seam_sgd_chunk_t* __restrict__ chunks, int n_chunks,
                                                            const seam_sgd_groups_t groups, unsigned long long* __restrict__ fp,
                                                            const seam_clip_record_t* __restrict__ rec, int skip_nonfinite,
                                                            const int* __restrict__ pending_in, int* __restrict__ pending_out) {
    const int tid = threadIdx.x;
    unsigned long long fp_old = 0, fp_new = 0;
    const float coef = rec->clip_coef;
    const bool skip = skip_nonfinite != 0 && rec->finite == 0;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const seam_sgd_chunk_t ch = chunks[c];
        const seam_sgd_tensor_t t = tensors[ch.tensor];
        const seam_sgd_group_t gr = groups.g[t.group];
        Hyper h;
        h.lr = gr.lr; h.momentum = gr.momentum; h.omd = gr.one_minus_dampening; h.wd = gr.weight_decay;
        h.nesterov = gr.nesterov != 0; h.maximize = gr.maximize != 0; h.first = gr.first != 0;
        h.has_buf = gr.momentum != 0.f && t.buf != nullptr;
        h.first = h.first || pending_in[t.slot] != 0;
        if (tid == 0) pending_out[t.slot] = (skip && h.has_buf && h.first) ? 1 : 0;
        if (skip) {
            if (FP) {
                const GF* q = (const GF*)(t.p + ch.offset);
                for (int i = tid; i < ch.count; i += 256) {
                    const unsigned long long term = fp_term(q[i], ch.tensor, ch.offset + i);
                    fp_old += term;
                    fp_new += term;
                }
            }
            continue;
        }
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
                const f32x4 gv = __builtin_nontemporal_load(g4 + i) * coef;
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
            update(pv, g[i] * coef, bv, h);
            if (FP) fp_new += fp_term(pv, ch.tensor, ch.offset + i);
            p[i] = pv;
            if (h.has_buf) b[i] = bv;
        }
    }
    if (FP) fp_reduce(fp_old, fp_new, fp, tid);
}

// ---- the global gradient norm ------------------------------------------------------------------------------------------------------
// Stage 1, one fp64 partial per chunk.  A lane adds its elements' exact fp64 squares in index order, the 64 lanes of a wave are
// combined by a fixed butterfly, the four waves in wave order: the partial depends on the data and its alignment only.
// INF: the partial is max |g| (exact in fp64), or NaN when any element is NaN -- carried as a flag, not through a compare.
__device__ __forceinline__ void norm_acc(double& acc, bool& nan, float v, bool inf) {
    if (inf) {
        nan = nan || v != v;
        const double a = (double)__builtin_fabsf(v);
        acc = a > acc ? a : acc;
    } else {
        const double d = (double)v;
        acc = acc + d * d;
    }
}

template <bool INF>
__global__ __launch_bounds__(256) void grad_norm_partial_kernel(const seam_sgd_tensor_t* __restrict__ tensors,
                                                                const seam_sgd_chunk_t* __restrict__ chunks, int n_chunks,
                                                                double* __restrict__ partial) {
    __shared__ double red[4];
    __shared__ int red_nan[4];
    const int tid = threadIdx.x;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const seam_sgd_chunk_t ch = chunks[c];
        const seam_sgd_tensor_t t = tensors[ch.tensor];
        const GF* g = (const GF*)(t.g + ch.offset);
        const int n = ch.count;
        double acc = 0.0;
        bool nan = false;
        int done = 0;
        if (((uintptr_t)g & 15) == 0) {
            const int n4 = n >> 2;
            const GF4* g4 = (const GF4*)g;
#pragma unroll 2
            for (int i = tid; i < n4; i += 256) {
                const f32x4 gv = g4[i];
#pragma unroll
                for (int e = 0; e < 4; ++e) norm_acc(acc, nan, gv[e], INF);
            }
            done = n4 << 2;
        }
        for (int i = done + tid; i < n; i += 256) norm_acc(acc, nan, g[i], INF);
        int nanw = nan ? 1 : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double other = __shfl_xor(acc, o, 64);
            if (INF) {
                acc = other > acc ? other : acc;
                nanw |= __shfl_xor(nanw, o, 64);
            } else {
                acc = acc + other;
            }
        }
        if ((tid & 63) == 0) {
            red[tid >> 6] = acc;
            red_nan[tid >> 6] = nanw;
        }
        __syncthreads();
        if (tid == 0) {
            double r;
            if (INF) {
                r = red[0];
                for (int w = 1; w < 4; ++w) r = red[w] > r ? red[w] : r;
                if (red_nan[0] | red_nan[1] | red_nan[2] | red_nan[3]) r = __builtin_nan("");
            } else {
                r = ((red[0] + red[1]) + red[2]) + red[3];
            }
            partial[c] = r;
        }
        __syncthreads();
    }
}

// Stage 2, one block: lane l combines the partials of chunks [l * per, (l + 1) * per) in chunk order, then the lanes are combined
// by the same fixed butterfly and wave order.  Writes the record.
template <bool INF>
__global__ __launch_bounds__(256) void grad_norm_final_kernel(const double* __restrict__ partial, int n_chunks, int clip, float max_norm,
                                                              int count_mode, seam_clip_record_t* __restrict__ rec) {
    __shared__ double red[4];
    __shared__ int red_nan[4];
    const int tid = threadIdx.x;
    const int per = (n_chunks + 255) / 256;
    const int lo = tid * per;
    const int hi = lo + per < n_chunks ? lo + per : n_chunks;
    double acc = 0.0;
    int nanw = 0;
    for (int i = lo; i < hi; ++i) {
        const double v = partial[i];
        if (INF) {
            nanw |= v != v ? 1 : 0;
            acc = v > acc ? v : acc;
        } else {
            acc = acc + v;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double other = __shfl_xor(acc, o, 64);
        if (INF) {
            acc = other > acc ? other : acc;
            nanw |= __shfl_xor(nanw, o, 64);
        } else {
            acc = acc + other;
        }
    }
    if ((tid & 63) == 0) {
        red[tid >> 6] = acc;
        red_nan[tid >> 6] = nanw;
    }
    __syncthreads();
    if (tid == 0) {
        double r;
        if (INF) {
            r = red[0];
            for (int w = 1; w < 4; ++w) r = red[w] > r ? red[w] : r;
            if (red_nan[0] | red_nan[1] | red_nan[2] | red_nan[3]) r = __builtin_nan("");
        } else {
            r = __builtin_sqrt(((red[0] + red[1]) + red[2]) + red[3]);
        }
        const float total = (float)r;
        // torch: clip_coef = max_norm / (total_norm + 1e-6) is Tensor.__rtruediv__, reciprocal() * max_norm; then clamp(max=1),
        // which keeps NaN.  Every operation rounded to fp32 on its own.
        float coef = 1.f;
        if (clip) {
            const float den = total + 1e-6f;
            const float rcp = 1.f / den;
            coef = rcp * max_norm;
            coef = coef > 1.f ? 1.f : coef;
        }
        const int finite = (total == total && __builtin_fabsf(total) != __builtin_inff()) ? 1 : 0;
        rec->total_norm = total;
        rec->clip_coef = coef;
        rec->finite = finite;
        rec->reserved = 0;
        const unsigned long long bump = finite ? 0ull : 1ull;
        rec->nonfinite_steps = count_mode ? rec->nonfinite_steps + bump : bump;
    }
}

// g *= clip_coef over the tables.  T is the gradients' element type (float).  A template on purpose: hipcc emits templates after
// the plain kernels of a file, in the order of their first use, so this kernel lands behind the step kernels and their code, block
// labels included, stays what tools/isa_same.py compares with.
template <typename T>
__global__ __launch_bounds__(256) void grad_scale_kernel(const seam_sgd_tensor_t* __restrict__ tensors,
                                                         const seam_sgd_chunk_t* __restrict__ chunks, int n_chunks,
                                                         const seam_clip_record_t* __restrict__ rec) {
    typedef __attribute__((address_space(1))) T GT;
    typedef T T4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(1))) T4 GT4;
    const int tid = threadIdx.x;
    const T coef = rec->clip_coef;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const seam_sgd_chunk_t ch = chunks[c];
        const seam_sgd_tensor_t t = tensors[ch.tensor];
        GT* g = (GT*)(const_cast<T*>(t.g) + ch.offset);
        const int n = ch.count;
        int done = 0;
        if (((uintptr_t)g & 15) == 0) {
            const int n4 = n >> 2;
            GT4* g4 = (GT4*)g;
#pragma unroll 2
            for (int i = tid; i < n4; i += 256) g4[i] = g4[i] * coef;
            done = n4 << 2;
        }
        for (int i = done + tid; i < n; i += 256) g[i] = g[i] * coef;
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

int seam_sgd_step_clip_f32(const seam_sgd_tensor_t* tensors, const seam_sgd_chunk_t* chunks, int n_chunks,
                           const seam_sgd_groups_t* groups, unsigned long long* fingerprint, const seam_clip_record_t* record,
                           int skip_nonfinite, const int* pending_in, int* pending_out, void* stream) {
    if (n_chunks < 0 || !groups || groups->n < 0 || groups->n > SEAM_SGD_MAX_SLOTS) return (int)hipErrorInvalidValue;
    if (!record || !pending_in || !pending_out || pending_in == pending_out) return (int)hipErrorInvalidValue;
    if (fingerprint) {
        const hipError_t e = hipMemsetAsync(fingerprint, 0, 2 * SEAM_SGD_FP_SLOTS * sizeof(unsigned long long), (hipStream_t)stream);
        if (e != hipSuccess) return (int)e;
    }
    if (n_chunks == 0) return 0;
    if (!tensors || !chunks) return (int)hipErrorInvalidValue;
    const unsigned grid = n_chunks < MAX_BLOCKS ? (unsigned)n_chunks : (unsigned)MAX_BLOCKS;
    if (fingerprint)
        hipLaunchKernelGGL(sgd_step_clip_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, tensors, chunks, n_chunks,
                           *groups, fingerprint, record, skip_nonfinite, pending_in, pending_out);
    else
        hipLaunchKernelGGL(sgd_step_clip_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, tensors, chunks, n_chunks,
                           *groups, (unsigned long long*)nullptr, record, skip_nonfinite, pending_in, pending_out);
    return (int)hipGetLastError();
}

int64_t seam_grad_norm_workspace_bytes(int n_chunks) {
    return n_chunks < 0 ? -1 : (int64_t)sizeof(double) * (n_chunks > 0 ? n_chunks : 1);
}

int seam_grad_norm_f32(const seam_sgd_tensor_t* tensors, const seam_sgd_chunk_t* chunks, int n_chunks, int norm_inf, int clip,
                       float max_norm, int keep_count, void* workspace, int64_t workspace_bytes, seam_clip_record_t* record,
                       void* stream) {
    if (n_chunks < 0 || !record || !workspace || workspace_bytes < seam_grad_norm_workspace_bytes(n_chunks) ||
        ((uintptr_t)workspace & 7) || ((uintptr_t)record & 7))
        return (int)hipErrorInvalidValue;
    if (n_chunks > 0 && (!tensors || !chunks)) return (int)hipErrorInvalidValue;
    double* partial = (double*)workspace;
    if (n_chunks > 0) {
        const unsigned grid = n_chunks < MAX_BLOCKS ? (unsigned)n_chunks : (unsigned)MAX_BLOCKS;
        if (norm_inf)
            hipLaunchKernelGGL(grad_norm_partial_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, tensors, chunks, n_chunks, partial);
        else
            hipLaunchKernelGGL(grad_norm_partial_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, tensors, chunks, n_chunks, partial);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    if (norm_inf)
        hipLaunchKernelGGL(grad_norm_final_kernel<true>, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, n_chunks, clip, max_norm, keep_count, record);
    else
        hipLaunchKernelGGL(grad_norm_final_kernel<false>, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, n_chunks, clip, max_norm, keep_count, record);
    return (int)hipGetLastError();
}

int seam_grad_scale_f32(const seam_sgd_tensor_t* tensors, const seam_sgd_chunk_t* chunks, int n_chunks,
                        const seam_clip_record_t* record, void* stream) {
    if (n_chunks < 0 || !record) return (int)hipErrorInvalidValue;
    if (n_chunks == 0) return 0;
    if (!tensors || !chunks) return (int)hipErrorInvalidValue;
    const unsigned grid = n_chunks < MAX_BLOCKS ? (unsigned)n_chunks : (unsigned)MAX_BLOCKS;
    hipLaunchKernelGGL(grad_scale_kernel<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, tensors, chunks, n_chunks, record);
    return (int)hipGetLastError();
}

}  // extern "C"
