// seam_device.h -- the device-side primitives more than one kernel file uses: vector types, LDS / scheduling macros, the persistent
// block's tile range, packed-fp32 ops, fixed-order sums.  Kernels, their argument structs and their constants stay in their files.
#pragma once
#include <hip/hip_runtime.h>

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

#define LDSQ __attribute__((address_space(3)))
#define SB() __builtin_amdgcn_sched_barrier(0)
// workgroup barrier that waits for the wave's own LDS traffic only: __syncthreads() also drains vmcnt, i.e. the global loads a
// producer / consumer kernel keeps in flight across the barrier on purpose
#define LDS_BAR() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
// one s_memtime stamp of the experiment builds (-DSEAM_*_TRACE, tools/experiments/*_abl.sh): `cap` stamps per wave, tag in the top
// byte.  A kernel file maps its own stamp macro to this one in such a build and to nothing otherwise.
#define SEAM_STAMP(cap, tag) do { if (tr_on) { const unsigned long long tm_ = __builtin_amdgcn_s_memtime(); if (lane == 0 && tr_k < cap) p.trace[wave * cap + tr_k] = tm_ | ((unsigned long long)(tag) << 56); ++tr_k; } } while (0)

// buffer-load / store byte offset that is out of range for every descriptor here (num_records <= 2^31; the launchers reject larger
// operands): the hardware returns zeros / drops the store, so padding and tails need no branch
constexpr unsigned kOob = 0x80000000u;

// LDS access by 32-bit byte address (the K phase keeps its fragment pointers as plain integers: hipcc otherwise re-derives
// "base + index" per access with a vector add, and every vector-ALU instruction between two MFMAs idles the matrix pipe)
typedef __attribute__((address_space(3))) f32x4 lds_f32x4;
typedef __attribute__((address_space(3))) char lds_char;
__device__ __forceinline__ f32x4 lds_read16(int addr) { return *reinterpret_cast<lds_f32x4*>((unsigned)addr); }

// The tiles of one block of a persistent grid: blocks are dealt to the 8 XCDs round robin, so XCD x (= blockIdx & 7) owns a
// contiguous range of the launch's tiles (neighbouring tiles share operands in that XCD's L2) and its blocks walk the range
// interleaved: tile0(), tile0() + stride, ... (ntiles of them; 0: the block has nothing to do and returns).  tile0() is a sum
// left to the caller so that it is formed behind that early return, where the kernels have always formed it.
struct XcdTiles {
    int start, slot, ntiles, stride;
    __device__ __forceinline__ int tile0() const { return start + slot; }
};
__device__ __forceinline__ XcdTiles xcd_tiles(int total_tiles) {
    const int T = total_tiles, G = gridDim.x;
    const int xcd = blockIdx.x & 7, sl0 = blockIdx.x >> 3;
    const int q8 = T >> 3, rem8 = T & 7;
    const int cnt = q8 + (xcd < rem8 ? 1 : 0);
    const int start = xcd < rem8 ? xcd * (q8 + 1) : rem8 * (q8 + 1) + (xcd - rem8) * q8;
    const int S = (G >> 3) + ((G & 7) > xcd ? 1 : 0);
    return {start, sl0, sl0 < cnt ? (cnt - sl0 + S - 1) / S : 0, S};
}

// Packed-fp32 VALU ops for the Winograd input transforms.  Written as asm because the DAG combiner scalarises a <4 x float> op
// whose lanes are extracted one by one (each feeds its own MFMA): 32 v_fma/v_sub per transform instead of 16 packed ones.
__device__ __forceinline__ f32x2 pk_fma(f32x2 a, f32x2 b, f32x2 c) {
    f32x2 d;
    asm("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
__device__ __forceinline__ f32x2 pk_add(f32x2 a, f32x2 b) {
    f32x2 d;
    asm("v_pk_add_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
    return d;
}
__device__ __forceinline__ f32x2 pk_sub(f32x2 a, f32x2 b) {
    f32x2 d;
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(d) : "v"(a), "v"(b));
    return d;
}
__device__ __forceinline__ f32x4 fma4(f32x2 c, f32x4 b, f32x4 a) {        // a + c * b
    const f32x2 lo = pk_fma(c, __builtin_shufflevector(b, b, 0, 1), __builtin_shufflevector(a, a, 0, 1));
    const f32x2 hi = pk_fma(c, __builtin_shufflevector(b, b, 2, 3), __builtin_shufflevector(a, a, 2, 3));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// block-wide sum of one value per thread (256 threads), summed left to right, result broadcast; `red` = 4 floats of LDS.  No
// barrier behind the reads of `red`: the next call's first barrier orders them before its writes.
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}
