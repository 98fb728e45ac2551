// seam_repack.hip -- every fp32 weight-pack form of a list of layers in ONE launch: the in-place refresh of the packed weights
// after an optimizer step (ops.PackPlan).  A device table holds one job per (layer, form): source, destination, the dimensions the
// form needs and the job's block range.  A block finds its job by binary search over the first blocks and grid-strides over the
// job's items with the item functions of seam_pack_items.h -- the functions the per-layer pack kernels run, so the bytes written
// are those of the per-layer ABI calls.  The three-plane split twin (SEAM_REPACK_SPLIT3) computes each value of the exact pack
// from the source and splits it, so it does not wait for another job of the same launch; the fragment-order split form of
// conv1x1_sxpc (SEAM_REPACK_SXPC; SEAM_REPACK_SXPC64: its 64-row and two-chunk forms) reads the row-major source itself.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "seam_device.h"
#include "seam_hip.h"
#include "seam_pack_items.h"

namespace {

constexpr int JOB_BLOCKS = 512;        // blocks per job at the most (a job's threads stride over its items beyond that)

__global__ __launch_bounds__(256) void repack_many_kernel(const seam_repack_job_t* __restrict__ jobs, int n_jobs) {
    int lo = 0, hi = n_jobs;           // the last job whose first block is <= blockIdx.x
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (jobs[mid].first_block <= (int)blockIdx.x) lo = mid; else hi = mid;
    }
    const seam_repack_job_t j = jobs[lo];
    const size_t i0 = (size_t)((int)blockIdx.x - j.first_block) * 256 + threadIdx.x;
    const size_t step = (size_t)j.n_blocks * 256;
    const size_t total = (size_t)j.items;
    const float* src = j.src;
    switch (j.form) {
    case SEAM_REPACK_IGEMM: {
        const int nk = j.kred / 32, bn = j.rows % 128 == 0 ? 128 : 64;
        float* out = (float*)j.dst;
        for (size_t i = i0; i < total; i += step) out[i] = seam_pack::igemm_value<32>(src, i, j.K, j.Cin, j.R, j.S, j.Cstore, nk, bn, j.mode);
        break;
    }
    case SEAM_REPACK_SPLIT3: {
        const int nk = j.kred / 32, bn = j.rows % 128 == 0 ? 128 : 64;
        unsigned short* out = (unsigned short*)j.dst;
        for (size_t i = i0; i < total; i += step)
            seam_pack::split3_item(seam_pack::igemm_value<32>(src, i, j.K, j.Cin, j.R, j.S, j.Cstore, nk, bn, j.mode), out, i, bn);
        break;
    }
    case SEAM_REPACK_WINO:
        for (size_t i = i0; i < total; i += step) seam_pack::wino_item(src, (float*)j.dst, i, j.K, j.Cin, j.Cstore / 8, j.mode);
        break;
    case SEAM_REPACK_WINO24:
        for (size_t i = i0; i < total; i += step) seam_pack::wino24_item(src, (float*)j.dst, i, j.K, j.Cin, j.Cstore / 8, j.mode);
        break;
    case SEAM_REPACK_W24SX:
        for (size_t i = i0; i < total; i += step) seam_pack::wino24sx_item(src, (unsigned short*)j.dst, i, j.K, j.Cin, j.Cstore / 16, j.mode);
        break;
    case SEAM_REPACK_PC:
        for (size_t i = i0; i < total; i += step) seam_pack::pwpc_item(src, (float*)j.dst, i, j.Cstore);
        break;
    case SEAM_REPACK_SXPC:
    case SEAM_REPACK_SXPC64:
        for (size_t i = i0; i < total; i += step) seam_pack::sxpc_item(src, (unsigned short*)j.dst, i, j.Cstore);
        break;
    case SEAM_REPACK_SW:
        for (size_t i = i0; i < total; i += step) seam_pack::sw_item(src, j.scale, (float*)j.dst, i, j.Cstore);
        break;
    case SEAM_REPACK_NARROW:
        for (size_t i = i0; i < total; i += step) seam_pack::narrow_item(src, (float*)j.dst, (int)i, j.K, j.Cstore);
        break;
    default:
        break;
    }
}

// items of a job (0: the job is refused), with kred / rows filled in for the implicit-GEMM forms
long long job_items(seam_repack_job_t& j) {
    if (!j.src || !j.dst || j.K < 1 || j.Cin < 1 || j.Cstore < j.Cin) return 0;
    const bool one = j.R == 1 && j.S == 1, plain = j.Cstore == j.Cin && j.mode == 0 && one;
    switch (j.form) {
    case SEAM_REPACK_IGEMM:
    case SEAM_REPACK_SPLIT3: {
        if (j.R < 1 || j.S < 1 || (j.Cstore % 4) || (j.Cstore >= 32 && j.Cstore % 32) || j.mode < 0 || j.mode > 2) return 0;
        if (j.mode == 1 && (!one || j.K % 4)) return 0;
        if ((long long)j.R * j.S * j.Cstore > (1 << 24)) return 0;
        j.kred = seam_conv_kred(j.Cstore, j.R, j.S);
        j.rows = seam_conv_rows_padded(j.K);
        return (long long)j.rows * j.kred;
    }
    case SEAM_REPACK_WINO:
    case SEAM_REPACK_WINO24:
        if (j.R != 3 || j.S != 3 || (j.mode != 0 && j.mode != 2) || !seam_wino_supported(j.Cstore, j.K, 3, 3, 1)) return 0;
        if ((j.K % 32) || (j.Cstore % 8)) return 0;
        return (long long)(j.K / 32) * (j.Cstore / 8) * 64;
    case SEAM_REPACK_W24SX:
        if (j.R != 3 || j.S != 3 || (j.mode != 0 && j.mode != 2) || !seam_conv3x3_wino24sx_supported(1, 16, 16, j.Cstore, j.K, 1, 1)) return 0;
        return (long long)(j.K / 32) * (j.Cstore / 16) * 64;
    case SEAM_REPACK_PC:
        if (!plain || (j.K % 128) || (j.Cstore % 128) || (((uintptr_t)j.src | (uintptr_t)j.dst) & 15)) return 0;
        return (long long)j.K * j.Cstore / 4;
    case SEAM_REPACK_SXPC:
        if (!plain || !seam_conv1x1_sxpc_supported(1, j.Cstore, j.K)) return 0;
        return (long long)j.K * j.Cstore / 8;
    case SEAM_REPACK_SXPC64:
        if (!plain || !(seam_conv1x1_sxpc64_supported(1, j.Cstore, j.K) || seam_conv1x1_sxpc_short_supported(1, j.Cstore, j.K))) return 0;
        return (long long)j.K * j.Cstore / 8;
    case SEAM_REPACK_SW:
        if (!plain) return 0;
        return (long long)j.K * j.Cstore;
    case SEAM_REPACK_NARROW:
        if (!plain || !seam_linear_narrow_supported(j.Cstore, j.K)) return 0;
        return (long long)(j.Cstore >> 4) * 256;
    default:
        return 0;
    }
}

}  // namespace

extern "C" {

long long seam_repack_layout(seam_repack_job_t* jobs, int n_jobs) {
    if (!jobs || n_jobs < 0) return -1;
    long long blocks = 0;
    for (int k = 0; k < n_jobs; ++k) {
        seam_repack_job_t& j = jobs[k];
        const long long items = job_items(j);
        if (items <= 0 || items >= (1LL << 40)) return -1 - k;
        long long nb = (items + 255) / 256;
        if (nb > JOB_BLOCKS) nb = JOB_BLOCKS;
        j.items = items;
        j.first_block = (int)blocks;
        j.n_blocks = (int)nb;
        blocks += nb;
        if (blocks >= (1LL << 30)) return -1 - k;
    }
    return blocks;
}

int seam_repack_many_f32(const seam_repack_job_t* jobs, int n_jobs, long long total_blocks, void* stream) {
    if (n_jobs < 0 || total_blocks < 0 || total_blocks >= (1LL << 30)) return (int)hipErrorInvalidValue;
    if (n_jobs == 0 || total_blocks == 0) return 0;
    if (!jobs) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(repack_many_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream, jobs, n_jobs);
    return (int)hipGetLastError();
}

}  // extern "C"
