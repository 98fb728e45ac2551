// seam_launch.h -- host-side launch helpers of the kernel files.  Nothing here reads the environment, allocates or synchronises.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <stddef.h>

namespace seam_launch {

// Compute units of device `dev`, read once per device (256 when the query fails).  Devices alias modulo 32.
inline int cu_count(int dev) {
    static std::atomic<int> cus[32];
    int ncu = cus[dev & 31].load(std::memory_order_relaxed);
    if (ncu <= 0) {
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu <= 0) ncu = 256;
        cus[dev & 31].store(ncu, std::memory_order_relaxed);
    }
    return ncu;
}

// Once per device and kernel: more than 64 KiB of dynamic LDS needs hipFuncAttributeMaxDynamicSharedMemorySize set before the first
// launch.  The attribute is per function, so every kernel instantiation has its own flag word -- one bit per device, acquire /
// release because the C ABI is thread-safe per stream.  Returns hipFuncSetAttribute's error unchanged (and sets no bit then);
// *ncu, when asked for, is the current device's CU count.
template <auto Kernel>
inline hipError_t prepare(int lds_bytes, int* ncu = nullptr) {
    static std::atomic<unsigned> attr_done{0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned bit = 1u << (dev & 31);
    if (!(attr_done.load(std::memory_order_acquire) & bit)) {
        const hipError_t e = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
        if (e != hipSuccess) return e;
        attr_done.fetch_or(bit, std::memory_order_release);
    }
    if (ncu) *ncu = cu_count(dev);
    return hipSuccess;
}

// grid of a grid-stride kernel with 256-thread blocks over `total` elements, at most `cap` blocks
inline unsigned grid256(size_t total, unsigned cap = 4096) {
    const size_t g = (total + 255) / 256;
    return g > cap ? cap : (unsigned)g;
}

}  // namespace seam_launch
