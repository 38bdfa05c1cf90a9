// The dynamic-LDS opt-in of the large-LDS kernels.  Needs nothing else of libhalo: the lab tools include it through gemm256.h / gemm_rows.h.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include "halo.h"

// A launch that asks for more than 64 KiB of dynamic LDS fails unless the kernel's MaxDynamicSharedMemorySize attribute allowed it that
// much before.  The attribute is per DEVICE, so a process-wide "done" flag leaves every device but the first without it.  One table per
// kernel (the static below exists once per instantiation), indexed by the HIP device ordinal: the bytes already granted there.  Relaxed
// atomics: racing host threads ask for the same kernel's size and write the same value.  A device ordinal past the table is not
// remembered: the attribute is then set on every call.  Returns HALO_OK / HALO_ELAUNCH.
template <auto Kernel>
int halo_allow_dyn_lds(int bytes) {
    constexpr int MAX_DEVICES = 64;
    static std::atomic<int> granted[MAX_DEVICES];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return HALO_ELAUNCH;
    std::atomic<int> *g = dev >= 0 && dev < MAX_DEVICES ? &granted[dev] : nullptr;
    if (g && bytes <= g->load(std::memory_order_relaxed)) return HALO_OK;
    if (hipFuncSetAttribute((const void *)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return HALO_ELAUNCH;
    if (g) g->store(bytes, std::memory_order_relaxed);
    return HALO_OK;
}

// ... and the launch it serves, so that a (kernel, bytes) pair is written once.  Returns the opt-in's status: the launch's own is read by
// the caller as after any other launch (halo_launch_status).
template <auto Kernel, typename... Args>
int halo_launch_lds(dim3 grid, dim3 block, int bytes, hipStream_t st, const Args &...args) {
    const int rc = halo_allow_dyn_lds<Kernel>(bytes);
    if (rc == HALO_OK) hipLaunchKernelGGL(Kernel, grid, block, (size_t)bytes, st, args...);
    return rc;
}
