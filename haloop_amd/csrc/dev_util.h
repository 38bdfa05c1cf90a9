// Small device-side pieces with no owner: the split-bf16 operand form of the `bf16x3` products, a whole-range buffer descriptor and
// the bound of every spin wait.  Shared by the persistent LSTM launches (lstm_persist_dev.h) and the CTC head family (ctc_head_dev.h).
#pragma once
#include <hip/hip_runtime.h>

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr unsigned long long SPIN_TIMEOUT_TICKS = 20000000ull;   // 0.2 s of the 100 MHz s_memrealtime counter

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void *base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, 0x7fffffff, 0x00020000);
}

// x = hi + lo with hi = bf16(x), lo = bf16(x - hi): a product of two such operands as hi*hi + hi*lo + lo*hi is fp32-grade
__device__ __forceinline__ void split8(const float *x, bf16x8 &hi, bf16x8 &lo) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const __bf16 h = (__bf16)x[e];
        hi[e] = h;
        lo[e] = (__bf16)(x[e] - (float)h);
    }
}

}  // namespace
