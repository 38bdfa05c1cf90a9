// Device helpers shared by the decode-step attention launches (decode.hip, decode_beam.hip).
#pragma once
#include <hip/hip_fp16.h>

// DPL consecutive float16 values (2, 4, 8 or 16: one lane's chunk of a cached key or value) as floats, by one or two vector loads
template <int DPL>
__device__ __forceinline__ void load_halfs(const __half *src, float *out) {
    if constexpr (DPL == 2) {
        const __half2 v = *reinterpret_cast<const __half2 *>(src);
        out[0] = __low2float(v); out[1] = __high2float(v);
    } else {
        typedef unsigned uvec __attribute__((ext_vector_type(DPL == 4 ? 2 : 4)));
#pragma unroll
        for (int part = 0; part < (DPL == 16 ? 2 : 1); ++part) {
            const uvec raw = *reinterpret_cast<const uvec *>(src + part * 8);
#pragma unroll
            for (int w = 0; w < (DPL == 4 ? 2 : 4); ++w) {
                const unsigned u = raw[w];
                const __half2 v = *reinterpret_cast<const __half2 *>(&u);
                out[part * 8 + 2 * w] = __low2float(v);
                out[part * 8 + 2 * w + 1] = __high2float(v);
            }
        }
    }
}
