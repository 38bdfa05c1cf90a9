// The masked objectives of the GPT trainer (ha/attention_loop.py:110-120): BERT-style token masking on the device, and the row
// compaction that lets ln_f, the lm_head and the cross-entropy run on the rows that carry a target only.
//   mask_tokens_kernel / mlm_batch_u16_kernel   mask_tokens                                       ha/mlm.py:11-40, attention_loop.py:113-114
//   target_rows_kernel                           the rows F.cross_entropy(ignore_index=0) keeps    ha/attention.py:230-231
//   gather_rows_kernel / scatter_rows_kernel     rows [M, C] <-> compact rows [K, C]
// Integer work and copies: every kernel is bit-exact and deterministic (no atomics; placement by ballot / popcount scans).
#include <math.h>

#include "halo_common.h"

namespace {

struct MlmCfg {
    uint32_t k0, k1, step;
    uint32_t thr_select, thr_replace, thr_random;
    int64_t mask_token, endoftext_token;
    uint64_t max_token;
};

// the threshold of include/halo.h: min(int(float32(p) * 2^32), 0xFFFFFFFF)
uint32_t mlm_threshold(float p) {
    const double t = (double)p * 4294967296.0;
    return t >= 4294967295.0 ? 0xffffffffu : (uint32_t)t;
}

// (input, label) of flat position e holding ``token``: one Philox call, four draws
__device__ __forceinline__ void mlm_draw(const MlmCfg &c, uint64_t e, int64_t token, int64_t &input, int64_t &label) {
    const Philox4 r = philox4x32_10((uint32_t)e, (uint32_t)(e >> 32), HALO_MLM_STREAM, c.step, c.k0, c.k1);
    const bool selected = token != c.endoftext_token && r.v[0] < c.thr_select;
    const bool replaced = selected && r.v[1] < c.thr_replace;
    const bool random = selected && !replaced && r.v[2] < c.thr_random;
    label = selected ? token : 0;
    input = replaced ? c.mask_token : random ? (int64_t)(((uint64_t)r.v[3] * c.max_token) >> 32) : token;
}

__global__ __launch_bounds__(256) void mask_tokens_kernel(int64_t *__restrict__ inputs, int64_t *__restrict__ labels, long n, MlmCfg c) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    int64_t in, lb;
    mlm_draw(c, (uint64_t)e, inputs[e], in, lb);
    inputs[e] = in;
    labels[e] = lb;
}

// x[b, t] = mask(data[ix[b] + t]) (0 past the tape, which takes part in the draw like any token), y = the labels
__global__ __launch_bounds__(256) void mlm_batch_u16_kernel(const uint16_t *__restrict__ data, long n_tokens, const int64_t *__restrict__ ix,
                                                            long n, int T, MlmCfg c, int64_t *__restrict__ x, int64_t *__restrict__ y) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const long s = ix[e / T] + e % T;
    const int64_t token = (s >= 0 && s < n_tokens) ? (int64_t)data[s] : 0;
    int64_t in, lb;
    mlm_draw(c, (uint64_t)e, token, in, lb);
    x[e] = in;
    y[e] = lb;
}

// One workgroup of 1024 walks the M targets in tiles of 1024 rows in ascending order: a row's place among the kept rows is the running
// count + the kept rows of the lower waves of its tile (LDS) + the kept lanes below it in its wave (ballot, popcount).  The first
// ``limit`` kept rows get a place; rows / targets_c hold ``cap`` >= limit entries, padded behind the placed ones.
__global__ __launch_bounds__(1024) void target_rows_kernel(const int64_t *__restrict__ targets, int M, int64_t ignore_index, int cap, int limit,
                                                           int *__restrict__ rows, int64_t *__restrict__ targets_c, int *__restrict__ slot,
                                                           int *__restrict__ count) {
    __shared__ int wave_n[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = 0;
    for (int r0 = 0; r0 < M; r0 += 1024) {
        const int i = r0 + threadIdx.x;
        const int64_t tg = i < M ? targets[i] : ignore_index;
        const bool keep = tg != ignore_index;
        const unsigned long long votes = __ballot(keep);
        if (lane == 0) wave_n[wave] = __popcll(votes);
        __syncthreads();
        int below = 0, tile_n = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const int c = wave_n[w];
            below += w < wave ? c : 0;
            tile_n += c;
        }
        __syncthreads();
        const int pos = base + below + __popcll(votes & ((1ull << lane) - 1ull));
        if (i < M) {
            const bool placed = keep && pos < limit;
            slot[i] = placed ? pos : -1;
            if (placed) {
                rows[pos] = i;
                targets_c[pos] = tg;
            }
        }
        base += tile_n;
    }
    for (int k = min(base, limit) + threadIdx.x; k < cap; k += 1024) {
        rows[k] = -1;
        targets_c[k] = ignore_index;
    }
    if (threadIdx.x == 0) *count = base;
}

// dst[k, :] = src[rows[k], :], a zero row where rows[k] is not a row of src.  VEC: 16-byte accesses along C (C % 4 == 0).
template <bool VEC>
__global__ __launch_bounds__(256) void gather_rows_kernel(const float *__restrict__ src, const int *__restrict__ rows, int M, long K, int C,
                                                          float *__restrict__ dst) {
    const int per_row = VEC ? C / 4 : C;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= K * per_row) return;
    const long k = idx / per_row;
    const int q = (int)(idx % per_row);
    const int r = rows[k];
    const bool ok = r >= 0 && r < M;
    if (VEC) {
        const f32x4 v = ok ? *reinterpret_cast<const f32x4 *>(src + (long)r * C + 4 * q) : f32x4{0.f, 0.f, 0.f, 0.f};
        *reinterpret_cast<f32x4 *>(dst + k * C + 4 * q) = v;
    } else {
        dst[k * C + q] = ok ? src[(long)r * C + q] : 0.f;
    }
}

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

// dst[i, :] = src[slot[i], :], a zero row where slot[i] is not a row of src; every one of the M rows is written.  With ``count``:
// NaN in every element when *count > limit (more targets than the caller allowed for).  dst_b16: the same rows as row-major bf16.
template <bool VEC>
__global__ __launch_bounds__(256) void scatter_rows_kernel(const float *__restrict__ src, const int *__restrict__ slot, const int *__restrict__ count,
                                                           int cap, int limit, long M, int C, float *__restrict__ dst, __bf16 *__restrict__ dst_b16) {
    const int per_row = VEC ? C / 4 : C;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= M * per_row) return;
    const long i = idx / per_row;
    const int q = (int)(idx % per_row);
    const int s = slot[i];
    const bool ok = s >= 0 && s < cap;
    const bool overflow = count && *count > limit;
    if (VEC) {
        f32x4 v = ok ? *reinterpret_cast<const f32x4 *>(src + (long)s * C + 4 * q) : f32x4{0.f, 0.f, 0.f, 0.f};
        if (overflow) v = f32x4{NAN, NAN, NAN, NAN};
        *reinterpret_cast<f32x4 *>(dst + i * C + 4 * q) = v;
        if (dst_b16) *reinterpret_cast<bf16x4 *>(dst_b16 + i * C + 4 * q) = bf16x4{(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
    } else {
        float v = ok ? src[(long)s * C + q] : 0.f;
        if (overflow) v = NAN;
        dst[i * C + q] = v;
        if (dst_b16) dst_b16[i * C + q] = (__bf16)v;
    }
}

int mlm_cfg(float p, long mask_token, long endoftext_token, long max_token, uint64_t seed, uint32_t step, MlmCfg &c) {
    HALO_CHECK_ARG(p >= 0.f && p <= 1.f && mask_token >= 0 && max_token > 0 && max_token <= (1L << 32));
    c.k0 = (uint32_t)(seed & 0xffffffffu);
    c.k1 = (uint32_t)(seed >> 32);
    c.step = step;
    c.thr_select = mlm_threshold(p);
    c.thr_replace = mlm_threshold(0.8f);
    c.thr_random = mlm_threshold(0.5f);
    c.mask_token = mask_token;
    c.endoftext_token = endoftext_token;
    c.max_token = (uint64_t)max_token;
    return HALO_OK;
}

bool vec_ok(int C, const void *a, const void *b, const void *c) {
    return C % 4 == 0 && ((uintptr_t)a | (uintptr_t)b) % 16 == 0 && (uintptr_t)c % 8 == 0;
}

}  // namespace

extern "C" {

int halo_mask_tokens(int64_t *inputs, int64_t *labels, long n, float mlm_probability, long mask_token, long endoftext_token, long max_token,
                     uint64_t seed, uint32_t step, halo_stream_t stream) {
    HALO_CHECK_ARG(inputs && labels && n > 0);
    MlmCfg c;
    if (int rc = mlm_cfg(mlm_probability, mask_token, endoftext_token, max_token, seed, step, c)) return rc;
    hipLaunchKernelGGL(mask_tokens_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, inputs, labels, n, c);
    return halo_launch_status();
}

int halo_mlm_batch_u16(const uint16_t *data, long n_tokens, const int64_t *offsets, int B, int T, float mlm_probability, long mask_token,
                       long endoftext_token, long max_token, uint64_t seed, uint32_t step, int64_t *x, int64_t *y, halo_stream_t stream) {
    HALO_CHECK_ARG(data && offsets && x && y && n_tokens > 0 && B > 0 && T > 0);
    MlmCfg c;
    if (int rc = mlm_cfg(mlm_probability, mask_token, endoftext_token, max_token, seed, step, c)) return rc;
    const long n = (long)B * T;
    hipLaunchKernelGGL(mlm_batch_u16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, data, n_tokens, offsets, n, T,
                       c, x, y);
    return halo_launch_status();
}

int halo_target_rows(const int64_t *targets, int M, long ignore_index, int capacity, int limit, int *rows, int64_t *targets_c, int *slot,
                     int *count, halo_stream_t stream) {
    HALO_CHECK_ARG(targets && rows && targets_c && slot && count && M > 0 && limit > 0 && limit <= capacity);
    hipLaunchKernelGGL(target_rows_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, targets, M, (int64_t)ignore_index, capacity, limit,
                       rows, targets_c, slot, count);
    return halo_launch_status();
}

int halo_gather_rows(const float *src, const int *rows, int M, int K, int C, float *dst, halo_stream_t stream) {
    HALO_CHECK_ARG(src && rows && dst && M > 0 && K > 0 && C > 0);
    hipStream_t st = (hipStream_t)stream;
    if (vec_ok(C, src, dst, nullptr)) {
        const long n = (long)K * (C / 4);
        hipLaunchKernelGGL(gather_rows_kernel<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, rows, M, (long)K, C, dst);
    } else {
        const long n = (long)K * C;
        hipLaunchKernelGGL(gather_rows_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, rows, M, (long)K, C, dst);
    }
    return halo_launch_status();
}

int halo_scatter_rows(const float *src, const int *slot, const int *count, int capacity, int limit, int M, int C, float *dst, void *dst_bf16,
                      halo_stream_t stream) {
    HALO_CHECK_ARG(src && slot && dst && M > 0 && limit > 0 && limit <= capacity && C > 0);
    hipStream_t st = (hipStream_t)stream;
    if (vec_ok(C, src, dst, dst_bf16)) {
        const long n = (long)M * (C / 4);
        hipLaunchKernelGGL(scatter_rows_kernel<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, slot, count, capacity, limit, (long)M,
                           C,
                           dst, (__bf16 *)dst_bf16);
    } else {
        const long n = (long)M * C;
        hipLaunchKernelGGL(scatter_rows_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, slot, count, capacity, limit, (long)M,
                           C,
                           dst, (__bf16 *)dst_bf16);
    }
    return halo_launch_status();
}

}  // extern "C"
