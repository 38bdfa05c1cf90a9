// halo_rope_rows: the interleaved rotary embedding (ha/transformer.py:16-31) on the packed q | k | v rows the GPT block forms keep, q and k
// in ONE launch, in place.  Columns [0, 2C) of a row are 2 * heads heads of head_dim; v (and whatever follows it) is never touched.
//
// Memory-bound: 16 bytes per lane and direction (4 fp32 = 2 pairs, 8 bf16 = 4 pairs), consecutive lanes on consecutive 16-byte chunks
// of a row, the cos / sin of a chunk's pairs as one 8- or 16-byte load each from the tables of halo_rope_table (L2-resident: T * head_dim / 2
// floats).  No LDS, a dozen VGPRs: occupancy is set by the block size alone.  head_dim % 8 == 0 keeps a chunk inside one head.
#include "halo_internal.h"

typedef __bf16 rr_bf16x8 __attribute__((ext_vector_type(8)));
typedef float rr_f32x2 __attribute__((ext_vector_type(2)));

// the same expressions as rope_apply_kernel (attn.hip): s carries the sign of the direction
__device__ __forceinline__ void rope_pair(float &x0, float &x1, float c, float s) {
    const float a = x0, b = x1;
    x0 = a * c + (-b) * s;
    x1 = b * c + a * s;
}

// chunk `idx` of the launch -> its row and first column; false past the end
__device__ __forceinline__ bool rope_chunk(long idx, long n_rows, int chunks_per_row, int vec, long &row, int &col) {
    if (idx >= n_rows * chunks_per_row) return false;
    row = idx / chunks_per_row;
    col = (int)(idx % chunks_per_row) * vec;
    return true;
}

__global__ __launch_bounds__(256) void rope_rows_f32_kernel(float *__restrict__ x, long row_stride, long n_rows, int T, int chunks_per_row,
                                                            int head_dim, int t0, const float *__restrict__ cs,
                                                            const float *__restrict__ sn, float sign) {
    long row;
    int col;
    if (!rope_chunk((long)blockIdx.x * 256 + threadIdx.x, n_rows, chunks_per_row, 4, row, col)) return;
    const int half = head_dim / 2;
    const long tab = (long)(t0 + (int)(row % T)) * half + (col % head_dim) / 2;
    const rr_f32x2 c = *reinterpret_cast<const rr_f32x2 *>(cs + tab), s = *reinterpret_cast<const rr_f32x2 *>(sn + tab);
    f32x4 *p = reinterpret_cast<f32x4 *>(x + row * row_stride + col);
    f32x4 v = *p;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        float x0 = v[2 * j], x1 = v[2 * j + 1];
        rope_pair(x0, x1, c[j], sign * s[j]);
        v[2 * j] = x0;
        v[2 * j + 1] = x1;
    }
    *p = v;
}

// bf16 rows: upcast, rotate in fp32, one round-to-nearest-even on the way back
__global__ __launch_bounds__(256) void rope_rows_b16_kernel(__bf16 *__restrict__ x, long row_stride, long n_rows, int T, int chunks_per_row,
                                                            int head_dim, int t0, const float *__restrict__ cs,
                                                            const float *__restrict__ sn, float sign) {
    long row;
    int col;
    if (!rope_chunk((long)blockIdx.x * 256 + threadIdx.x, n_rows, chunks_per_row, 8, row, col)) return;
    const int half = head_dim / 2;
    const long tab = (long)(t0 + (int)(row % T)) * half + (col % head_dim) / 2;
    const f32x4 c = *reinterpret_cast<const f32x4 *>(cs + tab), s = *reinterpret_cast<const f32x4 *>(sn + tab);
    rr_bf16x8 *p = reinterpret_cast<rr_bf16x8 *>(x + row * row_stride + col);
    rr_bf16x8 v = *p;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float x0 = (float)v[2 * j], x1 = (float)v[2 * j + 1];
        rope_pair(x0, x1, c[j], sign * s[j]);
        v[2 * j] = (__bf16)x0;
        v[2 * j + 1] = (__bf16)x1;
    }
    *p = v;
}

int halo_rope_rows(void *x, int is_bf16, long row_stride, long n_rows, int T, int heads, int head_dim, int t0, const float *cos_table,
                   const float *sin_table, int table_rows, int inverse, halo_stream_t stream) {
    HALO_CHECK_ARG(x && cos_table && sin_table && n_rows > 0 && T > 0 && heads > 0 && head_dim > 0 && t0 >= 0);
    HALO_CHECK_ARG(head_dim % 8 == 0 && (long)t0 + T <= table_rows);
    const int vec = is_bf16 ? 8 : 4;                          // elements of a 16-byte chunk
    const long width = 2L * heads * head_dim;                 // the q and k columns
    HALO_CHECK_ARG(row_stride >= width && row_stride % vec == 0 && (uintptr_t)x % 16 == 0);
    HALO_CHECK_ARG((uintptr_t)cos_table % 16 == 0 && (uintptr_t)sin_table % 16 == 0);
    const int chunks_per_row = (int)(width / vec);
    const long blocks = (n_rows * chunks_per_row + 255) / 256;
    HALO_CHECK_ARG(blocks <= 0x7fffffffL);
    const float sign = inverse ? -1.0f : 1.0f;
    if (is_bf16)
        hipLaunchKernelGGL(rope_rows_b16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (__bf16 *)x, row_stride, n_rows, T,
                           chunks_per_row, head_dim, t0, cos_table, sin_table, sign);
    else
        hipLaunchKernelGGL(rope_rows_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (float *)x, row_stride, n_rows, T,
                           chunks_per_row, head_dim, t0, cos_table, sin_table, sign);
    return halo_launch_status();
}
