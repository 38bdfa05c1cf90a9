// LoRA adapters of the GPT c_attn Linear on row-major bf16 rows (haloop_amd/lora.py; ha/lora.py:84-91 and its autograd backward).
//
// With h = ln_1(x) [M][C] as bf16 rows, A [r][C], B [3C][r], s = lora_alpha / r, m the dropout mask of the adapter's input:
//     forward   u = (m*h) A^T [M][r]            qkv += s u B^T
//     backward  du = s dqkv B [M][r]            dB = s dqkv^T u         dA = du^T (m*h)         d_ln1 += m * (du A)
// Three kernels, all with the rank padded to 16 (zero rows / columns) so that one v_mfma_f32_16x16x32_bf16 spans it, fp32 accumulation:
//     lora_down  U [M][16] = scale * (m*X [M][K]) P [16][K]^T     one pass over X; the four waves of a workgroup cut K between them
//     lora_up    Y [M][N] += scale * mask * U [M][16] P [N][16]^T  read-modify-write of bf16 or fp32 rows; the contraction is the rank
//     lora_tn    G [16][K] = scale * U [M][16]^T (m*X [M][K])      M cut into slabs (one workgroup each, four waves meeting in LDS), partial
//                tiles to a workspace, fixed-order reduce
// The mask is never a tensor: every kernel recomputes it with dropout_mult4 on the flat index row * width + col of the [M][width] rows,
// which is what halo_dropout_fwd draws.  Only its 0 / 1 part touches the bf16 operands; the 1 / (1 - p) factor goes into the fp32 scale.
#include "halo_common.h"
#include "halo_internal.h"

namespace {
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
constexpr int RP = 16;                 // the padded rank
constexpr int TN_SLAB_ROWS = 256;      // rows of M per partial tile of lora_tn
constexpr int UP_SPAN = 256;           // columns of Y per workgroup of lora_up

__device__ __forceinline__ bf16x8 zero8() {
    bf16x8 z;
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = (__bf16)0.0f;
    return z;
}

// A [r][n_in], B [n_out][r] fp32 -> A16 [16][n_in] | At16 [n_in][16] | B16 [n_out][16] | Bt16 [16][n_out], bf16, rank padded with zeros
__global__ __launch_bounds__(256) void lora_pack_kernel(const float *__restrict__ A, const float *__restrict__ B, int r, int n_in, int n_out,
                                                        __bf16 *__restrict__ out) {
    const long idx = blockIdx.x * 256L + threadIdx.x, na = (long)RP * n_in, nb = (long)RP * n_out;
    if (idx >= 2 * (na + nb)) return;
    float v = 0.f;
    if (idx < na) {                                     // A16[i][c]
        const int i = idx / n_in, c = idx % n_in;
        if (i < r) v = A[(long)i * n_in + c];
    } else if (idx < 2 * na) {                          // At16[c][i]
        const long e = idx - na;
        const int c = e / RP, i = e % RP;
        if (i < r) v = A[(long)i * n_in + c];
    } else if (idx < 2 * na + nb) {                     // B16[n][i]
        const long e = idx - 2 * na;
        const int n = e / RP, i = e % RP;
        if (i < r) v = B[(long)n * r + i];
    } else {                                            // Bt16[i][n]
        const long e = idx - 2 * na - nb;
        const int i = e / n_out, n = e % n_out;
        if (i < r) v = B[(long)n * r + i];
    }
    out[idx] = (__bf16)v;
}

// One workgroup per 16 rows of X; wave w takes the 32-deep k-blocks w, w + 4, ...; the four partial 16 x 16 tiles meet in LDS.
// MFMA operands (cdna 16x16x32 maps): A[row i][k = 8g + j] = X[row0 + i][k0 + 8g + j], B[k][col n] = P[n][k0 + 8g + j], D[row 4g + reg][col n].
__global__ __launch_bounds__(256) void lora_down_kernel(const __bf16 *__restrict__ X, long ldx, const __bf16 *__restrict__ P, int K, float scale,
                                                        __bf16 *__restrict__ U, const DropoutCfg d, int use_drop) {
    __shared__ float red[4][256];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
    const long row = blockIdx.x * 16L + i;
    const __bf16 *xr = X + row * ldx + 8 * g, *pr = P + (long)i * K + 8 * g;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = wave * 32; k0 < K; k0 += 128) {
        bf16x8 a = *reinterpret_cast<const bf16x8 *>(xr + k0);
        const bf16x8 b = *reinterpret_cast<const bf16x8 *>(pr + k0);
        if (use_drop) {
            const uint64_t e = (uint64_t)row * K + k0 + 8 * g;
            const f32x4 m0 = dropout_mult4(d, e), m1 = dropout_mult4(d, e + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (m0[j] == 0.f) a[j] = (__bf16)0.0f;
                if (m1[j] == 0.f) a[4 + j] = (__bf16)0.0f;
            }
        }
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) red[wave][(4 * g + reg) * 16 + i] = acc[reg];
    __syncthreads();
    const int t = threadIdx.x;
    const float v = ((red[0][t] + red[1][t]) + (red[2][t] + red[3][t])) * scale;
    U[blockIdx.x * 256L + t] = (__bf16)v;
}

// One wave per 16 rows of Y and UP_SPAN columns, 32 columns per step as two MFMAs of the TRANSPOSED product (P tile) x U^T, so that a lane
// ends with 8 consecutive columns of one row: A-row ii of MFMA t is column nb + 8 (ii >> 2) + 4 t + (ii & 3), the result D[row 4g + reg][col i]
// is Y[m0 + i][nb + 8g + 4t + reg].  The upper half of the 32-deep contraction is zero (the rank is at most 16).
template <bool F32>
__global__ __launch_bounds__(256) void lora_up_kernel(const __bf16 *__restrict__ U, const __bf16 *__restrict__ P, int M, int N, float scale,
                                                      void *__restrict__ Yv, long ldy, const DropoutCfg d, int use_drop) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
    const long m0 = (blockIdx.x * 4L + wave) * 16;
    if (m0 >= M) return;
    const long row = m0 + i;
    const bf16x8 ub = g < 2 ? *reinterpret_cast<const bf16x8 *>(U + row * RP + 8 * g) : zero8();
    const int n_begin = blockIdx.y * UP_SPAN, n_end = n_begin + UP_SPAN < N ? n_begin + UP_SPAN : N;
    for (int nb = n_begin; nb < n_end; nb += 32) {
        f32x4 acc[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const long n = nb + 8 * (i >> 2) + 4 * t + (i & 3);
            const bf16x8 pa = g < 2 ? *reinterpret_cast<const bf16x8 *>(P + n * RP + 8 * g) : zero8();
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, ub, z, 0, 0, 0);
        }
        const int col = nb + 8 * g;
        float upd[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) upd[j] = acc[j >> 2][j & 3] * scale;
        if (use_drop) {
            const uint64_t e = (uint64_t)row * N + col;
            const f32x4 k0 = dropout_mult4(d, e), k1 = dropout_mult4(d, e + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) { upd[j] *= k0[j]; upd[4 + j] *= k1[j]; }
        }
        if (F32) {
            f32x4 *y = reinterpret_cast<f32x4 *>(static_cast<float *>(Yv) + row * ldy + col);
            f32x4 y0 = y[0], y1 = y[1];
#pragma unroll
            for (int j = 0; j < 4; ++j) { y0[j] += upd[j]; y1[j] += upd[4 + j]; }
            y[0] = y0; y[1] = y1;
        } else {
            bf16x8 *y = reinterpret_cast<bf16x8 *>(static_cast<__bf16 *>(Yv) + row * ldy + col);
            bf16x8 v = *y;
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (__bf16)((float)v[j] + upd[j]);
            *y = v;
        }
    }
}

// One workgroup per (64 columns of X, slab of TN_SLAB_ROWS rows), its four waves taking every fourth 32-row step and meeting in LDS:
// D[row ii][col c] += sum over 32 rows m of U[m][ii] X[m][c], operands A[row ii = i][k = 8g + jj] = U[m0 + 8g + jj][i],
// B[k][col i] = X[m0 + 8g + jj][c0 + 16 t + i]; both are gathers of 2-byte elements down a column, 32 contiguous bytes per 16 lanes, the
// four column tiles of a wave using up each 128-byte line in the same step.  Only the r real rows of the tile reach the workspace.
// The mask: the four lanes of a quad share one Philox block per row; lane b of the quad draws rows jj = b and b + 4 and the quad
// exchanges the keep bits.
__global__ __launch_bounds__(256) void lora_tn_kernel(const __bf16 *__restrict__ U, const __bf16 *__restrict__ X, long ldx, int M, int K, int r,
                                                      float *__restrict__ ws, const DropoutCfg d, int use_drop) {
    __shared__ float red[4][4][256];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
    const int nchunks = (K + 63) / 64;
    const int c = blockIdx.x % nchunks;
    const long s = blockIdx.x / nchunks;
    const int c0 = c * 64, nt = (K - c0) / 16 < 4 ? (K - c0) / 16 : 4;
    const long m_end = (s + 1) * TN_SLAB_ROWS < M ? (s + 1) * TN_SLAB_ROWS : M;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (long m0 = s * TN_SLAB_ROWS + wave * 32; m0 < m_end; m0 += 128) {
        const long r0 = m0 + 8 * g;
        bf16x8 a;
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) a[jj] = U[(r0 + jj) * RP + i];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (t < nt) {
                const int col = c0 + 16 * t + i;
                bf16x8 b;
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) b[jj] = X[(r0 + jj) * ldx + col];
                if (use_drop) {
                    const int q = i & 3;
                    const uint64_t e = (uint64_t)(r0 + q) * K + (col & ~3);
                    const f32x4 k0 = dropout_mult4(d, e), k1 = dropout_mult4(d, e + 4 * (uint64_t)K);
                    int bits = 0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) bits |= (k0[j] != 0.f ? 1 << j : 0) | (k1[j] != 0.f ? 16 << j : 0);
#pragma unroll
                    for (int b4 = 0; b4 < 4; ++b4) {
                        const int v = __shfl(bits, (lane & ~3) | b4);
                        if (!((v >> q) & 1)) b[b4] = (__bf16)0.0f;
                        if (!((v >> (4 + q)) & 1)) b[4 + b4] = (__bf16)0.0f;
                    }
                }
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[t], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) red[wave][t][(4 * g + reg) * 16 + i] = acc[t][reg];
    __syncthreads();
    const int row = threadIdx.x >> 4, col = threadIdx.x & 15;
    if (row < r)
        for (int t = 0; t < nt; ++t)
            ws[(s * RP + row) * K + c0 + 16 * t + col] =
                (red[0][t][threadIdx.x] + red[1][t][threadIdx.x]) + (red[2][t][threadIdx.x] + red[3][t][threadIdx.x]);
}

// G[i][c] (or G[c][i]) = scale * sum over the slabs in their order: two runs give the same bits
__global__ __launch_bounds__(256) void lora_tn_reduce_kernel(const float *__restrict__ ws, int nslabs, int K, int r, float scale, int transpose,
                                                             float *__restrict__ G) {
    const long idx = blockIdx.x * 256L + threadIdx.x;
    if (idx >= (long)r * K) return;
    const int i = idx / K, c = idx % K;
    float sum = 0.f;
#pragma unroll 8
    for (int s = 0; s < nslabs; ++s) sum += ws[((long)s * RP + i) * K + c];
    G[transpose ? (long)c * r + i : idx] = sum * scale;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
}  // namespace

extern "C" {

int halo_lora_supported(int M, int n_in, int n_out, int r) {
    return M > 0 && M % 32 == 0 && n_in > 0 && n_in % 32 == 0 && n_out > 0 && n_out % 32 == 0 && r > 0 && r <= RP;
}

size_t halo_lora_pack_bytes(int n_in, int n_out) {
    return n_in > 0 && n_out > 0 ? (size_t)2 * RP * ((size_t)n_in + n_out) * 2 : 0;
}

int halo_lora_pack(const float *A, const float *B, int r, int n_in, int n_out, void *packed, halo_stream_t stream) {
    HALO_CHECK_ARG(A && B && packed && r > 0 && r <= RP && n_in > 0 && n_out > 0 && n_in % 8 == 0 && n_out % 8 == 0 && aligned16(packed));
    const long n = 2L * RP * ((long)n_in + n_out);
    hipLaunchKernelGGL(lora_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, A, B, r, n_in, n_out,
                       static_cast<__bf16 *>(packed));
    return halo_launch_status();
}

int halo_lora_down(const void *x_bf16, long ldx, const void *p16, int M, int K, float scale, void *u_bf16, float p_drop, uint64_t seed,
                   uint32_t stream_id, uint32_t offset, const uint32_t *offset_dev, halo_stream_t stream) {
    HALO_CHECK_ARG(x_bf16 && p16 && u_bf16 && M > 0 && M % 16 == 0 && K > 0 && K % 32 == 0 && ldx >= K && ldx % 8 == 0);
    HALO_CHECK_ARG(aligned16(x_bf16) && aligned16(p16) && aligned16(u_bf16) && p_drop >= 0.f && p_drop < 1.f);
    const DropoutCfg d = make_dropout(p_drop, seed, stream_id, offset, offset_dev);
    hipLaunchKernelGGL(lora_down_kernel, dim3(M / 16), dim3(256), 0, (hipStream_t)stream, static_cast<const __bf16 *>(x_bf16), ldx,
                       static_cast<const __bf16 *>(p16), K, scale * d.scale, static_cast<__bf16 *>(u_bf16), d, p_drop > 0.f ? 1 : 0);
    return halo_launch_status();
}

int halo_lora_up(const void *u_bf16, const void *p16, int M, int N, float scale, void *y_bf16, float *y_f32, long ldy, float p_drop,
                 uint64_t seed, uint32_t stream_id, uint32_t offset, const uint32_t *offset_dev, halo_stream_t stream) {
    HALO_CHECK_ARG(u_bf16 && p16 && ((y_bf16 != nullptr) != (y_f32 != nullptr)) && M > 0 && M % 16 == 0 && N > 0 && N % 32 == 0 && ldy >= N);
    HALO_CHECK_ARG(aligned16(u_bf16) && aligned16(p16) && aligned16(y_bf16) && aligned16(y_f32) && ldy % 8 == 0 && p_drop >= 0.f && p_drop < 1.f);
    const DropoutCfg d = make_dropout(p_drop, seed, stream_id, offset, offset_dev);
    const dim3 grid((M / 16 + 3) / 4, (N + UP_SPAN - 1) / UP_SPAN);
    const int use_drop = p_drop > 0.f ? 1 : 0;
    if (y_f32)
        hipLaunchKernelGGL(lora_up_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, static_cast<const __bf16 *>(u_bf16),
                           static_cast<const __bf16 *>(p16), M, N, scale, (void *)y_f32, ldy, d, use_drop);
    else
        hipLaunchKernelGGL(lora_up_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, static_cast<const __bf16 *>(u_bf16),
                           static_cast<const __bf16 *>(p16), M, N, scale, y_bf16, ldy, d, use_drop);
    return halo_launch_status();
}

size_t halo_lora_tn_workspace_bytes(int M, int K) {
    return M > 0 && K > 0 ? (size_t)((M + TN_SLAB_ROWS - 1) / TN_SLAB_ROWS) * RP * (size_t)K * sizeof(float) : 0;
}

int halo_lora_tn(const void *u_bf16, const void *x_bf16, long ldx, int M, int K, int r, float scale, int transpose_out, float *g,
                 void *workspace, float p_drop, uint64_t seed, uint32_t stream_id, uint32_t offset, const uint32_t *offset_dev,
                 halo_stream_t stream) {
    HALO_CHECK_ARG(u_bf16 && x_bf16 && g && workspace && M > 0 && M % 32 == 0 && K > 0 && K % 16 == 0 && ldx >= K && r > 0 && r <= RP);
    HALO_CHECK_ARG(p_drop >= 0.f && p_drop < 1.f);
    const DropoutCfg d = make_dropout(p_drop, seed, stream_id, offset, offset_dev);
    const int nslabs = (M + TN_SLAB_ROWS - 1) / TN_SLAB_ROWS, nchunks = (K + 63) / 64;
    hipLaunchKernelGGL(lora_tn_kernel, dim3((unsigned)(nslabs * nchunks)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const __bf16 *>(u_bf16), static_cast<const __bf16 *>(x_bf16), ldx, M, K, r, static_cast<float *>(workspace), d,
                       p_drop > 0.f ? 1 : 0);
    hipLaunchKernelGGL(lora_tn_reduce_kernel, dim3((unsigned)(((long)r * K + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const float *>(workspace), nslabs, K, r, scale * d.scale, transpose_out ? 1 : 0, g);
    return halo_launch_status();
}

}  // extern "C"
