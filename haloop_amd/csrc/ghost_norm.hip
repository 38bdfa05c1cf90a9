// Per-utterance squared gradient norms from the back-propagated signals, without forming a per-utterance gradient.
//
// A parameter whose gradient for utterance n is dW_n = sum_t a_t b_t^T has ||dW_n||_F^2 = sum_{t,t'} <a_t, a_t'> <b_t, b_t'>: the
// elementwise product of two T x T Gram matrices, summed.  A *term* is one `a` operand [N][T][Ka], up to two `b` operands (their Grams
// add: W_ih and W_hh of an LSTM layer share the gate gradient) and n_bias bias vectors (gradient sum_t a_t: a `b` Gram of all ones):
//
//     sq[term][n] = sum_{t,t' < T} <a_t, a_t'> * (n_bias + sum_j <b^j_t, b^j_t'>)
//
// Launch 1, one workgroup per (term, utterance, pair of 32-frame tiles i <= j): the rows of both tiles are staged through LDS in
// chunks of 128 floats along K (16-byte loads; the K tail and the frame tail are zero-filled here, the caller's buffers are read in
// place through their strides), the four waves take 32 floats of every chunk each and accumulate their share of the 32 x 32 Gram
// tile on the exact-f32 MFMA 32x32x2 -- whatever the library's arithmetic mode: the product of Grams cancels when per-frame outer
// products cancel, which bf16 operands would not survive.  The waves' shares are added in wave order, the products in a fixed order,
// off-diagonal pairs count twice, and the workgroup writes ONE partial.  Launch 2 adds a row's partials in pair order and, when asked,
// writes norm[n] = sqrt(sum over terms).  No atomics, no workgroup reads what another of the same launch wrote: same inputs, same bits.
#include "halo_common.h"
#include "halo_internal.h"

namespace {

constexpr int TT = 32;             // frames per tile (one MFMA 32x32x2 output tile)
constexpr int KC = 128;            // floats of K staged per step
constexpr int LDW = KC + 4;        // LDS row stride in floats: 16-byte aligned rows, ds_read_b128 of 16 rows x one column conflict-free
constexpr int MAX_TERMS = 16;      // terms per launch (kernel-argument table)

struct TermTable {
    halo_ghost_term t[MAX_TERMS];
};

__device__ __forceinline__ f32x4 load_row4(const float *__restrict__ row, int k, int K, bool vec) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!row || k >= K) return v;
    if (vec && k + 4 <= K) return *reinterpret_cast<const f32x4 *>(row + k);
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (k + e < K) v[e] = row[k + e];
    return v;
}

// acc += X_i X_j^T over the operand's K, X_i / X_j = rows [ti0, +32) / [tj0, +32) of utterance n (rows >= T are zero)
__device__ __forceinline__ void gram_accumulate(f32x16 &acc, const halo_ghost_operand &op, int n, int ti0, int tj0, bool diag, int T,
                                                float *lds) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = op.K;
    const float *base = op.ptr + (long)n * op.stride_n;
    // 16-byte loads need every row start on a 16-byte boundary
    const bool vec = ((uintptr_t)op.ptr % 16 == 0) && op.stride_n % 4 == 0 && op.stride_t % 4 == 0;
    const int nq = diag ? 4 : 8;                       // 256 threads x nq float4 = (32 or 64) rows x 128 floats
    const int c4 = (tid & 31) * 4;
    const float *rowp[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int r = (tid >> 5) + 8 * q;              // staged row: 0..31 tile i, 32..63 tile j
        const int t = r < TT ? ti0 + r : tj0 + (r - TT);
        rowp[q] = (q < nq && t < T) ? base + (long)t * op.stride_t : nullptr;
    }
    f32x4 stage[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) stage[q] = load_row4(rowp[q], c4, K, vec);
    const int nchunks = (K + KC - 1) / KC;
    const float *rowA = lds + (lane & 31) * LDW + wave * 32 + (lane >> 5) * 16;
    const float *rowB = diag ? rowA : rowA + TT * LDW;
    for (int c = 0; c < nchunks; ++c) {
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (q < nq) *reinterpret_cast<f32x4 *>(lds + ((tid >> 5) + 8 * q) * LDW + c4) = stage[q];
        __syncthreads();
        if (c + 1 < nchunks) {
#pragma unroll
            for (int q = 0; q < 8; ++q) stage[q] = load_row4(rowp[q], (c + 1) * KC + c4, K, vec);
        }
        if (c * KC + wave * 32 < K) {                  // (wave-uniform: this wave's 32 floats of the chunk hold data)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const f32x4 a4 = *reinterpret_cast<const f32x4 *>(rowA + 4 * v);
                const f32x4 b4 = *reinterpret_cast<const f32x4 *>(rowB + 4 * v);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], b4[e], acc, 0, 0, 0);
            }
        }
        __syncthreads();
    }
}

// the four waves' shares of a Gram tile, added in wave order: thread tid gets elements tid + 256 q of the [16 registers][64 lanes] tile
__device__ __forceinline__ void gram_combine(const f32x16 &acc, float *lds, float (&g)[4]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int r = 0; r < 16; ++r) lds[(wave * 16 + r) * 64 + lane] = acc[r];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = tid + 256 * q;
        g[q] = ((lds[e] + lds[1024 + e]) + lds[2048 + e]) + lds[3072 + e];
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void ghost_gram_kernel(TermTable tab, int term0, int N, int T, int nt, int npairs, float *__restrict__ part) {
    __shared__ __attribute__((aligned(16))) float lds[2 * TT * LDW];
    const halo_ghost_term &tm = tab.t[blockIdx.z];
    const int n = blockIdx.y;
    int ti = 0, rem = blockIdx.x;                      // pair index -> (ti <= tj), row by row of the upper triangle
    while (rem >= nt - ti) { rem -= nt - ti; ++ti; }
    const int tj = ti + rem;
    const bool diag = ti == tj;
    f32x16 accA, accB;
#pragma unroll
    for (int r = 0; r < 16; ++r) { accA[r] = 0.f; accB[r] = 0.f; }
    gram_accumulate(accA, tm.a, n, ti * TT, tj * TT, diag, T, lds);
    if (tm.n_b > 0) gram_accumulate(accB, tm.b[0], n, ti * TT, tj * TT, diag, T, lds);
    if (tm.n_b > 1) gram_accumulate(accB, tm.b[1], n, ti * TT, tj * TT, diag, T, lds);
    float ga[4], gb[4] = {0.f, 0.f, 0.f, 0.f};
    gram_combine(accA, lds, ga);
    if (tm.n_b > 0) gram_combine(accB, lds, gb);
    // rows past T were staged as zeros: their G_a entries are exact zeros, so the bias count adds nothing there
    const float nb = (float)tm.n_bias;
    float v = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) v += ga[q] * (nb + gb[q]);
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = ((lds[0] + lds[1]) + lds[2]) + lds[3];
        if (!diag) s *= 2.f;
        part[((long)(term0 + blockIdx.z) * N + n) * npairs + blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(256) void ghost_reduce_kernel(const float *__restrict__ part, float *__restrict__ sq, float *__restrict__ norm,
                                                           int n_terms, int N, int npairs) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float tot = 0.f;
    for (int term = 0; term < n_terms; ++term) {
        const float *p = part + ((long)term * N + n) * npairs;
        float s = 0.f;
        for (int q = 0; q < npairs; ++q) s += p[q];
        if (sq) sq[(long)term * N + n] = s;
        tot += s;
    }
    if (norm) norm[n] = sqrtf(tot);
}

inline long tile_pairs(int T) {
    const long nt = (T + TT - 1) / TT;
    return nt * (nt + 1) / 2;
}

inline bool operand_ok(const halo_ghost_operand &o) { return o.ptr && o.K >= 1 && o.stride_n >= 0 && o.stride_t >= 0; }

}  // namespace

extern "C" {

int halo_ghost_tile(void) { return TT; }

size_t halo_ghost_sqnorm_workspace_bytes(int n_terms, int N, int T) {
    if (n_terms <= 0 || N <= 0 || T <= 0) return 0;
    return (size_t)n_terms * N * tile_pairs(T) * sizeof(float);
}

int halo_ghost_sqnorm(const halo_ghost_term *terms, int n_terms, int N, int T, float *workspace, float *sq, float *norm,
                      halo_stream_t stream) {
    HALO_CHECK_ARG(terms && workspace && (sq || norm) && n_terms > 0 && N > 0 && T > 0);
    for (int i = 0; i < n_terms; ++i) {
        const halo_ghost_term &tm = terms[i];
        HALO_CHECK_ARG(tm.n_b >= 0 && tm.n_b <= 2 && tm.n_bias >= 0 && tm.n_bias <= 2 && operand_ok(tm.a));
        for (int j = 0; j < tm.n_b; ++j) HALO_CHECK_ARG(operand_ok(tm.b[j]));
    }
    const long npairs = tile_pairs(T);
    if (N > 65535 || npairs > 0x7fffffffL) return HALO_ENOTSUP;         // grid limits
    hipStream_t st = (hipStream_t)stream;
    const int nt = (T + TT - 1) / TT;
    for (int t0 = 0; t0 < n_terms; t0 += MAX_TERMS) {
        const int cnt = n_terms - t0 < MAX_TERMS ? n_terms - t0 : MAX_TERMS;
        TermTable tab = {};
        for (int i = 0; i < cnt; ++i) tab.t[i] = terms[t0 + i];
        hipLaunchKernelGGL(ghost_gram_kernel, dim3((unsigned)npairs, (unsigned)N, (unsigned)cnt), dim3(256), 0, st, tab, t0, N, T, nt, (int)npairs,
                           workspace);
        const int rc = halo_launch_status();
        if (rc) return rc;
    }
    hipLaunchKernelGGL(ghost_reduce_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, workspace, sq, norm, n_terms, N, (int)npairs);
    return halo_launch_status();
}

}  // extern "C"
