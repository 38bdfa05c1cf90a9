// The small-M product of the fused decode launches, shared by csrc/decode.hip (the ASR greedy decode) and csrc/gpt_decode.hip (the GPT
// sampler): the kernel body is stated once here and each translation unit instantiates the variants it launches.
#pragma once
#include <type_traits>
#include "halo_common.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ void split8(const float *x, bf16x8 &hi, bf16x8 &lo) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const __bf16 h = (__bf16)x[e];
        hi[e] = h;
        lo[e] = (__bf16)(x[e] - (float)h);
    }
}

struct DecLinearArgs {
    const float *x;        // [rows][K] fp32, leading dimension ldx
    long ldx;
    int rows, K;
    const float *lnw;      // LayerNorm weight [K] (LN variants)
    float eps;
    const char *w;         // decode image of W [n_out][K]
    int n_tiles, n_out;
    float *out;            // [rows][n_out], leading dimension ldo
    long ldo;
    int flags;             // HALO_GEMM_ACCUM: out += ...; HALO_GEMM_GELU_ERF / HALO_GEMM_GELU: the variant's GELU (ACT)
    // The residual stream as a PAIR (main, side): x = main + side.  LN variants: x2 != NULL is the side (same strides as x), added to the rows
    // before the statistics.  Accumulating products with side_out != NULL run as TWO K-slices (grid.z): slice 0 writes
    // out = (out + side_in) + its half of the product, slice 1 its half alone to side_out -- twice the workgroups, each streaming half of K,
    // every sum in a fixed order; the next launch reads out + side_out.
    const float *x2, *side_in;
    float *side_out;
};

// grid (feature groups of 16*NT, row groups of 16); KSW_LN > 0: F.layer_norm (no bias) of the rows first, K == 128 * KSW_LN.
// PASSES: 3 = the split product (hi and lo fragments of both operands, three MFMAs), 1 = activations rounded to bf16 against the hi
// fragment alone (the lo half of the image is never read).  ACT: which activation bit of `flags` this variant honours (8: exact GELU,
// the ASR decoder's; 2: tanh-GELU, the GPT block's).  No LayerNorm: K / 128 (/ 2 with two K-slices) k-steps per wave, walked 8 at a time
// while that divides them, else 4 and a last 2 -- any even count.
// ARGS: DecLinearArgs, or a record derived from it that finishes the summed tiles itself (csrc/rnnt_decode.hip: the LSTM cell behind the
// gate product) through ``template <int NT> void finish(float (*red)[NT][64][4], int nt0) const`` in place of the store below.
template <int NT, int KSW_LN, int PASSES = 3, int ACT = 8, class ARGS = DecLinearArgs>
__global__ __launch_bounds__(256) void dec_linear_kernel(const ARGS p) {
    __shared__ float red[4][NT][64][4];
    __shared__ float stat[4][16];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int row = blockIdx.y * 16 + r;
    const bool rok = row < p.rows;
    const int nt0 = blockIdx.x * NT;
    const int nsl = (KSW_LN == 0 && p.side_out) ? 2 : 1, kslice = nsl == 2 ? (int)blockIdx.z : 0;
    const int KS = p.K / 32, ksw = KS / nsl / 4, ks0 = kslice * (KS / nsl) + wave * ksw;
    const float *xr = p.x + (long)(rok ? row : 0) * p.ldx + g * 8;
    f32x4 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    // a feature tile past the last one (odd tile count, NT = 2) re-reads the last tile; its sums are never stored
    const char *wbase[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) wbase[nt] = p.w + (long)min(nt0 + nt, p.n_tiles - 1) * KS * 2048 + lane * 16;
    auto product = [&](const float *xv, const bf16x8 (&wh)[NT], const bf16x8 (&wl)[NT]) {
        bf16x8 ah, al;
        split8(xv, ah, al);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            if constexpr (PASSES == 3) {
                acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, wh[nt], acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, wl[nt], acc[nt], 0, 0, 0);
            }
            acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, wh[nt], acc[nt], 0, 0, 0);
        }
    };
    if constexpr (KSW_LN > 0) {
        constexpr int NK = KSW_LN;
        float xv[NK][8];
        bf16x8 wh[NK][NT], wl[NK][NT];
#pragma unroll
        for (int i = 0; i < NK; ++i) {
            f32x4 a = *reinterpret_cast<const f32x4 *>(xr + (ks0 + i) * 32), b = *reinterpret_cast<const f32x4 *>(xr + (ks0 + i) * 32 + 4);
            if (p.x2) {                                      // x = main + side (uniform branch)
                const float *x2r = p.x2 + (xr - p.x);
                a += *reinterpret_cast<const f32x4 *>(x2r + (ks0 + i) * 32);
                b += *reinterpret_cast<const f32x4 *>(x2r + (ks0 + i) * 32 + 4);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) { xv[i][j] = rok ? a[j] : 0.f; xv[i][4 + j] = rok ? b[j] : 0.f; }
        }
#pragma unroll
        for (int i = 0; i < NK; ++i)                     // the weight fragments are in flight under the LayerNorm statistics
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                wh[i][nt] = *reinterpret_cast<const bf16x8 *>(wbase[nt] + (long)(ks0 + i) * 2048);
                if constexpr (PASSES == 3) wl[i][nt] = *reinterpret_cast<const bf16x8 *>(wbase[nt] + (long)(ks0 + i) * 2048 + 1024);
            }
        // biased variance around the mean, eps inside the square root (F.layer_norm); the row is spread over 4 lanes x 4 waves
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NK; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) s += xv[i][j];
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        if (g == 0) stat[wave][r] = s;
        __syncthreads();
        const float mean = ((stat[0][r] + stat[1][r]) + (stat[2][r] + stat[3][r])) / (float)p.K;
        __syncthreads();
        float v = 0.f;
#pragma unroll
        for (int i = 0; i < NK; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) { const float d = xv[i][j] - mean; v += d * d; }
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (g == 0) stat[wave][r] = v;
        __syncthreads();
        const float rstd = rsqrtf(((stat[0][r] + stat[1][r]) + (stat[2][r] + stat[3][r])) / (float)p.K + p.eps);
#pragma unroll
        for (int i = 0; i < NK; ++i) {
            const float *wn = p.lnw + (ks0 + i) * 32 + g * 8;
            const f32x4 a = *reinterpret_cast<const f32x4 *>(wn), b = *reinterpret_cast<const f32x4 *>(wn + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                xv[i][j] = (xv[i][j] - mean) * rstd * a[j];
                xv[i][4 + j] = (xv[i][4 + j] - mean) * rstd * b[j];
            }
        }
#pragma unroll
        for (int i = 0; i < NK; ++i) product(xv[i], wh[i], wl[i]);
    } else {
        // every wave walks its ksw k steps U at a time (8 while that divides it: K = 1024 is then one round of loads, K = 2048 two; else
        // 4, and a last group of 2 when ksw % 4 == 2 -- two K-slices at K = 1536 or 512, one slice at K = 768), all loads of a group
        // issued before its first MFMA.  ksw = K / (128 * nsl) is even for every K the hosts accept (the ASR entry points: K % 512 == 0;
        // the GPT entry point, always one slice: K % 256 == 0).
        auto group = [&](int i0, auto uc) {
            constexpr int U = decltype(uc)::value;
            float xv[U][8];
            bf16x8 wh[U][NT], wl[U][NT];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int ks = ks0 + i0 + u;
                const f32x4 a = *reinterpret_cast<const f32x4 *>(xr + ks * 32), b = *reinterpret_cast<const f32x4 *>(xr + ks * 32 + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) { xv[u][j] = rok ? a[j] : 0.f; xv[u][4 + j] = rok ? b[j] : 0.f; }
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    wh[u][nt] = *reinterpret_cast<const bf16x8 *>(wbase[nt] + (long)ks * 2048);
                    if constexpr (PASSES == 3) wl[u][nt] = *reinterpret_cast<const bf16x8 *>(wbase[nt] + (long)ks * 2048 + 1024);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) product(xv[u], wh[u], wl[u]);
        };
        if (ksw % 8 == 0) {
            for (int i0 = 0; i0 < ksw; i0 += 8) group(i0, std::integral_constant<int, 8>{});
        } else {
            int i0 = 0;
            for (; i0 + 4 <= ksw; i0 += 4) group(i0, std::integral_constant<int, 4>{});
            if (i0 < ksw) group(i0, std::integral_constant<int, 2>{});
        }
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int e = 0; e < 4; ++e) red[wave][nt][lane][e] = acc[nt][e];
    __syncthreads();
    if constexpr (!std::is_same<ARGS, DecLinearArgs>::value) {
        p.template finish<NT>(red, nt0);
        return;
    }
    // D layout of the 16x16 MFMA: column = lane % 16 (feature), rows 4*(lane/16) + e
    for (int u = threadIdx.x; u < NT * 64; u += 256) {
        const int nt = u >> 6, l = u & 63;
        if (nt0 + nt >= p.n_tiles) continue;
        const int col = (nt0 + nt) * 16 + (l & 15);
        if (col >= p.n_out) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int orow = blockIdx.y * 16 + 4 * (l >> 4) + e;
            if (orow >= p.rows) continue;
            float v = (red[0][nt][l][e] + red[1][nt][l][e]) + (red[2][nt][l][e] + red[3][nt][l][e]);
            v = gemm_activation(v, p.flags & ACT);
            const long oi = (long)orow * p.ldo + col;
            if (kslice == 1) { p.side_out[oi] = v; continue; }         // the second half of K: alone, for the next launch to add
            float *o = p.out + oi;
            if (p.flags & 4) v += p.side_in ? *o + p.side_in[oi] : *o;
            *o = v;
        }
    }
}

}  // namespace
