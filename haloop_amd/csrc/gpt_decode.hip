// Fused launches of one batched GPT sampling step (haloop_amd/generation.py; ha/attention.py:253-321 with a KV cache, T == 1): per layer
//   1. LayerNorm(ln_1) + c_attn -> q | k | v rows                                  (dec_linear_kernel of decode_linear.h, LN variant)
//   2. store k / v at the row's position of the fp32 cache, attention over keys 0 .. pos   (gpt_attention_kernel)
//   3. c_proj, residual add                                                        (dec_linear_kernel, accumulate)
//   4. LayerNorm(ln_2) + c_fc + tanh-GELU                                          (dec_linear_kernel, LN variant, GELU)
//   5. mlp.c_proj, residual add                                                    (dec_linear_kernel, K = 4C, accumulate)
// and per token LayerNorm(ln_f) + lm_head (dec_linear_kernel) and the draw with its bookkeeping and the next input row
// (gpt_sample_kernel): 5 n_layer + 2 launches.  Nothing a step needs from the host changes between steps: the position, the draw
// counter, the alive flags and the draw's settings are device words, so a captured step is replayed for every position.
#include <stdlib.h>
#include "halo_common.h"
#include "halo_internal.h"
#include "decode_linear.h"

namespace {

// ---- cache store + attention of one layer.  One workgroup of NW waves per (row, head); eight lanes share a key (lane = 8 * key
//      group + dim chunk of 8), so a pass of the workgroup scores 8 NW keys; scores go through LDS, the softmax over the workgroup, then
//      each key group accumulates p * v for its keys and the groups meet by shuffles (inside a wave) and a fixed-order sum over the
//      waves.  The keys are split over the waves of ONE workgroup (NW = 16 when rows x heads leave most CUs idle: B = 1 gives 12
//      workgroups), not over workgroups: no second launch or in-launch hand-off to combine partial softmaxes.  The loops run to
//      pos + 1 <= cache_len: bounded whatever the device word holds. ----
struct GptAttnArgs {
    const float *qkv;        // [B][>= 3C]: q | k | v
    long rs;
    int C, heads;
    float *ck, *cv;          // [B][heads][Tc][64]
    int Tc;
    const int *pos;          // [B]
    float *y;                // [B][C]
    long y_rs;
};

template <int MAXK, int NW>
__global__ __launch_bounds__(64 * NW) void gpt_attention_kernel(const GptAttnArgs p) {
    constexpr int HD = 64, NT = 64 * NW, KPP = 8 * NW;
    __shared__ float ps[MAXK];
    __shared__ float red[2 * NW];
    __shared__ float part[NW][HD];
    const int h = blockIdx.x, n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = tid & 7, kg = tid >> 3;
    const int tq = min(max(p.pos[n], 0), p.Tc - 1), n_keys = tq + 1;
    const float *qp = p.qkv + (long)n * p.rs + (long)h * HD + c * 8;
    float q[8], kf[8], vf[8];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(qp + 4 * half), b = *reinterpret_cast<const f32x4 *>(qp + p.C + 4 * half),
                    d = *reinterpret_cast<const f32x4 *>(qp + 2 * p.C + 4 * half);
#pragma unroll
        for (int i = 0; i < 4; ++i) { q[4 * half + i] = a[i] * 0.125f; kf[4 * half + i] = b[i]; vf[4 * half + i] = d[i]; }
    }
    const long base = ((long)n * p.heads + h) * p.Tc * HD;
    const float *kb = p.ck + base, *vb = p.cv + base;
    if (kg == 0) {                                            // this step's key and value row
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            *reinterpret_cast<f32x4 *>(p.ck + base + (long)tq * HD + c * 8 + 4 * half) = f32x4{kf[4 * half], kf[4 * half + 1], kf[4 * half + 2], kf[4 * half + 3]};
            *reinterpret_cast<f32x4 *>(p.cv + base + (long)tq * HD + c * 8 + 4 * half) = f32x4{vf[4 * half], vf[4 * half + 1], vf[4 * half + 2], vf[4 * half + 3]};
        }
    }
    // (the loads of four passes are issued before the first is used: a pass is one round trip to the cache, and they are independent)
    for (int j0 = 0; j0 < n_keys; j0 += 4 * KPP) {
        f32x4 ka[4], kb4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + u * KPP + kg;
            if (j < n_keys && j != tq) {                      // tq: not from the store just issued
                ka[u] = *reinterpret_cast<const f32x4 *>(kb + (long)j * HD + c * 8);
                kb4[u] = *reinterpret_cast<const f32x4 *>(kb + (long)j * HD + c * 8 + 4);
            } else {
                ka[u] = f32x4{kf[0], kf[1], kf[2], kf[3]};
                kb4[u] = f32x4{kf[4], kf[5], kf[6], kf[7]};
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + u * KPP + kg;
            float sc = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) sc = fmaf(q[i], ka[u][i], sc);
#pragma unroll
            for (int i = 0; i < 4; ++i) sc = fmaf(q[4 + i], kb4[u][i], sc);
            sc += __shfl_xor(sc, 1, 64);
            sc += __shfl_xor(sc, 2, 64);
            sc += __shfl_xor(sc, 4, 64);
            if (c == 0 && j < n_keys) ps[j] = sc;
        }
    }
    __syncthreads();
    float mx = -INFINITY;
    for (int j = tid; j < n_keys; j += NT) mx = fmaxf(mx, ps[j]);
    mx = wave_max(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = red[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) mx = fmaxf(mx, red[w]);
    float sum = 0.f;
    for (int j = tid; j < n_keys; j += NT) {
        const float e = expf(ps[j] - mx);
        ps[j] = e;
        sum += e;
    }
    sum = wave_sum(sum);
    if (lane == 0) red[NW + wave] = sum;
    __syncthreads();
    float total = red[NW];
#pragma unroll
    for (int w = 1; w < NW; ++w) total += red[NW + w];
    const float inv = 1.0f / total;
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.f;
    for (int j0 = 0; j0 < n_keys; j0 += 4 * KPP) {
        f32x4 va[4], vb4[4];
        float pj[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + u * KPP + kg;
            if (j < n_keys && j != tq) {
                va[u] = *reinterpret_cast<const f32x4 *>(vb + (long)j * HD + c * 8);
                vb4[u] = *reinterpret_cast<const f32x4 *>(vb + (long)j * HD + c * 8 + 4);
            } else {
                va[u] = f32x4{vf[0], vf[1], vf[2], vf[3]};
                vb4[u] = f32x4{vf[4], vf[5], vf[6], vf[7]};
            }
            pj[u] = j < n_keys ? ps[j] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int i = 0; i < 4; ++i) { acc[i] = fmaf(pj[u], va[u][i], acc[i]); acc[4 + i] = fmaf(pj[u], vb4[u][i], acc[4 + i]); }
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        float v = acc[i];
        v += __shfl_xor(v, 8, 64);
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (lane < 8) part[wave][c * 8 + i] = v;
    }
    __syncthreads();
    if (tid < HD) {
        float o = part[0][tid];
#pragma unroll
        for (int w = 1; w < NW; ++w) o += part[w][tid];
        p.y[(long)n * p.y_rs + (long)h * HD + tid] = o * inv;
    }
}

// ---- the draw of one step and its bookkeeping (include/halo.h states the definition a CPU restatement follows).  One workgroup per
//      row; thread t owns the vocabulary chunk [t * chunk, (t + 1) * chunk).  The top-k threshold is the exact k-th largest logit, found
//      by a four-pass radix select over order-preserving keys (integer histograms in LDS: the result does not depend on the order the
//      threads arrive in). ----
struct GptSampleArgs {
    const float *logits;
    long ld;
    int B, V;
    const int *cfg;
    int *state;
    long sld;
    int64_t *tokens;
    long tld;
    int n_slots;
    int64_t *next_ids;
    const float *wte, *wpe;
    int n_pos, C;
    float *x;
};

// (-0.0 and +0.0 share a key: the kept set is defined by the float comparison >=, under which they are equal)
__device__ __forceinline__ unsigned order_key(float f) {
    const unsigned b = __float_as_uint(f);
    if (b == 0x80000000u) return 0x80000000u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__global__ __launch_bounds__(256) void gpt_sample_kernel(const GptSampleArgs p) {
    __shared__ unsigned hist[256];
    __shared__ float fred[256], part[256];
    __shared__ int ired[256];
    __shared__ unsigned s_sel[2];
    __shared__ float s_target;
    __shared__ int s_chunk, s_tok, s_id, s_pos;
    const int row = blockIdx.x, tid = threadIdx.x, V = p.V;
    const float *lg = p.logits + (long)row * p.ld;
    const float inv_t = __int_as_float(p.cfg[0]);
    const int top_k = p.cfg[1], stop = p.cfg[2];
    const unsigned k0 = (unsigned)p.cfg[3], k1 = (unsigned)p.cfg[4];
    const int step = p.state[p.sld + row];
    // float4 loads where the row allows them; thread t then owns elements 4 t + e + 1024 k of the coalesced passes
    const bool vec = V % 4 == 0 && p.ld % 4 == 0 && (uintptr_t)p.logits % 16 == 0;
    auto load4 = [&](int i) {                                 // elements i .. i + 3 (i % 4 == 0), -inf past the row
        if (vec) return i < V ? *reinterpret_cast<const f32x4 *>(lg + i) : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        f32x4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = i + e < V ? lg[i + e] : -INFINITY;
        return r;
    };
    // the largest logit and its lowest index
    float m = -INFINITY;
    int am = 0x7fffffff;
    for (int i = tid * 4; i < V; i += 4096) {
        f32x4 b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) b[u] = load4(i + 1024 * u);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (b[u][e] > m) { m = b[u][e]; am = i + 1024 * u + e; }
    }
    const unsigned mykey = order_key(m);                      // this thread's largest: 256 distinct elements of the row
    fred[tid] = m; ired[tid] = am;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            const float om = fred[tid + o];
            const int oa = ired[tid + o];
            if (om > fred[tid] || (om == fred[tid] && oa < ired[tid])) { fred[tid] = om; ired[tid] = oa; }
        }
        __syncthreads();
    }
    m = fred[0];
    am = ired[0] == 0x7fffffff ? 0 : ired[0];
    __syncthreads();
    int token = am;
    if (top_k != 1) {
        unsigned thr = 0u;                                    // keep every key >= thr
        if (top_k > 1 && top_k < V) {
            // A floor under the threshold first: the k-th largest of the 256 thread maxima (k distinct elements are at least that
            // large, so the row's k-th largest is too).  Only keys at or above the floor enter the histograms: a few hundred LDS
            // atomics instead of V, and the k-th largest of those candidates is the k-th largest of the row.
            unsigned floor_key = 0u;
            if (top_k <= 256) {
                hist[tid] = mykey;
                if (tid == 0) s_sel[0] = 0u;
                __syncthreads();
                int gt = 0, ge = 0;
                for (int t = 0; t < 256; ++t) {
                    const unsigned o = hist[t];
                    gt += o > mykey; ge += o >= mykey;
                }
                if (gt < top_k && top_k <= ge) s_sel[0] = mykey;       // (every thread that qualifies holds the same key)
                __syncthreads();
                floor_key = s_sel[0];
                __syncthreads();
            }
            unsigned prefix = 0u, mask = 0u;
            int krem = top_k;
            for (int pass = 3; pass >= 0; --pass) {
                hist[tid] = 0u;
                __syncthreads();
                for (int i = tid * 4; i < V; i += 4096) {
                    f32x4 b[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) b[u] = load4(i + 1024 * u);
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const unsigned key = order_key(b[u][e]);
                            if (i + 1024 * u + e < V && key >= floor_key && (key & mask) == prefix) atomicAdd(&hist[(key >> (8 * pass)) & 255u], 1u);
                        }
                }
                __syncthreads();
                if (tid == 0) {                               // the bin that holds the krem-th largest of the keys still in play
                    int cum = 0, b = 255;
                    for (; b > 0; --b) {
                        if (cum + (int)hist[b] >= krem) break;
                        cum += (int)hist[b];
                    }
                    s_sel[0] = (unsigned)b; s_sel[1] = (unsigned)(krem - cum);
                }
                __syncthreads();
                prefix |= s_sel[0] << (8 * pass);
                mask |= 0xffu << (8 * pass);
                krem = (int)s_sel[1];
                __syncthreads();
            }
            thr = prefix;
        }
        const float ms = m * inv_t;
        const int chunk = 4 * ((V + 1023) / 1024), i0 = min(V, tid * chunk), i1 = min(V, i0 + chunk);
        float s = 0.f;
        for (int i = i0; i < i1; i += 32) {                    // eight loads in flight, then the sums left to right
            f32x4 b[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) b[u] = load4(i + 4 * u);
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float v = b[u][e];
                    if (i + 4 * u + e < i1 && order_key(v) >= thr) s += expf(v * inv_t - ms);
                }
        }
        part[tid] = s;
        __syncthreads();
        if (tid == 0) {
            float cum = 0.f;
            int last = 0;
            for (int t = 0; t < 256; ++t) {
                fred[t] = cum;                                // the chunk's prefix
                cum += part[t];
                if (part[t] > 0.f) last = t;
            }
            const unsigned r = philox4x32_10((unsigned)row, 0u, HALO_GPT_SAMPLE_STREAM, (unsigned)step, k0, k1).v[0];
            const float target = (float)(r >> 8) * 5.9604644775390625e-8f * cum;
            int sel = last;                                   // (rounding left nothing above the target: the last chunk with mass)
            for (int t = 0; t < 256; ++t)
                if (fred[t] + part[t] > target) { sel = t; break; }
            s_target = target; s_chunk = sel; s_tok = am;
        }
        __syncthreads();
        if (tid == s_chunk) {
            const float target = s_target, pre = fred[tid];
            float run = 0.f;
            int tok = -1, lastkept = -1;
            for (int i = i0; i < i1 && tok < 0; i += 32) {
                f32x4 b[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) b[u] = load4(i + 4 * u);
#pragma unroll
                for (int u = 0; u < 8; ++u)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float v = b[u][e];
                        if (tok >= 0 || i + 4 * u + e >= i1 || order_key(v) < thr) continue;
                        run += expf(v * inv_t - ms);
                        lastkept = i + 4 * u + e;
                        if (pre + run > target) tok = i + 4 * u + e;
                    }
            }
            if (tok < 0) tok = lastkept;
            if (tok >= 0) s_tok = tok;
        }
        __syncthreads();
        token = s_tok;
    }
    if (tid == 0) {
        const int pos = p.state[row] + 1;
        int len = p.state[2 * p.sld + row], alive = p.state[3 * p.sld + row];
        long tok = token;
        if (alive) {
            if (tok == (long)stop) alive = 0;                 // the stop token is not emitted (ha/attention.py:318-319)
            else len += 1;
        }
        if (!alive) tok = stop;
        if (step >= 0 && step < p.n_slots) p.tokens[(long)row * p.tld + step] = tok;
        const int id = (int)(tok < 0 ? 0 : (tok >= V ? V - 1 : tok));
        p.next_ids[row] = id;
        p.state[row] = pos;
        p.state[p.sld + row] = step + 1;
        p.state[2 * p.sld + row] = len;
        p.state[3 * p.sld + row] = alive;
        s_id = id;
        s_pos = min(max(pos, 0), p.n_pos - 1);
    }
    if (!p.x) return;
    __syncthreads();
    const f32x4 *te = reinterpret_cast<const f32x4 *>(p.wte + (long)s_id * p.C), *pe = reinterpret_cast<const f32x4 *>(p.wpe + (long)s_pos * p.C);
    for (int u = tid; u < p.C / 4; u += 256) reinterpret_cast<f32x4 *>(p.x + (long)row * p.C)[u] = te[u] + pe[u];
}

}  // namespace

extern "C" {

int halo_gpt_decode_linear_supported(int k, int layernorm) {
    if (halo_math_mode() == HALO_MATH_F32) return 0;
    if (layernorm) return k == 512 || k == 768 || k == 1024;
    return k > 0 && k % 256 == 0;
}

int halo_gpt_decode_linear(const float *x, long ldx, int rows, int k, const float *ln_weight, float eps, const void *w_image, int n_out,
                           float *out, long ldo, int flags, halo_stream_t stream) {
    HALO_CHECK_ARG(x && w_image && out && rows > 0 && n_out > 0 && ldx >= k && ldo >= n_out);
    HALO_CHECK_ARG((flags & ~(HALO_GEMM_ACCUM | HALO_GEMM_GELU)) == 0);
    HALO_CHECK_ARG(((uintptr_t)x | (uintptr_t)w_image | (uintptr_t)ln_weight) % 16 == 0 && ldx % 4 == 0);
    const int mode = halo_math_mode();
    if (mode == HALO_MATH_F32) return HALO_ENOTSUP;
    HALO_CHECK_ARG(halo_gpt_decode_linear_supported(k, ln_weight != nullptr));
    DecLinearArgs p;
    p.x = x; p.ldx = ldx; p.rows = rows; p.K = k; p.lnw = ln_weight; p.eps = eps; p.w = (const char *)w_image;
    p.n_tiles = (n_out + 15) / 16; p.n_out = n_out; p.out = out; p.ldo = ldo; p.flags = flags;
    p.x2 = nullptr; p.side_in = nullptr; p.side_out = nullptr;
    const int row_groups = (rows + 15) / 16;
    // two feature tiles per workgroup while that still gives the chip a workgroup per CU, else one
    const bool two = (long)((p.n_tiles + 1) / 2) * row_groups >= 256;
    const dim3 grid((unsigned)(two ? (p.n_tiles + 1) / 2 : p.n_tiles), (unsigned)row_groups, 1);
    hipStream_t st = (hipStream_t)stream;
#define HALO_GPT_LAUNCH(LN, PASSES)                                                                       \
    do {                                                                                                  \
        if (two) hipLaunchKernelGGL((dec_linear_kernel<2, LN, PASSES, 2>), grid, dim3(256), 0, st, p);    \
        else hipLaunchKernelGGL((dec_linear_kernel<1, LN, PASSES, 2>), grid, dim3(256), 0, st, p);        \
    } while (0)
#define HALO_GPT_LAUNCH_LN(PASSES)                  \
    do {                                            \
        if (!ln_weight) HALO_GPT_LAUNCH(0, PASSES); \
        else if (k == 512) HALO_GPT_LAUNCH(4, PASSES); \
        else if (k == 768) HALO_GPT_LAUNCH(6, PASSES); \
        else HALO_GPT_LAUNCH(8, PASSES);            \
    } while (0)
    if (mode == HALO_MATH_BF16) HALO_GPT_LAUNCH_LN(1);
    else HALO_GPT_LAUNCH_LN(3);
#undef HALO_GPT_LAUNCH_LN
#undef HALO_GPT_LAUNCH
    return halo_launch_status();
}

int halo_gpt_decode_attention(const float *qkv, long row_stride, int B, int heads, int head_dim, float *cache_k, float *cache_v, int cache_len,
                              const int *pos, float *y, long y_row_stride, halo_stream_t stream) {
    HALO_CHECK_ARG(qkv && cache_k && cache_v && pos && y && B > 0 && B <= 65535 && heads > 0 && cache_len > 0);
    if (head_dim != 64 || cache_len > 8192) return HALO_ENOTSUP;
    const int C = heads * head_dim;
    HALO_CHECK_ARG(row_stride >= 3L * C && y_row_stride >= C && row_stride % 4 == 0);
    HALO_CHECK_ARG(((uintptr_t)qkv | (uintptr_t)cache_k | (uintptr_t)cache_v) % 16 == 0);
    GptAttnArgs p;
    p.qkv = qkv; p.rs = row_stride; p.C = C; p.heads = heads; p.ck = cache_k; p.cv = cache_v; p.Tc = cache_len; p.pos = pos;
    p.y = y; p.y_rs = y_row_stride;
    const dim3 grid((unsigned)heads, (unsigned)B);
    // few (row, head) pairs: sixteen waves share a pair's keys; else four.  HALO_GPT_ATTN_WAVES=4|16, read once per process, pins one
    // (measurement switch of tools/bench_gpt_generate.py)
    static const int pinned = [] { const char *pin = getenv("HALO_GPT_ATTN_WAVES"); return pin ? atoi(pin) : 0; }();
    const bool wide = pinned == 16 || (pinned != 4 && (long)B * heads <= 128);
    hipStream_t st = (hipStream_t)stream;
    if (cache_len <= 1024) {
        if (wide) hipLaunchKernelGGL((gpt_attention_kernel<1024, 16>), grid, dim3(1024), 0, st, p);
        else hipLaunchKernelGGL((gpt_attention_kernel<1024, 4>), grid, dim3(256), 0, st, p);
    } else {
        if (wide) hipLaunchKernelGGL((gpt_attention_kernel<8192, 16>), grid, dim3(1024), 0, st, p);
        else hipLaunchKernelGGL((gpt_attention_kernel<8192, 4>), grid, dim3(256), 0, st, p);
    }
    return halo_launch_status();
}

int halo_gpt_sample(const float *logits, long ld, int B, int V, const int *cfg, int *state, long state_ld, int64_t *tokens, long tokens_ld,
                    int n_slots, int64_t *next_ids, const float *wte, const float *wpe, int n_pos, int C, float *x_next,
                    halo_stream_t stream) {
    HALO_CHECK_ARG(logits && cfg && state && tokens && next_ids && B > 0 && V > 0 && ld >= V && state_ld >= B && n_slots >= 0 &&
                   tokens_ld >= n_slots);
    HALO_CHECK_ARG(!x_next || (wte && wpe && n_pos > 0 && C > 0 && C % 4 == 0 && ((uintptr_t)wte | (uintptr_t)wpe | (uintptr_t)x_next) % 16 == 0));
    GptSampleArgs p;
    p.logits = logits; p.ld = ld; p.B = B; p.V = V; p.cfg = cfg; p.state = state; p.sld = state_ld; p.tokens = tokens; p.tld = tokens_ld;
    p.n_slots = n_slots; p.next_ids = next_ids; p.wte = wte; p.wpe = wpe; p.n_pos = n_pos; p.C = C; p.x = x_next;
    hipLaunchKernelGGL(gpt_sample_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, p);
    return halo_launch_status();
}

}  // extern "C"
