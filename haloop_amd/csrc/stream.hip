// Streaming LSTM-CTC recognition (haloop_amd/streaming.py): the two launches around the LSTM of one chunk.
//
//   halo_stream_front   one workgroup per stream: the stride-4 convolution over [carry | chunk] (or [carry | tail | 3 zeros] when the
//                       stream ends) with ReLU, time-major like halo_subsample_fwd; the stream's step count; the new carry (the chunk's
//                       last 3 frames); for a stream that begins, the reset of its recurrent state and of its hypothesis.
//   halo_stream_head    one workgroup per stream: classifier -> log_softmax -> best class per step (the product as in head.hip's
//                       ctc_head_greedy2_kernel), or the best class of log-probs the caller computed (collapse-only mode); the greedy
//                       collapse continued from the label the previous call ended on; the LSTM state of the streams that go on.
//   halo_stream_logits  one workgroup per stream, for the transducer head: the classifier product alone -- logits, no
//                       softmax, zeros past the stream's steps -- or, on logits the caller computed, that zeroing alone; the same commit
//                       of the LSTM state.
//
// Both are fp32, take no atomics and sum in a fixed order: a stream's results do not depend on which other streams share the launch.
// A stream is touched by exactly one workgroup per launch, so the carry and the hypothesis are read and replaced without a hand-off
// between workgroups.
#include <float.h>
#include "halo_common.h"
#include "halo_internal.h"
#include "ctc_head_dev.h"

namespace {

constexpr int KS = 5, STRIDE = 4, CARRY = 3;      // the reference's subsample geometry (ha/rnn.py:9): the only one streamed
constexpr int FLAG_ACTIVE = 1, FLAG_BEGIN = 2, FLAG_FINAL = 4;
constexpr int MAX_STEPS = 64;                     // steps of one call (the head keeps them in LDS)

struct FrontArgs {
    const float *frames;       // [B][Tc][F]
    float *carry;              // [B][3][F]
    const int *length, *flags; // [B]
    const float *w, *bias;     // [C][F][5], [C]
    float *y;                  // [S][B][C]
    int *n_steps;              // [B]
    float *h, *c;              // [L][B][H] persistent state (rows of beginning streams are zeroed)
    int64_t *hyp;              // [B][capacity] (the row of a beginning stream is zeroed)
    int64_t *hyp_len, *steps;  // [B]
    float *score;              // [B]
    int *last_label;           // [B]
    unsigned char *truncated;  // [B]
    int B, Tc, F, C, S, L, H, capacity;
};

// element f of row i of the stream's convolution input: rows 0..2 the carry (zeros when the stream begins), then `len` frames, then zeros
__device__ __forceinline__ float front_input(const FrontArgs &p, int b, int i, int f, int len, bool begin) {
    if (i < CARRY) return begin ? 0.f : p.carry[((long)b * CARRY + i) * p.F + f];
    const int t = i - CARRY;
    return t < len ? p.frames[((long)b * p.Tc + t) * p.F + f] : 0.f;
}

// STAGED: the 4 S + 1 input rows of the stream sit in LDS (every output of a step reads the same 5 rows: broadcast reads); otherwise
// (a window beyond the LDS: very wide features) they are read from global memory in place
template <bool STAGED>
__global__ __launch_bounds__(256) void stream_front_kernel(const FrontArgs p) {
    extern __shared__ __attribute__((aligned(16))) float win[];      // [4 S + 1][F] when STAGED
    const int b = blockIdx.x, tid = threadIdx.x;
    const int F = p.F, C = p.C, S = p.S;
    const int flags = p.flags[b];
    const bool active = flags & FLAG_ACTIVE, begin = flags & FLAG_BEGIN, final = flags & FLAG_FINAL;
    if (!active) {                        // nothing of the stream changes; the LSTM still reads defined inputs
        for (int idx = tid; idx < S * C; idx += 256) p.y[((long)(idx / C) * p.B + b) * C + idx % C] = 0.f;
        if (tid == 0) p.n_steps[b] = 0;
        return;
    }
    const int len = max(0, min(p.length[b], p.Tc));
    const int n = min(S, final ? (len + 1) / STRIDE + 1 : len / STRIDE);
    const int rows = STRIDE * S + 1;
    if (STAGED) {
        for (int idx = tid; idx < rows * F; idx += 256) win[idx] = front_input(p, b, idx / F, idx % F, len, begin);
        __syncthreads();
    }
    // thread = (channel, group of four steps): the channel's 5 F weights are read once per four outputs
    const int groups = (S + 3) / 4;
    for (int item = tid; item < C * groups; item += 256) {
        const int ch = item % C, s0 = (item / C) * 4;
        const float *wr = p.w + (long)ch * F * KS;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
        for (int f = 0; f < F; ++f) {
            float wv[KS];
#pragma unroll
            for (int k = 0; k < KS; ++k) wv[k] = wr[f * KS + k];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int s = min(s0 + q, S - 1);             // (a clamped step repeats the last one; it is not stored)
#pragma unroll
                for (int k = 0; k < KS; ++k) {
                    const int i = STRIDE * s + k;
                    const float xv = STAGED ? win[i * F + f] : front_input(p, b, i, f, len, begin);
                    acc[q] = fmaf(wv[k], xv, acc[q]);
                }
            }
        }
        const float bv = p.bias[ch];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int s = s0 + q;
            if (s < S) p.y[((long)s * p.B + b) * C + ch] = s < n ? fmaxf(acc[q] + bv, 0.f) : 0.f;
        }
    }
    if (begin) {
        for (int idx = tid; idx < p.L * p.H; idx += 256) {
            const long o = ((long)(idx / p.H) * p.B + b) * p.H + idx % p.H;
            p.h[o] = 0.f; p.c[o] = 0.f;
        }
        for (int idx = tid; idx < p.capacity; idx += 256) p.hyp[(long)b * p.capacity + idx] = 0;
        if (tid == 0) { p.hyp_len[b] = 0; p.steps[b] = 0; p.score[b] = 0.f; p.last_label[b] = -1; p.truncated[b] = 0; }
    }
    if (tid == 0) p.n_steps[b] = n;
    if (!final) {
        // the new carry: the last 3 of the len (= Tc) frames.  Every read of the old carry by this workgroup -- the only one that reads
        // this stream's -- lies before the barrier
        __syncthreads();
        for (int idx = tid; idx < CARRY * F; idx += 256) {
            const int t = len - CARRY + idx / F, f = idx % F;
            p.carry[(long)b * CARRY * F + idx] = t >= 0 ? p.frames[((long)b * p.Tc + t) * F + f] : 0.f;
        }
    }
}

struct HeadArgs {
    const float *feats;        // [B][S][H] (fused) or nullptr
    const float *w, *bias;     // [V][H], [V]
    const float *lp_in;        // [B][S][V] (collapse-only mode) or nullptr
    float *lp_out;             // [B][S][V] or nullptr (fused mode)
    const int *n_steps, *flags;
    const float *hn, *cn;      // [L][B][H] the LSTM's final state of this call
    float *h, *c;              // [L][B][H] persistent state
    int64_t *ali;              // [B][S]
    float *step_scores;        // [B][S]
    int64_t *hyp, *hyp_len, *steps;
    float *score;
    int *last_label;
    unsigned char *truncated;
    int B, S, H, V, L, capacity;
};

// the LSTM's final state of this call becomes stream b's persistent state (the streams that go on; stated once for both heads)
__device__ __forceinline__ void stream_commit_state(float *h, float *c, const float *hn, const float *cn, int L, int H, int B, int b) {
    for (int idx = threadIdx.x; idx < L * H; idx += TNT) {
        const long o = ((long)(idx / H) * B + b) * H + idx % H;
        h[o] = hn[o]; c[o] = cn[o];
    }
}

// the steps' best classes are in best_s / bv_s: continue the stream's collapse (one lane: at most MAX_STEPS dependent steps), commit the state
__device__ __forceinline__ void head_finish(const HeadArgs &p, int b, int n, bool active, bool final, const int *best_s, const float *bv_s) {
    const int tid = threadIdx.x;
    for (int s = tid; s < p.S; s += TNT) {
        p.ali[(long)b * p.S + s] = s < n ? best_s[s] : 0;
        p.step_scores[(long)b * p.S + s] = s < n ? bv_s[s] : 0.f;
    }
    if (!active) return;
    if (tid == 0 && n > 0) {
        int last = p.last_label[b];
        long len = p.hyp_len[b];
        float score = p.score[b];
        bool trunc = false;
        for (int s = 0; s < n; ++s) {
            const int lab = best_s[s];
            if (lab != last && lab != 0) {
                if (len < p.capacity) p.hyp[(long)b * p.capacity + len++] = lab;
                else trunc = true;
            }
            last = lab;
            score += bv_s[s];                    // in step order
        }
        p.last_label[b] = last; p.hyp_len[b] = len; p.score[b] = score; p.steps[b] += n;
        if (trunc) p.truncated[b] = 1;
    }
    if (!final) stream_commit_state(p.h, p.c, p.hn, p.cn, p.L, p.H, p.B, b);
}

// classifier product on split-bf16 MFMA with the fragments straight from global memory, log_softmax, best class: the steps of one
// stream are one 32-row tile and the classes one 32-column tile (halo_ctc_head_supported), as ctc_head_greedy2_kernel
__global__ __launch_bounds__(TNT) void stream_head_fused_kernel(const HeadArgs p) {
    extern __shared__ __attribute__((aligned(16))) float redg[];      // [TNW][1024]
    __shared__ float tile[32][LDT];
    __shared__ int best_s[MAX_STEPS];
    __shared__ float bv_s[MAX_STEPS];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int S = p.S, H = p.H, V = p.V;
    const int flags = p.flags[b];
    const bool active = flags & FLAG_ACTIVE, final = flags & FLAG_FINAL;
    const int n = active ? max(0, min(p.n_steps[b], S)) : 0;
    if (n == 0) {                         // (uniform over the workgroup)
        head_finish(p, b, 0, active, final, best_s, bv_s);
        return;
    }
    const int r = lane & 31, kh = lane >> 5;
    const f32x16 acc = head_logits_x3(p.feats, (long)b * S, n, p.w, V, H, H / 16, wave, r, kh);
    const int tj = tid & 31;
    float lpv[2];
    head_put_acc(acc, redg, wave, r, kh);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 2; ++q) lpv[q] = log_softmax32((tj < V) ? head_sum_waves(redg, q) + p.bias[tj] : -INFINITY, tj < V);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int ti = (tid >> 5) + 16 * q;
        tile[ti][tj] = lpv[q];
        if (p.lp_out && tj < V && ti < S) p.lp_out[((long)b * S + ti) * V + tj] = ti < n ? lpv[q] : 0.f;
    }
    __syncthreads();
    if (tid < n) {                        // one lane per step: the first maximum, like torch.max and halo_ctc_greedy
        float bv;
        best_s[tid] = row_argmax(tile, tid, V, bv);
        bv_s[tid] = bv;
    }
    __syncthreads();
    head_finish(p, b, n, active, final, best_s, bv_s);
}

// collapse-only mode: the log-probs [B][S][V] are the caller's (any V); wave w takes steps w, w + 8, ...
__global__ __launch_bounds__(TNT) void stream_head_collapse_kernel(const HeadArgs p) {
    __shared__ int best_s[MAX_STEPS];
    __shared__ float bv_s[MAX_STEPS];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int S = p.S, V = p.V;
    const int flags = p.flags[b];
    const bool active = flags & FLAG_ACTIVE, final = flags & FLAG_FINAL;
    const int n = active ? max(0, min(p.n_steps[b], S)) : 0;
    for (int s = wave; s < n; s += TNW) {
        const float *row = p.lp_in + ((long)b * S + s) * V;
        int best = 0x7fffffff;
        float bv = -INFINITY;
        for (int cc = lane; cc < V; cc += 64) {           // ascending classes: a strict > keeps the lane's lowest index
            const float v = row[cc];
            if (v > bv || best == 0x7fffffff) { bv = v; best = cc; }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const float ov = __shfl_xor(bv, d, 64);
            const int ob = __shfl_xor(best, d, 64);
            if (ob != 0x7fffffff && (best == 0x7fffffff || ov > bv || (ov == bv && ob < best))) { bv = ov; best = ob; }
        }
        if (lane == 0) { best_s[s] = best; bv_s[s] = bv; }
    }
    __syncthreads();
    head_finish(p, b, n, active, final, best_s, bv_s);
}

struct LogitsArgs {
    const float *feats;        // [B][S][H] (fused) or nullptr: f holds the caller's product
    const float *w, *bias;     // [V][H], [V]
    float *f;                  // [B][S][V]
    const int *n_steps, *flags;
    const float *hn, *cn;
    float *h, *c;
    int64_t *steps;            // [B] += n_steps
    int B, S, H, V, L;
};

// FUSED: the tile product of stream_head_fused_kernel, its sums plus the bias stored as they are.  Otherwise f is the caller's: only the
// steps past the stream's own are written (zeros).  Both commit the state.
template <bool FUSED>
__global__ __launch_bounds__(TNT) void stream_logits_kernel(const LogitsArgs p) {
    extern __shared__ __attribute__((aligned(16))) float redg[];      // [TNW][1024] when FUSED
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int S = p.S, V = p.V;
    const int flags = p.flags[b];
    const bool active = flags & FLAG_ACTIVE, final = flags & FLAG_FINAL;
    const int n = active ? max(0, min(p.n_steps[b], S)) : 0;
    if (FUSED && n > 0) {                 // (uniform over the workgroup)
        const int r = lane & 31, kh = lane >> 5;
        const f32x16 acc = head_logits_x3(p.feats, (long)b * S, n, p.w, V, p.H, p.H / 16, wave, r, kh);
        head_put_acc(acc, redg, wave, r, kh);
        __syncthreads();
        const int tj = tid & 31;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int ti = (tid >> 5) + 16 * q;
            const float v = head_sum_waves(redg, q);
            if (tj < V && ti < S) p.f[((long)b * S + ti) * V + tj] = ti < n ? v + p.bias[tj] : 0.f;
        }
    } else {
        for (int idx = tid + n * V; idx < S * V; idx += TNT) p.f[(long)b * S * V + idx] = 0.f;
    }
    if (!active) return;
    if (tid == 0) p.steps[b] += n;
    if (!final) stream_commit_state(p.h, p.c, p.hn, p.cn, p.L, p.H, p.B, b);
}

}  // namespace

extern "C" {

int halo_stream_front(const float *frames, float *carry, const int *length, const int *flags, const float *weight, const float *bias,
                      float *y, int *n_steps, float *h, float *c, int64_t *hyp, int64_t *hyp_len, int64_t *steps, float *score,
                      int *last_label, unsigned char *truncated, int B, int Tc, int F, int C, int S, int L, int H, int capacity,
                      halo_stream_t stream) {
    HALO_CHECK_ARG(frames && carry && length && flags && weight && bias && y && n_steps && h && c && hyp && hyp_len && steps &&
                   score && last_label && truncated);
    HALO_CHECK_ARG(B > 0 && Tc > 0 && F > 0 && C > 0 && S > 0 && L > 0 && H > 0 && capacity > 0);
    // (input rows past a stream's frames read as zeros, whatever S: no step reads outside [B][Tc][F])
    if (S > MAX_STEPS) return HALO_ENOTSUP;
    FrontArgs a;
    a.frames = frames; a.carry = carry; a.length = length; a.flags = flags; a.w = weight; a.bias = bias; a.y = y; a.n_steps = n_steps;
    a.h = h; a.c = c; a.hyp = hyp; a.hyp_len = hyp_len; a.steps = steps; a.score = score; a.last_label = last_label; a.truncated = truncated;
    a.B = B; a.Tc = Tc; a.F = F; a.C = C; a.S = S; a.L = L; a.H = H; a.capacity = capacity;
    const size_t lds = (size_t)(STRIDE * S + 1) * F * sizeof(float);
    if (lds <= 64 * 1024)          // (within what a launch may ask for without an opt-in)
        hipLaunchKernelGGL(stream_front_kernel<true>, dim3(B), dim3(256), lds, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(stream_front_kernel<false>, dim3(B), dim3(256), 0, (hipStream_t)stream, a);
    return halo_launch_status();
}

int halo_stream_head(const float *feats, const float *weight, const float *bias, const float *lp_in, float *lp_out, const int *n_steps,
                     const int *flags, const float *hn, const float *cn, float *h, float *c, int64_t *alignments, float *step_scores,
                     int64_t *hyp, int64_t *hyp_len, int64_t *steps, float *score, int *last_label, unsigned char *truncated, int B,
                     int S, int H, int V, int L, int capacity, halo_stream_t stream) {
    HALO_CHECK_ARG(n_steps && flags && hn && cn && h && c && alignments && step_scores && hyp && hyp_len && steps && score && last_label &&
                   truncated);
    HALO_CHECK_ARG(B > 0 && S > 0 && H > 0 && V > 0 && L > 0 && capacity > 0);
    HALO_CHECK_ARG((lp_in != nullptr) != (feats != nullptr));
    if (S > MAX_STEPS) return HALO_ENOTSUP;
    HeadArgs a;
    a.feats = feats; a.w = weight; a.bias = bias; a.lp_in = lp_in; a.lp_out = lp_out; a.n_steps = n_steps; a.flags = flags;
    a.hn = hn; a.cn = cn; a.h = h; a.c = c; a.ali = alignments; a.step_scores = step_scores; a.hyp = hyp; a.hyp_len = hyp_len;
    a.steps = steps; a.score = score; a.last_label = last_label; a.truncated = truncated;
    a.B = B; a.S = S; a.H = H; a.V = V; a.L = L; a.capacity = capacity;
    if (lp_in) {
        hipLaunchKernelGGL(stream_head_collapse_kernel, dim3(B), dim3(TNT), 0, (hipStream_t)stream, a);
        return halo_launch_status();
    }
    HALO_CHECK_ARG(weight && bias);
    // the fused product is split-bf16: the exact-f32 mode takes the collapse-only route behind halo_gemm_f32, like halo_ctc_head_train
    if (!halo_ctc_head_supported(S, H, V, 0) || halo_math_mode() == HALO_MATH_F32) return HALO_ENOTSUP;
    HALO_CHECK_ARG(((uintptr_t)feats % 16 == 0) && ((uintptr_t)weight % 16 == 0));
    hipLaunchKernelGGL(stream_head_fused_kernel, dim3(B), dim3(TNT), (size_t)TNW * 1024 * sizeof(float), (hipStream_t)stream, a);
    return halo_launch_status();
}

int halo_stream_logits(const float *feats, const float *weight, const float *bias, float *f, const int *n_steps, const int *flags,
                       const float *hn, const float *cn, float *h, float *c, int64_t *steps, int B, int S, int H, int V, int L,
                       halo_stream_t stream) {
    HALO_CHECK_ARG(f && n_steps && flags && hn && cn && h && c && steps);
    HALO_CHECK_ARG(B > 0 && S > 0 && H > 0 && V > 0 && L > 0);
    if (S > MAX_STEPS) return HALO_ENOTSUP;
    LogitsArgs a;
    a.feats = feats; a.w = weight; a.bias = bias; a.f = f; a.n_steps = n_steps; a.flags = flags; a.hn = hn; a.cn = cn; a.h = h; a.c = c;
    a.steps = steps; a.B = B; a.S = S; a.H = H; a.V = V; a.L = L;
    if (!feats) {                     // commit-only: f is the caller's product
        hipLaunchKernelGGL(stream_logits_kernel<false>, dim3(B), dim3(TNT), 0, (hipStream_t)stream, a);
        return halo_launch_status();
    }
    HALO_CHECK_ARG(weight && bias);
    if (!halo_ctc_head_supported(S, H, V, 0) || halo_math_mode() == HALO_MATH_F32) return HALO_ENOTSUP;
    HALO_CHECK_ARG(((uintptr_t)feats % 16 == 0) && ((uintptr_t)weight % 16 == 0));
    hipLaunchKernelGGL(stream_logits_kernel<true>, dim3(B), dim3(TNT), (size_t)TNW * 1024 * sizeof(float), (hipStream_t)stream, a);
    return halo_launch_status();
}

}  // extern "C"
