// Device-side building blocks of the CTC head family, each stated once: the plain CTC loss (ctc.hip), the two-launch and the one-launch
// training head and the greedy decode head (head.hip), the streaming head (stream.hip).
//
// The lattice recursions are NOT here: three alphas and two betas stay where they run, because they round differently on purpose and
// tests/test_gpu_ctc_f64.py bounds every route by its own form:
//   ctc_alpha_wave_kernel / ctc_beta_grad_wave_kernel (ctc.hip)   two chained log_add_exp_fast per step, neighbours by __shfl_up / __shfl_down,
//                                                                 the flag variants of halo_ctc_fwd (full lattice, finite minimum, wrap skip)
//   ctc_head_fwd_kernel / ctc_head_bwd_kernel (head.hip)          one log_add_exp_fast3 per step (one exp and one log latency), neighbours
//                                                                 by DPP (wave_up1 / wave_down1), F.ctc_loss semantics only
//   ctc_head_train_kernel (head.hip)                              alpha and beta side by side in log2 units (no scaling inside the chain),
//                                                                 masks folded into -inf operands
// ctc_alpha_kernel / ctc_beta_grad_kernel (ctc.hip, any number of states) use libm through halo_common.h's log_add_exp.
#pragma once
#include "halo_common.h"
#include "dev_util.h"

namespace {

constexpr int TNW = 8, TNT = 64 * TNW;    // the split-bf16 head kernels: 512 threads (256 VGPRs per lane: two passes of fragments, two prefetched tiles)
constexpr int LDT = 33;                   // padded leading dimension of the [32][32] tiles in LDS

// label of lattice state s: blanks at the even states, target s / 2 at the odd ones
__device__ __forceinline__ int ext_label(const int64_t *tg, int s) { return (s & 1) ? (int)tg[s >> 1] : 0; }

// log(e^a + e^b) on the hardware exp2/log2 units (v_exp_f32 / v_log_f32): ~1e-7 absolute error per call,
// an order below the lattice's own fp32 rounding over T steps; the serial chain is ~10x shorter than
// with the libm-accurate expf/log1pf, which is what bounds a one-wave-per-utterance recursion.  Measured against float64
// (tests/test_gpu_ctc_f64.py): at T = 480, 63 states, the wave forward's 1600-nat loss comes out 6.6e-4 off; at T = 70 and T = 32 both wave
// kernels are 1.4e-5 (losses) and 2e-5 (gradients) off -- to the printed digit what a float32 run of the same recursion with libm loses,
// so the fast forms add nothing measurable.
__device__ __forceinline__ float log_add_exp_fast(float a, float b) {
    if (isinf(a) && a == b) return a;
    const float m = fmaxf(a, b);
    return m + __logf(1.0f + __expf(-fabsf(a - b)));
}
// log(e^a + e^b + e^c) the way ATen's CTC loss writes it (max, three exponentials, one log: LossCTC.cpp): the exponentials are
// independent, so a lattice step pays one exp and one log latency instead of two of each.  All -inf -> -inf.
__device__ __forceinline__ float log_add_exp_fast3(float a, float b, float c) {
    const float m = fmaxf(a, fmaxf(b, c));
    if (m == -INFINITY) return -INFINITY;
    return m + __logf(__expf(a - m) + __expf(b - m) + __expf(c - m));
}
// the whole wave shifted by one lane on the VALU (DPP wave_shr:1 / wave_shl:1) instead of through the LDS crossbar of a
// ds_bpermute-based __shfl_up / __shfl_down; lane 0 (63) keeps `x` itself, like the shuffles
__device__ __forceinline__ float wave_up1(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, x), __builtin_bit_cast(int, x), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float wave_down1(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, x), __builtin_bit_cast(int, x), 0x130, 0xf, 0xf, false));
}

__device__ __forceinline__ int feature_length(long il, int ks, int stride, int pad, int T) {
    const float o = (float)(il + 2 * pad - ks);
    const int f = (int)floorf(o / (float)stride + 1.0f);          // float arithmetic like ha/rnn.py:13-18
    return max(0, min(f, T));
}

// row of accumulator element e of a 32x32 MFMA in lane (r, kh) = (lane & 31, lane >> 5); the column is r
__device__ __forceinline__ int acc_row(int e, int kh) { return (e & 3) + 8 * (e >> 2) + 4 * kh; }

// ---- the 32 x 32 classifier product on split-bf16 MFMA (v_mfma_f32_32x32x16_bf16; hi*hi + hi*lo + lo*hi), fragments straight from global
// memory in MFMA layout: logits[t][v] = sum_k feats[row0 + t][k] W[v][k] over nks 16-deep k-steps, rows of both operands H apart.  Wave w
// of the TNW takes k-steps w, w + 8, ..., two per pass; lane (r, kh) loads elements 8 kh .. 8 kh + 7 of row r of both operands.  Rows at
// and beyond nrows / V contribute zeros.  (ctc_head_train_kernel keeps its own copy over one K-slice, the dropout mask drawn under the loads) ----
__device__ __forceinline__ f32x16 head_logits_x3(const float *feats, long row0, int nrows, const float *w, int V, int H, int nks,
                                                 int wave, int r, int kh) {
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    const long frow = (row0 + min(r, nrows - 1)) * H, wrow = (long)min(r, V - 1) * H;
    for (int i0 = wave; i0 < nks; i0 += 2 * TNW) {
        f32x4 fa[2][2], wb[2][2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int kb = 16 * min(i0 + TNW * u, nks - 1) + 8 * kh;
            fa[u][0] = *reinterpret_cast<const f32x4 *>(feats + frow + kb);
            fa[u][1] = *reinterpret_cast<const f32x4 *>(feats + frow + kb + 4);
            wb[u][0] = *reinterpret_cast<const f32x4 *>(w + wrow + kb);
            wb[u][1] = *reinterpret_cast<const f32x4 *>(w + wrow + kb + 4);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const bool on = i0 + TNW * u < nks;
            float a8[8], b8[8];
            const bool arow = on && r < nrows, brow = on && r < V;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                a8[e] = arow ? fa[u][0][e] : 0.f; a8[4 + e] = arow ? fa[u][1][e] : 0.f;
                b8[e] = brow ? wb[u][0][e] : 0.f; b8[4 + e] = brow ? wb[u][1][e] : 0.f;
            }
            bf16x8 ahi, alo, bhi, blo;
            split8(a8, ahi, alo);
            split8(b8, bhi, blo);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ahi, blo, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(alo, bhi, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ahi, bhi, acc, 0, 0, 0);
        }
    }
    return acc;
}

// the TNW waves' accumulators -> red[wave][32 x 32]; after a barrier, element (tid >> 5) + 16 q, tid & 31 of the tile summed in wave order
__device__ __forceinline__ void head_put_acc(const f32x16 &acc, float *red, int wave, int r, int kh) {
#pragma unroll
    for (int e = 0; e < 16; ++e) red[wave * 1024 + acc_row(e, kh) * 32 + r] = acc[e];
}
__device__ __forceinline__ float head_sum_waves(const float *red, int q) {
    float sum = 0.f;
#pragma unroll
    for (int w = 0; w < TNW; ++w) sum += red[w * 1024 + threadIdx.x + TNT * q];
    return sum;
}

// reductions over the 32 lanes that hold one frame's classes
__device__ __forceinline__ float max32(float v) {
#pragma unroll
    for (int d = 16; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 32));
    return v;
}
__device__ __forceinline__ float sum32(float v) {
#pragma unroll
    for (int d = 16; d >= 1; d >>= 1) v += __shfl_xor(v, d, 32);
    return v;
}
// log-softmax over the classes, one class per lane: x is -inf in the lanes that hold no class (valid = false)
__device__ __forceinline__ float log_softmax32(float x, bool valid) {
    const float m = max32(x);
    const float s = sum32(valid ? expf(x - m) : 0.f);
    return x - m - logf(s);
}

// best class of frame t of a tile of log-probs: the first maximum, like torch.max
__device__ __forceinline__ int row_argmax(const float (*tile)[LDT], int t, int V, float &bv) {
    int best = 0;
    float m = tile[t][0];
    for (int c = 1; c < V; ++c) {
        const float v = tile[t][c];
        if (v > m) { m = v; best = c; }
    }
    bv = m;
    return best;
}
// greedy decode of utterance n in ONE wave, one lane per frame (T <= 32): best class and its log-prob per frame, then unique_consecutive +
// drop blanks, zero padded like the separate fill launch wrote it
__device__ __forceinline__ void greedy_collapse(const float (*tile)[LDT], int n, int T, int V, int lane, int64_t *ali, float *scores,
                                                int64_t *hyp, int64_t *hyp_len) {
    const int t = lane;
    int best = -1;
    float bv = -INFINITY;
    if (t < T) {
        best = row_argmax(tile, t, V, bv);
        ali[(long)n * T + t] = best;
        scores[(long)n * T + t] = bv;
    }
    int left = __shfl_up(best, 1, 64);
    if (lane == 0) left = -1;
    const bool keep = (t < T) && best != left && best != 0;
    const unsigned long long mask = __ballot(keep);
    const int pos = __popcll(mask & ((1ull << lane) - 1ull)), count = __popcll(mask);
    if (keep) hyp[(long)n * T + pos] = best;
    if (t < T && t >= count) hyp[(long)n * T + t] = 0;
    if (lane == 0) hyp_len[n] = count;
}

// ---- the loss ticket, called by one whole wave per utterance.  Lane 0 hands nll[n] to the workgroup that finishes last: write-through
// store, then also() (the utterance's other outputs of this launch), drained, then the ticket (Guideline 16 R1).  Returns whether this
// wave drew the last of the B tickets; that wave then calls loss_mean_last ----
template <class Also>
__device__ __forceinline__ bool loss_ticket(float *nll, int n, float out, unsigned *ticket, int B, int lane, Also also) {
    unsigned old = 0;
    if (lane == 0) {
        __hip_atomic_store(nll + n, out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        also();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        old = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    old = __builtin_amdgcn_readfirstlane(old);
    return old == (unsigned)B - 1u;
}
// reduction='mean' (ha/recognizer.py:71): mean_n(nll[n] / max(tl[n], 1)); the whole wave loads (one utterance per lane and pass), partial
// sums combine in a fixed order; the ticket is ready for the next call
__device__ __forceinline__ void loss_mean_last(const float *nll, const int64_t *tl, int B, float *loss, unsigned *ticket, int lane) {
    float s = 0.f;
    for (int i0 = 0; i0 < B; i0 += 64) {
        const int i = i0 + lane;
        float v = 0.f;
        if (i < B) v = __hip_atomic_load(nll + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) / fmaxf((float)tl[i], 1.0f);
        s += wave_sum(v);
    }
    if (lane == 0) {
        *loss = s / (float)B;
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- gradient at the log-probs in ATen's convention, on the hardware exp2/log2 forms (the wave kernel and the heads; ctc_beta_grad_kernel
// keeps libm and its own text) ----
// log-sum of row[s] (alpha + beta of one frame) over the states that emit class c
__device__ __forceinline__ float class_log_sum_fast(const float *row, const int64_t *tg, int states, int c) {
    float m = -INFINITY;
    if (c == 0) { for (int s = 0; s < states; s += 2) m = fmaxf(m, row[s]); }
    else        { for (int s = 1; s < states; s += 2) if ((int)tg[s >> 1] == c) m = fmaxf(m, row[s]); }
    float lcab = -INFINITY;
    if (m > -INFINITY) {
        float sum = 0.f;
        if (c == 0) { for (int s = 0; s < states; s += 2) sum += __expf(row[s] - m); }
        else        { for (int s = 1; s < states; s += 2) if ((int)tg[s >> 1] == c) sum += __expf(row[s] - m); }
        lcab = m + __logf(sum);
    }
    return lcab;
}
// l: the log-prob of (t, c); lcab: the class log-sum; go: the incoming gradient of the utterance's loss
__device__ __forceinline__ float grad_at_log_prob_fast(float l, float lcab, float nll, float go) {
    return (__expf(l) - __expf(lcab + nll - l)) * go;
}

}  // namespace
