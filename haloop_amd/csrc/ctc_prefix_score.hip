// CTC prefix scores for the joint CTC/attention beam search (haloop_amd/transformer.py BeamDecoder with ctc_log_probs; the
// definition: include/halo.h).  A live slot with prefix g carries r[t][2], t < T_n: the log-mass of the CTC paths over frames 0 .. t that
// spell exactly g and end in a non-blank (r[t][0]) or in a blank (r[t][1]).
//   ctc_prefix_scores_kernel   psi(g, k) for every class k of every live slot from g's state alone: one workgroup per (slot, CLASSES
//                              classes), CLASSES = 64, or 32 when V <= 32; both[] = logaddexp(r[.][0], r[.][1]) and r[.][1] of the slot
//                              are built once in LDS, a thread is (class, one of 256 / CLASSES frame partitions), so a wave's loads of
//                              x[n][t][.] are contiguous over classes; per partition a max pass and a sum pass, the partitions combined
//                              in ascending order, one log per (slot, class).
//   ctc_prefix_advance_kernel  the state of g.k from g's: one wave per kept slot.  The recurrence is a serial chain over the frames; the
//                              wave loads 64 frames' operands at once (lane = frame), walks the chain on values read lane by lane
//                              (v_readlane; the two log-sum-exps of a frame on the hardware exp2 / log2, whose absolute error in
//                              log(1 + e), e <= 1, is below the rounding of the sums they feed), and stores the 64 results at once.
// fp32 in every arithmetic mode, no atomics, every sum in one order.  Frames t >= T_n of x and of the states are neither read nor written.
#include "halo_common.h"
#include "halo_internal.h"

namespace {

constexpr int PS_THREADS = 256;
constexpr int PS_MAX_S = 4096, PS_MAX_V = 8192, PS_MAX_W = 16;      // two rows of S floats: 32 KiB of LDS, under the 64 KiB without the opt-in

__device__ __forceinline__ float logaddexp(float a, float b) {
    const float m = fmaxf(a, b);
    if (!(m > -INFINITY)) return -INFINITY;
    return m + log1pf(expf(-fabsf(a - b)));
}

// the chain's form: v_exp_f32 / v_log_f32
__device__ __forceinline__ float logaddexp_chain(float a, float b) {
    const float m = fmaxf(a, b);
    if (!(m > -INFINITY)) return -INFINITY;
    return m + __logf(1.0f + __expf(-fabsf(a - b)));
}

__device__ __forceinline__ float read_lane(float v, int lane) {      // lane: the same in every lane
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

struct PrefixScoreArgs {
    const float *x;            // [N][S][V] log-probabilities, unit class stride
    long x_ns, x_ts;
    const int *lens;           // [N]
    const float *state;        // [N * W][S][2]
    const int *last, *len, *fin;       // [N * W]: the beam's records, as the selection reads them (not read at t == 0)
    const float *score;
    int S, V, W, t, etx;
    float *psi;                // [N * W][psi_ld]
    long psi_ld;
};

template <int PS_CLASSES>
__global__ __launch_bounds__(PS_THREADS) void ctc_prefix_scores_kernel(const PrefixScoreArgs p) {
    constexpr int PS_PARTS = PS_THREADS / PS_CLASSES;
    extern __shared__ float ps_rows[];                                 // both[T] | r[.][1][T]
    __shared__ float s_max[PS_PARTS][PS_CLASSES], s_sum[PS_PARTS][PS_CLASSES];
    const int slot = blockIdx.x, n = slot / p.W, tid = threadIdx.x;
    const int kc = tid % PS_CLASSES, part = tid / PS_CLASSES, k = blockIdx.y * PS_CLASSES + kc;
    const int T = min(max(p.lens[n], 0), p.S);
    bool live;
    int len = 0, last = -1;
    if (p.t == 0) {                                                    // the records are not read: slot 0 holds the empty prefix
        live = slot % p.W == 0;
    } else {
        len = p.len[slot];
        live = p.score[slot] > -INFINITY && !p.fin[slot] && len >= 0 && len <= p.t;
        if (live && len > 0) last = p.last[slot];
    }
    float *out = p.psi + (long)slot * p.psi_ld;
    if (!live || T == 0) {                                             // (uniform) empty and finished slots: no candidate
        if (part == 0 && k < p.V) out[k] = -INFINITY;
        return;
    }
    float *both = ps_rows, *rb = ps_rows + T;
    const float2 *st = reinterpret_cast<const float2 *>(p.state + (long)slot * p.S * 2);
    for (int t = tid; t < T; t += PS_THREADS) {
        const float2 r = st[t];
        both[t] = logaddexp(r.x, r.y);
        rb[t] = r.y;
    }
    __syncthreads();
    // frames 1 .. T - 1 in PS_PARTS contiguous stretches; partition 0 also holds the term x[0][k] of the empty prefix
    const int chunk = (T - 1 + PS_PARTS - 1) / PS_PARTS, t0 = 1 + part * chunk, t1 = min(T, t0 + chunk);
    const bool label = k < p.V && k != 0 && k != p.etx;
    const float *phi = k == last ? rb : both;
    const float *xk = p.x + (long)n * p.x_ns + k;
    const bool first = part == 0 && len == 0;
    float m = -INFINITY;
    if (label) {
        for (int t = t0; t < t1; ++t) m = fmaxf(m, phi[t - 1] + xk[(long)t * p.x_ts]);
        if (first) m = fmaxf(m, xk[0]);
    }
    s_max[part][kc] = m;
    __syncthreads();
    float gm = s_max[0][kc];
#pragma unroll
    for (int q = 1; q < PS_PARTS; ++q) gm = fmaxf(gm, s_max[q][kc]);
    float s = 0.f;
    if (label && gm > -INFINITY) {
        for (int t = t0; t < t1; ++t) s += expf(phi[t - 1] + xk[(long)t * p.x_ts] - gm);
        if (first) s += expf(xk[0] - gm);
    }
    s_sum[part][kc] = s;
    __syncthreads();
    if (part != 0 || k >= p.V) return;
    float v = -INFINITY;
    if (k == p.etx) {
        v = both[T - 1];                                               // the whole utterance spells exactly g
    } else if (label && gm > -INFINITY) {
        float tot = s_sum[0][kc];
#pragma unroll
        for (int q = 1; q < PS_PARTS; ++q) tot += s_sum[q][kc];
        v = gm + logf(tot);
    }
    out[k] = v;
}

struct PrefixAdvanceArgs {
    const float *x;
    long x_ns, x_ts;
    const int *lens;
    const float *in;           // [N * W][S][2]: the beam the selection read
    float *out;                // [N * W][S][2]: the beam it wrote
    const int *parents;        // [N * W] (NULL: the empty prefix's state into slot 0 of every utterance)
    const int *last_new, *len_new, *last_prev;
    int S, V, W, etx;
};

__global__ __launch_bounds__(HALO_WAVE) void ctc_prefix_advance_kernel(const PrefixAdvanceArgs p) {
    const int slot = blockIdx.x, n = slot / p.W, lane = threadIdx.x;
    const bool init = !p.parents;
    int par = 0, k = 0;
    bool empty_g = false, same = false;
    if (init) {
        if (slot % p.W) return;
    } else {
        par = p.parents[slot];
        k = p.last_new[slot];
        if (par < 0 || par >= p.W || k <= 0 || k >= p.V || k == p.etx) return;          // finished and empty slots need no state
        empty_g = p.len_new[slot] <= 1;
        same = !empty_g && p.last_prev[n * p.W + par] == k;
    }
    const int T = min(max(p.lens[n], 0), p.S);
    const float *xb = p.x + (long)n * p.x_ns;
    const float2 *in = reinterpret_cast<const float2 *>(p.in + ((long)n * p.W + par) * p.S * 2);
    float2 *out = reinterpret_cast<float2 *>(p.out + (long)slot * p.S * 2);
    float q0 = -INFINITY, q1 = -INFINITY;                               // the chain: the same values in every lane
    for (int t0 = 0; t0 < T; t0 += HALO_WAVE) {
        const int t = t0 + lane;
        float xk = 0.f, x0 = 0.f, ph = -INFINITY;
        if (t < T) {
            x0 = xb[(long)t * p.x_ts];
            if (!init) {
                xk = xb[(long)t * p.x_ts + k];
                if (t >= 1) {
                    const float2 r = in[t - 1];
                    ph = same ? r.y : logaddexp(r.x, r.y);
                }
            }
        }
        float my0 = -INFINITY, my1 = -INFINITY;
        const int cnt = min(HALO_WAVE, T - t0);
        for (int i = 0; i < cnt; ++i) {
            const float xki = read_lane(xk, i), x0i = read_lane(x0, i), phi = read_lane(ph, i);
            float n0, n1;
            if (init) {
                n0 = -INFINITY;
                n1 = t0 + i == 0 ? x0i : q1 + x0i;
            } else if (t0 + i == 0) {
                n0 = empty_g ? xki : -INFINITY;
                n1 = -INFINITY;
            } else {
                n0 = logaddexp_chain(q0, phi) + xki;
                n1 = logaddexp_chain(q0, q1) + x0i;
            }
            q0 = n0; q1 = n1;
            if (lane == i) { my0 = n0; my1 = n1; }
        }
        if (t < T) out[t] = make_float2(my0, my1);
    }
}

}  // namespace

extern "C" {

int halo_ctc_prefix_scores(const float *log_probs, long batch_stride, long frame_stride, int N, int beam, int S, int V,
                           const int *input_lengths, const float *states, const int *last_tokens, const int *lengths, const float *scores,
                           const int *finished, int t, int etx, float *psi_cand, long psi_ld, halo_stream_t stream) {
    HALO_CHECK_ARG(log_probs && input_lengths && states && psi_cand && N > 0 && beam >= 1 && S > 0 && V > 0 && t >= 0);
    HALO_CHECK_ARG(t == 0 || (last_tokens && lengths && scores && finished));
    HALO_CHECK_ARG(etx > 0 && etx < V && psi_ld >= V && frame_stride >= V && batch_stride >= (long)(S - 1) * frame_stride + V);
    HALO_CHECK_ARG((uintptr_t)states % 8 == 0 && (long)N * beam <= 0x7fffffffL);
    if (S > PS_MAX_S || V > PS_MAX_V || beam > PS_MAX_W) return HALO_ENOTSUP;
    PrefixScoreArgs p;
    p.x = log_probs; p.x_ns = batch_stride; p.x_ts = frame_stride; p.lens = input_lengths; p.state = states;
    p.last = last_tokens; p.len = lengths; p.fin = finished; p.score = scores;
    p.S = S; p.V = V; p.W = beam; p.t = t; p.etx = etx; p.psi = psi_cand; p.psi_ld = psi_ld;
    const size_t lds = (size_t)2 * S * sizeof(float);
    if (V <= 32)
        hipLaunchKernelGGL(ctc_prefix_scores_kernel<32>, dim3((unsigned)(N * beam)), dim3(PS_THREADS), lds, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(ctc_prefix_scores_kernel<64>, dim3((unsigned)(N * beam), (unsigned)((V + 63) / 64)), dim3(PS_THREADS), lds,
                           (hipStream_t)stream, p);
    return halo_launch_status();
}

int halo_ctc_prefix_advance(const float *log_probs, long batch_stride, long frame_stride, int N, int beam, int S, int V,
                            const int *input_lengths, int etx, const float *states_in, float *states_out, const int *parents,
                            const int *last_tokens_new, const int *lengths_new, const int *last_tokens_prev, halo_stream_t stream) {
    HALO_CHECK_ARG(log_probs && input_lengths && states_out && N > 0 && beam >= 1 && S > 0 && V > 0);
    HALO_CHECK_ARG(!parents || (states_in && last_tokens_new && lengths_new && last_tokens_prev && states_in != states_out));
    HALO_CHECK_ARG(etx > 0 && etx < V && frame_stride >= V && batch_stride >= (long)(S - 1) * frame_stride + V);
    HALO_CHECK_ARG(((uintptr_t)states_in | (uintptr_t)states_out) % 8 == 0 && (long)N * beam <= 0x7fffffffL);
    if (S > PS_MAX_S || V > PS_MAX_V || beam > PS_MAX_W) return HALO_ENOTSUP;
    PrefixAdvanceArgs p;
    p.x = log_probs; p.x_ns = batch_stride; p.x_ts = frame_stride; p.lens = input_lengths; p.in = states_in; p.out = states_out;
    p.parents = parents; p.last_new = last_tokens_new; p.len_new = lengths_new; p.last_prev = last_tokens_prev;
    p.S = S; p.V = V; p.W = beam; p.etx = etx;
    hipLaunchKernelGGL(ctc_prefix_advance_kernel, dim3((unsigned)(N * beam)), dim3(HALO_WAVE), 0, (hipStream_t)stream, p);
    return halo_launch_status();
}

}  // extern "C"
