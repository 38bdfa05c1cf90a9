// Beam search of the RNN transducer head (haloop_amd/transducer.py BeamDecoder): alignment-length synchronous decoding with exact
// merging ([Saon20]).  Every hypothesis of a row alive at alignment step i has consumed t frames and emitted u symbols with
// t + u = i, so hypotheses that spell the same tokens sit at the same frame and merge by logaddexp.  Per alignment step
//   1. rnnt_beam_step_kernel  one workgroup per row: the log-sum-exp of F[n, t_j] + g_j over V for each live hypothesis j, the blank and
//                             label candidates, the merge, the W best, the row's running W best complete hypotheses, the new beam's
//                             records, and (the gather) every new slot's [x | h_prev] rows and c from its parent's copy
//   2. one halo_rnnt_lstm_cell per LSTM layer and halo_decode_linear (out_layer) on all N * W slots (csrc/rnnt_decode.hip, csrc/decode.hip)
//   3. rnnt_beam_keep_kernel  a blank-extended slot takes (h, c, g) of its parent back
// The state (h and c of every layer, g) is double-buffered by step parity: launch 1 and 3 read the copy of this step, which no launch of
// the step writes, and write only the slots of their own row / their own slot of the other copy.  The rounds, the log-sum-exp, the token
// rows and the gather are beam_common.h's; every thread rescans its candidates in every round, and the merge compares tokens per thread.
// The row's W * V joint logits are kept in LDS when they are 32 KiB or less (the rounds then read LDS) and recomputed from L2 in every
// round otherwise.  Besides that LDS holds W-sized records only (< 1 KiB).
// The same search carried across calls (transducer.BeamStream) is a second instantiation of the step body,
// rnnt_beam_step_kernel<true>, entered from a beam kept in device memory, and rnnt_beam_stream_open_kernel, which opens a call.
#include <climits>
#include "halo_common.h"
#include "halo_internal.h"
#include "beam_common.h"

namespace {

using namespace beam;

struct RnntBeamArgs {
    const float *f;            // [N][T][V] transcription logits, strides f_rs (row) and f_ts (frame)
    long f_rs, f_ts;
    int T, V;
    const float *g, *g_bias;   // [N * W][ldg] prediction logits of every slot without their bias; the bias [V] (may be NULL)
    long ldg;
    const int *il;             // [N] frames of each row (clipped to [0, T] here)
    int step, W, capacity;
    const float *score_in;     // the beam this step reads: [N][W] scores, [N][W] symbols emitted (-1: no hypothesis), [N][W][tok_ld]
    const int *u_in, *tok_in;
    float *score_out;          // the beam it writes
    int *u_out, *tok_out;
    long tok_ld;
    int *parent, *last;        // [N][W] of the new beam: the parent's slot within the row (-1: no hypothesis), the new token (0: blank)
    float *fin_score;          // [N][W] the row's best complete hypotheses, unordered: score, order of appending, length (-1: none)
    int *fin_seq, *fin_len, *fin_tok, *fin_n;    // tokens [N][W][tok_ld]; fin_n [N]: hypotheses completed so far
    StateGather state;         // this step's state -> the cells' inputs
    int *live;                 // one word: += 1 per row whose new beam is not empty (carried: whose next step can be executed)
    int cached;                // the row's W V joint logits are kept in LDS (BEAM_LDS_FLOATS or fewer), else recomputed from L2
    // the carried search only (halo_rnnt_beam_step_stream): f is the rows' ring of `ring` frames, frame t at t % ring; the row's words
    int ring;
    int *step_w, *closed;      // [N] the row's alignment step; 1: its search is over (or it never began)
    const int *recv, *fin;     // [N] frames received so far; 1: no more frames follow
};

constexpr int BEAM_LDS_FLOATS = 8192;      // 32 KiB of dynamic LDS, under the 64 KiB a launch gets without the opt-in

// CARRIED: the search of transducer.BeamStream.  The step, the frames received R and the final / closed flags are the
// row's own words, f is a ring, and the records are always read (the open launch wrote the empty hypothesis).  A row executes its step
// iff its beam is not empty and max_j t_j + 1 < R or it is final (then L = R); every other row does an identity round.
template <bool CARRIED>
__global__ __launch_bounds__(BEAM_THREADS) void rnnt_beam_step_kernel(const RnntBeamArgs p) {
    __shared__ float s_score[BEAM_MAX], s_lse[BEAM_MAX], s_blank[BEAM_MAX], s_msc[BEAM_MAX], s_fsc[BEAM_MAX], sel_sc[BEAM_MAX];
    __shared__ int s_u[BEAM_MAX], s_mj[BEAM_MAX], s_mk[BEAM_MAX], s_nm[BEAM_MAX], s_fseq[BEAM_MAX], s_flen[BEAM_MAX], s_fsrc[BEAM_MAX],
        sel_pos[BEAM_MAX];
    __shared__ FirstScratch s_first;
    extern __shared__ float zs[];                                      // cached: z[j][v] = F[n, t_j, v] + (g_j[v] + bias[v])
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, W = p.W, V = p.V;
    const long base = (long)n * W;
    const int step = CARRIED ? p.step_w[n] : p.step;
    const bool first = !CARRIED && step == 0;                          // the records are not read: the beam is the empty hypothesis
    int L, R = 0;
    bool fin = false;
    if (CARRIED) {
        R = p.recv[n]; fin = p.fin[n] != 0;
        int umin = INT_MAX;                                            // the latest frame a hypothesis stands at is step - umin
        for (int j = 0; j < W; ++j) {
            const int u = p.u_in[base + j];
            if (u >= 0 && u <= p.capacity && u <= step) umin = min(umin, u);
        }
        if (umin == INT_MAX || p.closed[n] || !(fin || step - umin + 1 < R)) {
            // ---- the identity round of a row that stalls, is closed or has no beam: everything crosses to the other copy unchanged
            if (tid < W) {
                const int u = p.u_in[base + tid];
                p.score_out[base + tid] = p.score_in[base + tid]; p.u_out[base + tid] = u;
                p.parent[base + tid] = u >= 0 ? tid : -1; p.last[base + tid] = 0;
                s_mj[tid] = tid; s_mk[tid] = 0;
            }
            for (int idx = tid; idx < W * p.capacity; idx += BEAM_THREADS) {
                const long at = (base + idx / p.capacity) * p.tok_ld + idx % p.capacity;
                p.tok_out[at] = p.tok_in[at];
            }
            __syncthreads();
            gather_state(p.state, base, W, s_mj, s_mk);                // halo_rnnt_beam_keep then carries h, c and g across
            return;
        }
        L = fin ? R : R + 1;                                           // not final: both tests on L come out as for any L > R
    } else {
        L = min(max(p.il[n], 0), p.T);
    }
    if (tid < BEAM_MAX) {
        int u = -1;
        float sc = -INFINITY;
        if (tid < W) {
            if (first) {
                if (tid == 0 && L > 0) { u = 0; sc = 0.f; }            // the empty hypothesis
            } else {
                u = p.u_in[base + tid];
                sc = p.score_in[base + tid];
            }
            const int t = step - u;
            if (u < 0 || u > p.capacity || t < 0 || t >= L) u = -1;    // t < L holds under the host's loop; never read a frame past it
            if (first) {                                               // the row's finals: none, or the empty one of a row of no frames
                const bool empty = tid == 0 && L == 0;
                s_fsc[tid] = empty ? 0.f : -INFINITY; s_fseq[tid] = 0; s_flen[tid] = empty ? 0 : -1;
            } else {
                s_fsc[tid] = p.fin_score[base + tid]; s_fseq[tid] = p.fin_seq[base + tid]; s_flen[tid] = p.fin_len[base + tid];
            }
        }
        s_u[tid] = u; s_score[tid] = sc; s_mj[tid] = -1; s_nm[tid] = 0; s_fsrc[tid] = -1;
    }
    __syncthreads();
    // the joint logit of hypothesis j (live) at v: the same operations whether it is read back from LDS or recomputed, so the same bits
    auto logit = [&](int j, int v) {
        const int t = step - s_u[j];
        return p.f[(long)n * p.f_rs + (long)(CARRIED ? t % p.ring : t) * p.f_ts + v] + (p.g[(base + j) * p.ldg + v] + (p.g_bias ? p.g_bias[v] : 0.f));
    };
    auto z = [&](int j, int v) { return p.cached ? zs[j * V + v] : logit(j, v); };
    // ---- 1. wave w: log-sum-exp of hypotheses w, w + 4, ...
    for (int j = wave; j < W; j += BEAM_WAVES) {
        if (s_u[j] < 0) continue;
        const float lse = wave_lse(j, V, p.cached ? zs + j * V : nullptr, logit);
        if (lane == 0) {
            s_lse[j] = lse;
            s_blank[j] = s_score[j] + (z(j, 0) - lse);
        }
    }
    __syncthreads();
    // ---- 2. the merge: the blank extension of s and the extension of j by s's last token spell the same tokens when y_j = y_s[:-1]
    {
        const int s = tid / BEAM_MAX, j = tid % BEAM_MAX;
        if (s < W && j < W && s_u[s] >= 1 && s_u[j] == s_u[s] - 1 && step - s_u[s] + 1 < L) {
            const int *ts = p.tok_in + (base + s) * p.tok_ld, *tj = p.tok_in + (base + j) * p.tok_ld;
            bool eq = true;
            for (int x = 0; x < s_u[j]; ++x) eq = eq && ts[x] == tj[x];
            const int k = ts[s_u[s] - 1];
            if (eq && k >= 1 && k < V) {
                s_mj[s] = j; s_mk[s] = k;
                s_msc[s] = s_score[j] + (z(j, k) - s_lse[j]);
                atomicAdd(&s_nm[j], 1);                                // (an integer count: only zero / nonzero is used)
            }
        }
    }
    __syncthreads();
    if (tid < W && s_mj[tid] >= 0) s_blank[tid] = logaddexpf_(s_blank[tid], s_msc[tid]);
    // ---- 3. complete hypotheses (the blank at the row's last frame), in beam order, into the running W best: a later one displaces the
    //         worst kept (lowest score, the latest among equals) only with a strictly higher score
    if (tid == 0) {
        int cnt = first ? (L == 0 ? 1 : 0) : p.fin_n[n];
        bool any = first;
        for (int j = 0; j < W; ++j) {
            if (s_u[j] < 0 || step - s_u[j] + 1 != L) continue;
            const float sc = s_blank[j];
            int slot = -1;
            for (int w = 0; w < W && slot < 0; ++w) if (s_flen[w] < 0) slot = w;
            if (slot < 0) {
                int worst = 0;
                for (int w = 1; w < W; ++w)
                    if (s_fsc[w] < s_fsc[worst] || (s_fsc[w] == s_fsc[worst] && s_fseq[w] > s_fseq[worst])) worst = w;
                if (sc > s_fsc[worst]) slot = worst;
            }
            if (slot >= 0) { s_fsc[slot] = sc; s_fseq[slot] = cnt; s_flen[slot] = s_u[j]; s_fsrc[slot] = j; }
            cnt += 1; any = true;
        }
        if (any) p.fin_n[n] = cnt;
    }
    __syncthreads();
    if (tid < W && (first || s_fsrc[tid] >= 0)) {
        p.fin_score[base + tid] = s_fsc[tid]; p.fin_seq[base + tid] = s_fseq[tid]; p.fin_len[base + tid] = s_flen[tid];
    }
    for (int w = 0; w < W; ++w) {
        const int j = s_fsrc[w];
        if (j < 0) continue;
        for (int x = tid; x < s_u[j]; x += BEAM_THREADS) p.fin_tok[(base + w) * p.tok_ld + x] = p.tok_in[(base + j) * p.tok_ld + x];
    }
    // ---- 4. the W best candidates, one per round: the first in the order among those behind the last one taken.  Positions: the blank
    //         extension of j at j, the extension of j by k at W + j V + k.
    float psc = INFINITY;
    int ppos = -1, nsel = 0;
    for (int r = 0; r < W; ++r) {
        float bsc = -INFINITY;
        int bpos = NO_CANDIDATE;
        if (tid < W && s_u[tid] >= 0 && step - s_u[tid] + 1 != L) {
            const float sc = s_blank[tid];
            if (before(psc, ppos, sc, tid)) { bsc = sc; bpos = tid; }
        }
        for (int j = 0; j < W; ++j) {
            if (s_u[j] < 0 || s_u[j] >= p.capacity) continue;
            const float sj = s_score[j], lse = s_lse[j];
            const bool merged = s_nm[j] != 0;
            for (int k = 1 + tid; k < V; k += BEAM_THREADS) {
                const float sc = sj + (z(j, k) - lse);
                const int pos = W + j * V + k;
                if (!before(psc, ppos, sc, pos) || !before(sc, pos, bsc, bpos)) continue;
                if (merged) {
                    bool gone = false;
                    for (int s = 0; s < W; ++s) gone = gone || (s_mj[s] == j && s_mk[s] == k);
                    if (gone) continue;
                }
                bsc = sc; bpos = pos;
            }
        }
        first_in_workgroup(s_first, r, bsc, bpos);
        if (bpos == NO_CANDIDATE) break;                                // (uniform) no candidate is left
        if (tid == 0) { sel_sc[r] = bsc; sel_pos[r] = bpos; }
        psc = bsc; ppos = bpos; nsel = r + 1;
    }
    __syncthreads();
    // ---- 5. the new beam's records
    if (tid < W) {
        int par = -1, k = 0, u = -1;
        float sc = -INFINITY;
        if (tid < nsel) {
            const int pos = sel_pos[tid];
            par = pos < W ? pos : (pos - W) / V;
            k = pos < W ? 0 : (pos - W) % V;
            u = s_u[par] + (k != 0);
            sc = sel_sc[tid];
        }
        p.score_out[base + tid] = sc; p.u_out[base + tid] = u; p.parent[base + tid] = par; p.last[base + tid] = k;
        s_mj[tid] = par < 0 ? tid : par; s_mk[tid] = k;                 // (reused) the gather's source: a slot without a hypothesis takes its own
    }
    if (CARRIED && tid == 0) {                                         // (every thread read these words before the barriers above)
        p.step_w[n] = step + 1;
        if (nsel == 0 && fin) p.closed[n] = 1;                         // only a final row's beam runs empty: its search is over
    }
    if (nsel == 0) return;
    __syncthreads();
    if (tid == 0) {
        bool live = true;
        if (CARRIED && !fin) {                                         // the stall rule on the new beam at the next step
            int umin = INT_MAX;
            for (int r = 0; r < nsel; ++r) umin = min(umin, s_u[s_mj[r]] + (s_mk[r] != 0));
            live = step + 1 - umin + 1 < R;
        }
        if (live) atomicAdd(p.live, 1);
    }
    // up < capacity where a label is taken: only such hypotheses take labels
    child_rows(p.tok_out + base * p.tok_ld, p.tok_in + base * p.tok_ld, p.tok_ld, nsel, p.capacity, s_mj, s_u, s_mk,
               [&](int r, int) { return s_mk[r] != 0; });
    // ---- 6. the gather: every new slot's cell inputs and c from its parent's
    gather_state(p.state, base, W, s_mj, s_mk);
}

struct RnntKeepArgs {
    int W, V, H, layers;
    long slots, ldg;
    const int *parent, *last;
    const float *h_in, *c_in, *g_in;
    float *h_out, *c_out, *g_out;
};

// one workgroup per slot: a blank-extended hypothesis keeps its parent's state (the cells and out_layer ran on every slot)
__global__ __launch_bounds__(BEAM_THREADS) void rnnt_beam_keep_kernel(const RnntKeepArgs p) {
    const long slot = blockIdx.x;
    const int par = p.parent[slot];
    if (par < 0 || par >= p.W || p.last[slot] != 0) return;
    const long src = slot / p.W * p.W + par;
    const int H4 = p.H / 4;
    for (int l = 0; l < p.layers; ++l) {
        const f32x4 *hs = reinterpret_cast<const f32x4 *>(p.h_in + ((long)l * p.slots + src) * p.H);
        const f32x4 *cs = reinterpret_cast<const f32x4 *>(p.c_in + ((long)l * p.slots + src) * p.H);
        f32x4 *hd = reinterpret_cast<f32x4 *>(p.h_out + ((long)l * p.slots + slot) * p.H);
        f32x4 *cd = reinterpret_cast<f32x4 *>(p.c_out + ((long)l * p.slots + slot) * p.H);
        for (int x = threadIdx.x; x < H4; x += BEAM_THREADS) { hd[x] = hs[x]; cd[x] = cs[x]; }
    }
    for (int v = threadIdx.x; v < p.V; v += BEAM_THREADS) p.g_out[slot * p.ldg + v] = p.g_in[src * p.ldg + v];
}

// ---- opening a call of the carried search: one workgroup per row of the state (rows >= B take no part in the call)
struct RnntBeamOpenArgs {
    const float *f;            // [B][S][V] this call's logits, strides f_rs and f_ts
    long f_rs, f_ts;
    int B, S, V;
    const int *n_frames, *flags;   // [B]; flags may be NULL: bit 1 begin, bit 2 final (include/halo.h)
    float *ring;               // [rows][ring_n][V]
    int ring_n;
    int *step_w, *recv, *fin, *closed;
    int W;
    float *score;              // the records of the copy the next step reads: [rows][W]
    int *u;
    float *fin_score;          // the finals
    int *fin_seq, *fin_len, *fin_n;
    const float *h0, *c0, *g0; // the state after the zero prefix: [L][H], [L][H], [V]
    float *h, *c, *g;          // the copy the next step reads: [L][rows W][H] twice, [rows W][ldg]
    long ldg;
    int H, L;
    int *live, n_live;         // the call's live words, zeroed here
};

constexpr int STREAM_FLAG_BEGIN = 2, STREAM_FLAG_FINAL = 4;

__global__ __launch_bounds__(BEAM_THREADS) void rnnt_beam_stream_open_kernel(const RnntBeamOpenArgs p) {
    const int n = blockIdx.x, tid = threadIdx.x, W = p.W;
    if (n == 0)
        for (int i = tid; i < p.n_live; i += BEAM_THREADS) p.live[i] = 0;
    if (n >= p.B) return;
    const long base = (long)n * W, slots = (long)gridDim.x * W;
    const int flags = p.flags ? p.flags[n] : 0;
    const bool begin = flags & STREAM_FLAG_BEGIN;
    int R = p.recv[n], fin = p.fin[n], closed = p.closed[n];
    if (begin) {                                                       // the empty hypothesis on the state of the zero prefix, no finals
        R = 0; fin = 0; closed = 0;
        if (tid < W) {
            p.score[base + tid] = tid == 0 ? 0.f : -INFINITY; p.u[base + tid] = tid == 0 ? 0 : -1;
            p.fin_score[base + tid] = -INFINITY; p.fin_seq[base + tid] = 0; p.fin_len[base + tid] = -1;
        }
        for (int i = tid; i < p.L * p.H; i += BEAM_THREADS) {
            const long at = ((long)(i / p.H) * slots + base) * p.H + i % p.H;
            p.h[at] = p.h0[i]; p.c[at] = p.c0[i];
        }
        for (int v = tid; v < p.V; v += BEAM_THREADS) p.g[base * p.ldg + v] = p.g0[v];
    } else if (closed || fin) {
        return;                                                        // frames sent to a closed row change nothing
    }
    const int nf = min(max(p.n_frames[n], 0), p.S);
    for (int i = tid; i < nf * p.V; i += BEAM_THREADS) {
        const int s = i / p.V, v = i % p.V;
        p.ring[((long)n * p.ring_n + (R + s) % p.ring_n) * p.V + v] = p.f[(long)n * p.f_rs + (long)s * p.f_ts + v];
    }
    __syncthreads();                                                   // every thread has read the row's words
    if (tid != 0) return;
    R += nf;
    if (flags & STREAM_FLAG_FINAL) {
        fin = 1;
        if (R == 0) {                                                  // an utterance of no frames: the empty hypothesis is its one final
            p.score[base] = -INFINITY; p.u[base] = -1;
            p.fin_score[base] = 0.f; p.fin_seq[base] = 0; p.fin_len[base] = 0;
            closed = 1;
        }
    }
    if (begin) { p.step_w[n] = 0; p.fin_n[n] = 0; }
    if (closed) p.fin_n[n] = 1;
    p.recv[n] = R; p.fin[n] = fin; p.closed[n] = closed;
}

int step_launch(RnntBeamArgs &p, bool carried, int N, halo_stream_t stream) {
    p.cached = (long)p.W * p.V <= BEAM_LDS_FLOATS;
    const size_t lds = p.cached ? (size_t)p.W * p.V * sizeof(float) : 0;
    if (carried) hipLaunchKernelGGL(rnnt_beam_step_kernel<true>, dim3((unsigned)N), dim3(BEAM_THREADS), lds, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(rnnt_beam_step_kernel<false>, dim3((unsigned)N), dim3(BEAM_THREADS), lds, (hipStream_t)stream, p);
    return halo_launch_status();
}

}  // namespace

extern "C" {

int halo_rnnt_beam_step(const float *f, long f_row_stride, long f_frame_stride, int N, int T, int V, const float *g, long ldg,
                        const float *g_bias, const int *input_lengths, int step, int beam, int capacity, const float *scores_in,
                        const int *u_in, const int *tokens_in, float *scores_out, int *u_out, int *tokens_out, long tokens_ld,
                        int *parent, int *last, float *fin_scores, int *fin_seq, int *fin_lengths, int *fin_tokens, int *fin_n,
                        const float *wte, int hidden, int layers, const float *h_in, const float *c_in, float *xh, float *c_out,
                        int *live, halo_stream_t stream) {
    HALO_CHECK_ARG(f && g && input_lengths && scores_in && u_in && tokens_in && scores_out && u_out && tokens_out && parent && last);
    HALO_CHECK_ARG(fin_scores && fin_seq && fin_lengths && fin_tokens && fin_n && wte && h_in && c_in && xh && c_out && live);
    HALO_CHECK_ARG(N > 0 && T > 0 && V > 0 && V <= 8192 && capacity > 0 && step >= 0 && beam >= 1 && beam <= BEAM_MAX);
    HALO_CHECK_ARG(f_frame_stride >= V && f_row_stride >= (long)(T - 1) * f_frame_stride + V && ldg >= V && tokens_ld >= capacity);
    HALO_CHECK_ARG(hidden > 0 && hidden % 4 == 0 && layers > 0);
    HALO_CHECK_ARG(((uintptr_t)wte | (uintptr_t)h_in | (uintptr_t)c_in | (uintptr_t)xh | (uintptr_t)c_out) % 16 == 0);
    HALO_CHECK_ARG(scores_in != scores_out && u_in != u_out && tokens_in != tokens_out && h_in != xh && c_in != c_out);
    RnntBeamArgs p;
    p.f = f; p.f_rs = f_row_stride; p.f_ts = f_frame_stride; p.T = T; p.V = V; p.g = g; p.g_bias = g_bias; p.ldg = ldg;
    p.il = input_lengths; p.step = step; p.W = beam; p.capacity = capacity; p.score_in = scores_in; p.u_in = u_in; p.tok_in = tokens_in;
    p.score_out = scores_out; p.u_out = u_out; p.tok_out = tokens_out; p.tok_ld = tokens_ld; p.parent = parent; p.last = last;
    p.fin_score = fin_scores; p.fin_seq = fin_seq; p.fin_len = fin_lengths; p.fin_tok = fin_tokens; p.fin_n = fin_n;
    p.state = {wte, h_in, c_in, xh, c_out, hidden, layers}; p.live = live;
    p.ring = 0; p.step_w = nullptr; p.closed = nullptr; p.recv = nullptr; p.fin = nullptr;
    return step_launch(p, false, N, stream);
}

int halo_rnnt_beam_step_stream(const float *ring, int ring_frames, int rows, int V, const float *g, long ldg, const float *g_bias,
                               int *stream_state, long state_ld, int beam, int capacity, const float *scores_in, const int *u_in,
                               const int *tokens_in, float *scores_out, int *u_out, int *tokens_out, long tokens_ld, int *parent,
                               int *last, float *fin_scores, int *fin_seq, int *fin_lengths, int *fin_tokens, int *fin_n,
                               const float *wte, int hidden, int layers, const float *h_in, const float *c_in, float *xh, float *c_out,
                               int *live, halo_stream_t stream) {
    HALO_CHECK_ARG(ring && g && stream_state && scores_in && u_in && tokens_in && scores_out && u_out && tokens_out && parent && last);
    HALO_CHECK_ARG(fin_scores && fin_seq && fin_lengths && fin_tokens && fin_n && wte && h_in && c_in && xh && c_out && live);
    HALO_CHECK_ARG(rows > 0 && ring_frames > 0 && V > 0 && V <= 8192 && capacity > 0 && beam >= 1 && beam <= BEAM_MAX);
    HALO_CHECK_ARG(ldg >= V && tokens_ld >= capacity && state_ld >= rows && hidden > 0 && hidden % 4 == 0 && layers > 0);
    HALO_CHECK_ARG(((uintptr_t)wte | (uintptr_t)h_in | (uintptr_t)c_in | (uintptr_t)xh | (uintptr_t)c_out) % 16 == 0);
    HALO_CHECK_ARG(scores_in != scores_out && u_in != u_out && tokens_in != tokens_out && h_in != xh && c_in != c_out);
    RnntBeamArgs p;
    p.f = ring; p.f_rs = (long)ring_frames * V; p.f_ts = V; p.T = 0; p.V = V; p.g = g; p.g_bias = g_bias; p.ldg = ldg;
    p.il = nullptr; p.step = 0; p.W = beam; p.capacity = capacity; p.score_in = scores_in; p.u_in = u_in; p.tok_in = tokens_in;
    p.score_out = scores_out; p.u_out = u_out; p.tok_out = tokens_out; p.tok_ld = tokens_ld; p.parent = parent; p.last = last;
    p.fin_score = fin_scores; p.fin_seq = fin_seq; p.fin_len = fin_lengths; p.fin_tok = fin_tokens; p.fin_n = fin_n;
    p.state = {wte, h_in, c_in, xh, c_out, hidden, layers}; p.live = live;
    p.ring = ring_frames; p.step_w = stream_state; p.recv = stream_state + state_ld; p.fin = stream_state + 2 * state_ld;
    p.closed = stream_state + 3 * state_ld;
    return step_launch(p, true, rows, stream);
}

int halo_rnnt_beam_stream_open(const float *f, long f_row_stride, long f_frame_stride, int B, int S, int V, const int *n_frames,
                               const int *flags, int rows, float *ring, int ring_frames, int *stream_state, long state_ld, int beam,
                               float *scores, int *u, float *fin_scores, int *fin_seq, int *fin_lengths, int *fin_n, const float *h0,
                               const float *c0, const float *g0, float *h, float *c, float *g, long ldg, int hidden, int layers,
                               int *live, int n_live, halo_stream_t stream) {
    HALO_CHECK_ARG(f && n_frames && ring && stream_state && scores && u && fin_scores && fin_seq && fin_lengths && fin_n);
    HALO_CHECK_ARG(h0 && c0 && g0 && h && c && g && live && n_live >= 0);
    HALO_CHECK_ARG(B > 0 && rows >= B && S > 0 && V > 0 && ring_frames >= S && state_ld >= rows && beam >= 1 && beam <= BEAM_MAX);
    HALO_CHECK_ARG(f_frame_stride >= V && f_row_stride >= (long)(S - 1) * f_frame_stride + V && ldg >= V && hidden > 0 && layers > 0);
    RnntBeamOpenArgs p;
    p.f = f; p.f_rs = f_row_stride; p.f_ts = f_frame_stride; p.B = B; p.S = S; p.V = V; p.n_frames = n_frames; p.flags = flags;
    p.ring = ring; p.ring_n = ring_frames; p.step_w = stream_state; p.recv = stream_state + state_ld; p.fin = stream_state + 2 * state_ld;
    p.closed = stream_state + 3 * state_ld; p.W = beam; p.score = scores; p.u = u; p.fin_score = fin_scores; p.fin_seq = fin_seq;
    p.fin_len = fin_lengths; p.fin_n = fin_n; p.h0 = h0; p.c0 = c0; p.g0 = g0; p.h = h; p.c = c; p.g = g; p.ldg = ldg; p.H = hidden;
    p.L = layers; p.live = live; p.n_live = n_live;
    hipLaunchKernelGGL(rnnt_beam_stream_open_kernel, dim3((unsigned)rows), dim3(BEAM_THREADS), 0, (hipStream_t)stream, p);
    return halo_launch_status();
}

int halo_rnnt_beam_keep(int slots, int beam, int V, int hidden, int layers, const int *parent, const int *last, const float *h_in,
                        const float *c_in, const float *g_in, long ldg, float *h_out, float *c_out, float *g_out, halo_stream_t stream) {
    HALO_CHECK_ARG(parent && last && h_in && c_in && g_in && h_out && c_out && g_out);
    HALO_CHECK_ARG(slots > 0 && beam >= 1 && beam <= BEAM_MAX && slots % beam == 0 && V > 0 && ldg >= V && hidden > 0 && hidden % 4 == 0);
    HALO_CHECK_ARG(layers > 0 && ((uintptr_t)h_in | (uintptr_t)c_in | (uintptr_t)h_out | (uintptr_t)c_out) % 16 == 0);
    HALO_CHECK_ARG(h_in != h_out && c_in != c_out && g_in != g_out);
    RnntKeepArgs p;
    p.W = beam; p.V = V; p.H = hidden; p.layers = layers; p.slots = slots; p.ldg = ldg; p.parent = parent; p.last = last;
    p.h_in = h_in; p.c_in = c_in; p.g_in = g_in; p.h_out = h_out; p.c_out = c_out; p.g_out = g_out;
    hipLaunchKernelGGL(rnnt_beam_keep_kernel, dim3((unsigned)slots), dim3(BEAM_THREADS), 0, (hipStream_t)stream, p);
    return halo_launch_status();
}

}  // extern "C"
