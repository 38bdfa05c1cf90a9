// Beam search of the RNN transducer head with shallow fusion of an LSTM language model (haloop_amd/fusion.py TransducerFusionDecoder;
// DESIGN.md 3.3z; the definition in include/halo.h): the alignment-length synchronous search of csrc/rnnt_beam.hip with every candidate
// ranked by fma(a, lm', s') + b len(y'), s' its transducer mass and lm' the LM's log-probability of its tokens.  Slot n W + j carries two
// recurrent states: the prediction network's (g: its logits) and the LM's (lg: its logits).  Per alignment step
//   1. rnnt_lm_beam_step_kernel  one workgroup per row: both log-sum-exps of every live hypothesis, the blank and label candidates, the
//                                merge (masses only: the blank extension keeps its own lm), the W best by rank, the row's running W best
//                                complete hypotheses, the new beam's records s | lm | rank, and both gathers
//   2. one halo_rnnt_lstm_cell per layer of each network and one halo_decode_linear per out_layer on all N * W slots
//   3. halo_rnnt_beam_keep once per network: a blank-extended slot takes (h, c, logits) of its parent back
// so Lp + Ll + 5 launches.  The pieces are beam_common.h's; a thread owns the blank candidate tid and the label candidates of its classes
// and keeps the first of them behind the last one taken (csrc/ctc_lm_beam.hip's rounds).
// LDS: the row's W V joint logits and W V LM logits are both kept in dynamic LDS when 2 W V <= LDS_FLOATS (56 KiB at most, under the
// 64 KiB a launch gets without the opt-in) and both recomputed from L2 by the same operations otherwise: the same bits.  Besides that
// LDS holds W-sized records only (< 2 KiB static).
#include "halo_common.h"
#include "halo_internal.h"
#include "beam_common.h"

namespace {

using namespace beam;

constexpr int LDS_FLOATS = 14336;          // 56 KiB of dynamic LDS, as csrc/ctc_lm_beam.hip

struct RnntLmBeamArgs {
    const float *f;            // [N][T][V] transcription logits, strides f_rs (row) and f_ts (frame)
    long f_rs, f_ts;
    int T, V;
    const float *g, *g_bias;   // [N * W][ldg] prediction logits of every slot without their bias; the bias [V] (may be NULL)
    long ldg;
    const float *lg, *lg_bias; // [N * W][ldlg] LM logits of every slot without their bias; the bias [V] (may be NULL)
    long ldlg;
    const int *il;             // [N] frames of each row (clipped to [0, T] here)
    int step, W, capacity;
    float a, b;                // lm_weight, insertion_bonus
    const float *rec_in;       // the beam this step reads: [N][W][3] s | lm | rank, [N][W] symbols emitted (-1: no hypothesis), tokens
    const int *u_in, *tok_in;
    float *rec_out;            // the beam it writes
    int *u_out, *tok_out;
    long tok_ld;
    int *parent, *last;        // [N][W] of the new beam: the parent's slot within the row (-1: no hypothesis), the new token (0: blank)
    float *fin_rec;            // [N][W][3] rank | s | lm of the row's best complete hypotheses, unordered
    int *fin_seq, *fin_len, *fin_tok, *fin_n;    // order of appending, length (-1: none), tokens [N][W][tok_ld]; fin_n [N]: completed so far
    StateGather state, lm_state;   // this step's states -> the cells' inputs, per network
    int *live;                 // one word: += 1 per row whose new beam is not empty
    int cached;                // both tables of the row are kept in LDS, else recomputed from L2
};

__global__ __launch_bounds__(BEAM_THREADS) void rnnt_lm_beam_step_kernel(const RnntLmBeamArgs p) {
    // the beam read: mass, LM score, symbols; the step: both log-sum-exps, the blank candidates' masses, a label's bonus, the merge
    // (the member whose extension by s_mk merged into s, its mass, whether an extension of j was merged away); the finals; the new beam
    __shared__ float s_score[BEAM_MAX], s_lm[BEAM_MAX], s_lse[BEAM_MAX], s_llse[BEAM_MAX], s_blank[BEAM_MAX], s_msc[BEAM_MAX], s_bl[BEAM_MAX],
        s_frk[BEAM_MAX], s_fs[BEAM_MAX], s_flm[BEAM_MAX], sel_sc[BEAM_MAX];
    __shared__ int s_u[BEAM_MAX], s_mj[BEAM_MAX], s_mk[BEAM_MAX], s_nm[BEAM_MAX], s_fseq[BEAM_MAX], s_flen[BEAM_MAX], s_fsrc[BEAM_MAX],
        sel_pos[BEAM_MAX], s_src[BEAM_MAX], s_k[BEAM_MAX];
    __shared__ FirstScratch s_first;
    extern __shared__ float dyn[];                                     // cached: z[j][v] joint logits | zl[j][v] LM logits
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, W = p.W, V = p.V;
    const long base = (long)n * W;
    const int L = min(max(p.il[n], 0), p.T);
    float *zs = dyn, *zls = dyn + W * V;
    if (tid < BEAM_MAX) {
        int u = -1;
        float sc = -INFINITY, lm = -INFINITY;
        if (tid < W) {
            if (p.step == 0) {
                if (tid == 0 && L > 0) { u = 0; sc = 0.f; lm = 0.f; }  // the empty hypothesis
            } else {
                u = p.u_in[base + tid];
                sc = p.rec_in[(base + tid) * 3]; lm = p.rec_in[(base + tid) * 3 + 1];
            }
            const int t = p.step - u;
            if (u < 0 || u > p.capacity || t < 0 || t >= L) u = -1;    // t < L holds under the host's loop; never read a frame past it
            if (p.step == 0) {                                         // the row's finals: none, or the empty one of a row of no frames
                const bool empty = tid == 0 && L == 0;
                s_frk[tid] = empty ? 0.f : -INFINITY; s_fs[tid] = s_frk[tid]; s_flm[tid] = s_frk[tid];
                s_fseq[tid] = 0; s_flen[tid] = empty ? 0 : -1;
            } else {
                const float *fr = p.fin_rec + (base + tid) * 3;
                s_frk[tid] = fr[0]; s_fs[tid] = fr[1]; s_flm[tid] = fr[2];
                s_fseq[tid] = p.fin_seq[base + tid]; s_flen[tid] = p.fin_len[base + tid];
            }
        }
        s_u[tid] = u; s_score[tid] = sc; s_lm[tid] = lm; s_mj[tid] = -1; s_nm[tid] = 0; s_fsrc[tid] = -1;
        s_bl[tid] = p.b * (float)(u + 1);
    }
    __syncthreads();
    // the logits of hypothesis j (live) at v: the same operations whether they are read back from LDS or recomputed, so the same bits
    auto logit = [&](int j, int v) {
        return p.f[(long)n * p.f_rs + (long)(p.step - s_u[j]) * p.f_ts + v] + (p.g[(base + j) * p.ldg + v] + (p.g_bias ? p.g_bias[v] : 0.f));
    };
    auto lm_logit = [&](int j, int v) { return p.lg[(base + j) * p.ldlg + v] + (p.lg_bias ? p.lg_bias[v] : 0.f); };
    auto z = [&](int j, int v) { return p.cached ? zs[j * V + v] : logit(j, v); };
    auto zl = [&](int j, int v) { return p.cached ? zls[j * V + v] : lm_logit(j, v); };
    // a candidate's rank: the blank extension of j with mass s', the extension of j by k (its mass and LM score come back too)
    auto blank_rank = [&](int j, float s) { return __fmaf_rn(p.a, s_lm[j], s) + p.b * (float)s_u[j]; };
    auto label = [&](int j, int k, float &s, float &lm) {
        s = s_score[j] + (z(j, k) - s_lse[j]);
        lm = s_lm[j] + (zl(j, k) - s_llse[j]);
        return __fmaf_rn(p.a, lm, s) + s_bl[j];
    };
    // ---- 1. wave w: both log-sum-exps of hypotheses w, w + 4, ...
    for (int j = wave; j < W; j += BEAM_WAVES) {
        if (s_u[j] < 0) continue;
        const float lse = wave_lse(j, V, p.cached ? zs + j * V : nullptr, logit);
        const float llse = wave_lse(j, V, p.cached ? zls + j * V : nullptr, lm_logit);
        if (lane == 0) {
            s_lse[j] = lse; s_llse[j] = llse;
            s_blank[j] = s_score[j] + (z(j, 0) - lse);
        }
    }
    __syncthreads();
    // ---- 2. the merge: the blank extension of s and the extension of j by s's last token spell the same tokens when y_j = y_s[:-1]; the
    //         masses add, the blank extension (the earlier candidate) keeps its own LM score
    {
        const int s = tid / BEAM_MAX, j = tid % BEAM_MAX;
        if (s < W && j < W && s_u[s] >= 1 && s_u[j] == s_u[s] - 1 && p.step - s_u[s] + 1 < L) {
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
    __syncthreads();
    // ---- 3. complete hypotheses (the blank at the row's last frame), in beam order, into the running W best by rank: a later one
    //         displaces the worst kept (lowest rank, the latest among equals) only with a strictly higher rank
    if (tid == 0) {
        int cnt = p.step == 0 ? (L == 0 ? 1 : 0) : p.fin_n[n];
        bool any = p.step == 0;
        for (int j = 0; j < W; ++j) {
            if (s_u[j] < 0 || p.step - s_u[j] + 1 != L) continue;
            const float sc = blank_rank(j, s_blank[j]);
            int slot = -1;
            for (int w = 0; w < W && slot < 0; ++w) if (s_flen[w] < 0) slot = w;
            if (slot < 0) {
                int worst = 0;
                for (int w = 1; w < W; ++w)
                    if (s_frk[w] < s_frk[worst] || (s_frk[w] == s_frk[worst] && s_fseq[w] > s_fseq[worst])) worst = w;
                if (sc > s_frk[worst]) slot = worst;
            }
            if (slot >= 0) {
                s_frk[slot] = sc; s_fs[slot] = s_blank[j]; s_flm[slot] = s_lm[j]; s_fseq[slot] = cnt; s_flen[slot] = s_u[j]; s_fsrc[slot] = j;
            }
            cnt += 1; any = true;
        }
        if (any) p.fin_n[n] = cnt;
    }
    __syncthreads();
    if (tid < W && (p.step == 0 || s_fsrc[tid] >= 0)) {
        float *fr = p.fin_rec + (base + tid) * 3;
        fr[0] = s_frk[tid]; fr[1] = s_fs[tid]; fr[2] = s_flm[tid];
        p.fin_seq[base + tid] = s_fseq[tid]; p.fin_len[base + tid] = s_flen[tid];
    }
    for (int w = 0; w < W; ++w) {
        const int j = s_fsrc[w];
        if (j < 0) continue;
        for (int x = tid; x < s_u[j]; x += BEAM_THREADS) p.fin_tok[(base + w) * p.tok_ld + x] = p.tok_in[(base + j) * p.tok_ld + x];
    }
    // ---- 4. the W best candidates, one per round.  Positions: the blank extension of j at j, the extension of j by k at W + j V + k.  A
    //         thread owns the blank candidate tid and the extensions by its classes k = 1 + tid, 1 + tid + 256, ... of every hypothesis,
    //         and keeps the first of its candidates in the order behind the last one taken; only the thread that owned the one just taken
    //         looks for its next (positions are unique).
    const bool blank_ok = tid < W && s_u[tid] >= 0 && p.step - s_u[tid] + 1 != L;
    const float blank_sc = blank_ok ? blank_rank(tid, s_blank[tid]) : -INFINITY;
    auto first_behind = [&](float psc, int ppos, float &bsc, int &bpos) {
        bsc = -INFINITY; bpos = NO_CANDIDATE;
        if (blank_ok && before(psc, ppos, blank_sc, tid)) { bsc = blank_sc; bpos = tid; }
        for (int j = 0; j < W; ++j) {
            if (s_u[j] < 0 || s_u[j] >= p.capacity) continue;
            const bool merged = s_nm[j] != 0;
            for (int k = 1 + tid; k < V; k += BEAM_THREADS) {
                float s, lm;
                const float sc = label(j, k, s, lm);
                const int pos = W + j * V + k;
                if (!before(psc, ppos, sc, pos) || !before(sc, pos, bsc, bpos)) continue;
                if (merged) {
                    bool gone = false;
                    for (int s2 = 0; s2 < W; ++s2) gone = gone || (s_mj[s2] == j && s_mk[s2] == k);
                    if (gone) continue;
                }
                bsc = sc; bpos = pos;
            }
        }
    };
    float lsc;
    int lpos, nsel = 0;
    first_behind(INFINITY, -1, lsc, lpos);
    for (int r = 0; r < W; ++r) {
        float bsc = lsc;
        int bpos = lpos;
        first_in_workgroup(s_first, r, bsc, bpos);
        if (bpos == NO_CANDIDATE) break;                                // (uniform) no candidate is left
        if (tid == 0) { sel_sc[r] = bsc; sel_pos[r] = bpos; }
        nsel = r + 1;
        if (lpos == bpos && r + 1 < W) first_behind(bsc, bpos, lsc, lpos);
    }
    __syncthreads();
    // ---- 5. the new beam's records
    if (tid < W) {
        int par = -1, k = 0, u = -1;
        float s = -INFINITY, lm = -INFINITY, rank = -INFINITY;
        if (tid < nsel) {
            const int pos = sel_pos[tid];
            par = pos < W ? pos : (pos - W) / V;
            k = pos < W ? 0 : (pos - W) % V;
            u = s_u[par] + (k != 0);
            rank = sel_sc[tid];
            if (k == 0) { s = s_blank[par]; lm = s_lm[par]; }
            else label(par, k, s, lm);
        }
        float *ro = p.rec_out + (base + tid) * 3;
        ro[0] = s; ro[1] = lm; ro[2] = rank;
        p.u_out[base + tid] = u; p.parent[base + tid] = par; p.last[base + tid] = k;
        s_src[tid] = par < 0 ? tid : par; s_k[tid] = k;                 // the gathers' source: a slot without a hypothesis takes its own
    }
    if (nsel == 0) return;
    __syncthreads();
    if (tid == 0) atomicAdd(p.live, 1);
    // up < capacity where a label is taken: only such hypotheses take labels
    child_rows(p.tok_out + base * p.tok_ld, p.tok_in + base * p.tok_ld, p.tok_ld, nsel, p.capacity, s_src, s_u, s_k,
               [&](int r, int) { return s_k[r] != 0; });
    // ---- 6. the gathers: every new slot's cell inputs and c from its parent's, of the prediction network and of the LM
    gather_state(p.state, base, W, s_src, s_k);
    gather_state(p.lm_state, base, W, s_src, s_k);
}

}  // namespace

extern "C" {

int halo_rnnt_lm_beam_step(const float *f, long f_row_stride, long f_frame_stride, int N, int T, int V, const float *g, long ldg,
                           const float *g_bias, const float *lg, long ldlg, const float *lg_bias, const int *input_lengths, int step,
                           int beam, int capacity, float lm_weight, float insertion_bonus, const float *rec_in, const int *u_in,
                           const int *tokens_in, float *rec_out, int *u_out, int *tokens_out, long tokens_ld, int *parent, int *last,
                           float *fin_rec, int *fin_seq, int *fin_lengths, int *fin_tokens, int *fin_n, const float *wte, int hidden,
                           int layers, const float *h_in, const float *c_in, float *xh, float *c_out, const float *lm_wte, int lm_hidden,
                           int lm_layers, const float *lm_h_in, const float *lm_c_in, float *lm_xh, float *lm_c_out, int *live,
                           halo_stream_t stream) {
    HALO_CHECK_ARG(f && g && lg && input_lengths && rec_in && u_in && tokens_in && rec_out && u_out && tokens_out && parent && last);
    HALO_CHECK_ARG(fin_rec && fin_seq && fin_lengths && fin_tokens && fin_n && wte && h_in && c_in && xh && c_out && live);
    HALO_CHECK_ARG(lm_wte && lm_h_in && lm_c_in && lm_xh && lm_c_out);
    HALO_CHECK_ARG(N > 0 && T > 0 && V >= 2 && V <= 8192 && capacity > 0 && step >= 0 && beam >= 1 && beam <= BEAM_MAX);
    HALO_CHECK_ARG(f_frame_stride >= V && f_row_stride >= (long)(T - 1) * f_frame_stride + V && ldg >= V && ldlg >= V && tokens_ld >= capacity);
    HALO_CHECK_ARG(hidden > 0 && hidden % 4 == 0 && layers > 0 && lm_hidden > 0 && lm_hidden % 4 == 0 && lm_layers > 0);
    HALO_CHECK_ARG(lm_weight == lm_weight && insertion_bonus == insertion_bonus && fabsf(lm_weight) < INFINITY && fabsf(insertion_bonus) < INFINITY);
    HALO_CHECK_ARG(((uintptr_t)wte | (uintptr_t)h_in | (uintptr_t)c_in | (uintptr_t)xh | (uintptr_t)c_out) % 16 == 0);
    HALO_CHECK_ARG(((uintptr_t)lm_wte | (uintptr_t)lm_h_in | (uintptr_t)lm_c_in | (uintptr_t)lm_xh | (uintptr_t)lm_c_out) % 16 == 0);
    HALO_CHECK_ARG(rec_in != rec_out && u_in != u_out && tokens_in != tokens_out && h_in != xh && c_in != c_out);
    HALO_CHECK_ARG(lm_h_in != lm_xh && lm_c_in != lm_c_out);
    RnntLmBeamArgs p;
    p.f = f; p.f_rs = f_row_stride; p.f_ts = f_frame_stride; p.T = T; p.V = V; p.g = g; p.g_bias = g_bias; p.ldg = ldg;
    p.lg = lg; p.lg_bias = lg_bias; p.ldlg = ldlg; p.il = input_lengths; p.step = step; p.W = beam; p.capacity = capacity;
    p.a = lm_weight; p.b = insertion_bonus; p.rec_in = rec_in; p.u_in = u_in; p.tok_in = tokens_in;
    p.rec_out = rec_out; p.u_out = u_out; p.tok_out = tokens_out; p.tok_ld = tokens_ld; p.parent = parent; p.last = last;
    p.fin_rec = fin_rec; p.fin_seq = fin_seq; p.fin_len = fin_lengths; p.fin_tok = fin_tokens; p.fin_n = fin_n;
    p.state = {wte, h_in, c_in, xh, c_out, hidden, layers};
    p.lm_state = {lm_wte, lm_h_in, lm_c_in, lm_xh, lm_c_out, lm_hidden, lm_layers};
    p.live = live;
    p.cached = 2L * beam * V <= LDS_FLOATS;
    hipLaunchKernelGGL(rnnt_lm_beam_step_kernel, dim3((unsigned)N), dim3(BEAM_THREADS), p.cached ? (size_t)2 * beam * V * sizeof(float) : 0,
                       (hipStream_t)stream, p);
    return halo_launch_status();
}

}  // extern "C"
