// Beam search of the encoder-decoder ASR model (haloop_amd/transformer.py BeamDecoder; the definition: include/halo.h)
// on the fused decode launches of decode.hip: a step runs the 5 launches per layer and the LayerNorm + lm_head product on slots = N * W
// rows (slot n * W + r is hypothesis r of utterance n).  The attention launch is decode.hip's dec_attention_pair_kernel with the per-slot
// ancestor table (halo_decode_beam_attention, there); this file holds the launch in the place of dec_token_kernel:
//   dec_beam_select_kernel     one workgroup per utterance, on the pieces of beam_common.h: the log-sum-exp of every live slot, the W
//                              best of the W * V candidates by rank, and the new beam: scores, lengths, flags, tokens, the next step's
//                              ancestor rows and input embeddings.
// With LM shallow fusion (fusion.AttentionFusionDecoder) the same body ranks every candidate by fmaf(lm_weight, lmc, rank),
// lmc the LSTM language model's log-probability of the candidate's tokens: a second log-sum-exp per live slot over the LM's logits, the
// slots' lm carried like their scores, and after the selection the gather of the next LM step's cell inputs from the parents' state.
// Everything the selection writes goes to the OTHER parity copy of the beam (step t reads copy t & 1): the gathers across the slots of an
// utterance never read what this launch writes.  No float atomics, every sum in one order: two decodes are bit-equal.
#include <hip/hip_fp16.h>
#include "halo_common.h"
#include "halo_internal.h"
#include "beam_common.h"

namespace {

using namespace beam;

constexpr int BEAM_LDS_FLOATS = 8192;      // 32 KiB of dynamic LDS, under the 64 KiB a launch gets without the opt-in
constexpr int BEAM_LM_LDS_FLOATS = HALO_DECODE_BEAM_LM_LDS_FLOATS;     // with the LM: both tables, 2 W V floats, in 56 KiB at most (as csrc/rnnt_lm_beam.hip)

struct BeamSelArgs {
    const float *logits;       // [N * W][ld]
    long ld;
    int V, W, t, capacity, etx;
    float bonus;
    const float *score_in;     // the beam this step reads: [N][W] log-probabilities (-inf: empty), lengths, finished flags,
    const int *len_in, *fin_in, *tok_in, *anc_in;     // tokens [N][W][tok_ld], ancestor rows [N * W][anc_ld]
    float *score_out, *rank_out;                      // the beam it writes
    int *len_out, *fin_out, *tok_out, *anc_out;
    long tok_ld, anc_ld;
    const float *wte;          // [vocab][C]
    int C;
    float *y;                  // [N * W][C] <- wte[token] (NULL: the last step)
    int cached;                // the utterance's W V logits are kept in LDS (BEAM_LDS_FLOATS or fewer), else re-read from L2
    // the joint CTC/attention search (dec_beam_select_kernel<true>): rank = (1 - c) * rank + c * psi
    float c, omc;              // ctc_weight and 1 - ctc_weight
    const float *psi_cand;     // [N * W][psi_ld]: the CTC prefix score of every candidate of a live slot (csrc/ctc_prefix_score.hip)
    long psi_ld;
    const float *psi_in;       // [N][W]: the prefix score each slot carries (a finished slot's: its full CTC log-probability)
    float *psi_out;
    int *par_out, *last_out;   // [N][W]: the parent's slot index (-1: empty), the token taken
    // LM shallow fusion (dec_beam_select_kernel<., true>): rank = fmaf(lm_weight, lmc, rank)
    const float *lg, *lg_bias; // [N * W][ldlg] the LM's logits of every slot without their bias; the bias [V] (may be NULL)
    long ldlg;
    const float *lm_in;        // [N][W]: the LM's log-probability of each slot's tokens
    float *lm_out;
    float lmw;                 // lm_weight
    int lm_eos;                // the class whose LM log-probability a closing candidate takes (-1: closing costs nothing)
    StateGather lm_state;      // this step's LM state -> the next step's cell inputs (xh NULL: the last step, no gather)
};

enum { SLOT_EMPTY = 0, SLOT_LIVE = 1, SLOT_FINISHED = 2 };

// JOINT: the candidates are ranked by the mix with their CTC prefix scores; everything else is the same code, so the plain launch keeps
// its bits.  The mix is two products and a sum, each rounded (no fused multiply-add): c = 0 returns the plain rank bit for bit.
// LM: the candidates' ranks take fmaf(lm_weight, lmc, .) on top, under a second template parameter in the same way.
template <bool JOINT, bool LM>
__global__ __launch_bounds__(BEAM_THREADS) void dec_beam_select_kernel(const BeamSelArgs p) {
    __shared__ float s_score[BEAM_MAX], s_lse[BEAM_MAX], sel_rank[BEAM_MAX], s_psi[BEAM_MAX], s_lm[BEAM_MAX], s_llse[BEAM_MAX];
    __shared__ int s_len[BEAM_MAX], s_state[BEAM_MAX], sel_pos[BEAM_MAX], s_par[BEAM_MAX], s_k[BEAM_MAX], s_src[BEAM_MAX];
    __shared__ FirstScratch s_first;
    extern __shared__ float zs[];                                      // cached: zs[j][v] = logits of slot j | LM: zls[j][v] behind them
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, W = p.W, V = p.V;
    const long base = (long)n * W;
    float *zls = zs + W * V;
    if (tid < BEAM_MAX) {
        float sc = -INFINITY;
        int len = 0, st = SLOT_EMPTY;
        if (tid < W) {
            if (p.t == 0) {                                            // the records are not read: slot 0 holds [STX]
                if (tid == 0) { sc = 0.f; st = SLOT_LIVE; }
            } else {
                sc = p.score_in[base + tid];
                len = p.len_in[base + tid];
                st = sc > -INFINITY ? (p.fin_in[base + tid] ? SLOT_FINISHED : SLOT_LIVE) : SLOT_EMPTY;
                if (len < 0 || len > p.t) st = SLOT_EMPTY;             // (never under the host's loop) no token row is overrun
            }
        }
        s_score[tid] = sc; s_len[tid] = len; s_state[tid] = st;
        if (JOINT) s_psi[tid] = (tid < W && p.t > 0 && st != SLOT_EMPTY) ? p.psi_in[base + tid] : (st == SLOT_LIVE ? 0.f : -INFINITY);
        if (LM) s_lm[tid] = (tid < W && p.t > 0 && st != SLOT_EMPTY) ? p.lm_in[base + tid] : (st == SLOT_LIVE ? 0.f : -INFINITY);
    }
    __syncthreads();
    auto logit = [&](int j, int v) { return p.logits[(base + j) * p.ld + v]; };
    auto z = [&](int j, int v) { return p.cached ? zs[j * V + v] : logit(j, v); };
    auto lm_logit = [&](int j, int v) { return p.lg[(base + j) * p.ldlg + v] + (p.lg_bias ? p.lg_bias[v] : 0.f); };
    auto zl = [&](int j, int v) { return p.cached ? zls[j * V + v] : lm_logit(j, v); };
    // ---- 1. wave w: log-sum-exp of slots w, w + 4, ...
    for (int j = wave; j < W; j += BEAM_WAVES) {
        if (s_state[j] != SLOT_LIVE) continue;
        const float lse = wave_lse(j, V, p.cached ? zs + j * V : nullptr, logit);
        if (lane == 0) s_lse[j] = lse;
        if (LM) {
            const float llse = wave_lse(j, V, p.cached ? zls + j * V : nullptr, lm_logit);
            if (lane == 0) s_llse[j] = llse;
        }
    }
    __syncthreads();
    // the candidate (j, k) of a live slot: its log-probability and its rank, by the same operations wherever they are needed
    auto cand_score = [&](int j, int k) { return s_score[j] + (z(j, k) - s_lse[j]); };
    auto mix = [&](float rk, float psi) { return JOINT ? __fadd_rn(__fmul_rn(p.omc, rk), __fmul_rn(p.c, psi)) : rk; };
    // the LM's score of candidate (j, k) of a live slot: a label adds its log-probability, closing that of lm_eos (none: nothing)
    auto cand_lm = [&](int j, int k) {
        const int kl = k != p.etx ? k : p.lm_eos;
        return kl < 0 ? s_lm[j] : s_lm[j] + (zl(j, kl) - s_llse[j]);
    };
    auto cand_rank = [&](int j, int k, float sc) {
        float rk = fmaf(p.bonus, (float)(s_len[j] + (k != p.etx)), sc);
        if (JOINT) rk = mix(rk, p.psi_cand[(base + j) * p.psi_ld + k]);
        return LM ? fmaf(p.lmw, cand_lm(j, k), rk) : rk;
    };
    // ---- 2. the W best candidates, one per round: the first in the order among those behind the last one taken.  Position j V + k; a
    //         finished slot has the one candidate (j, ETX).
    float prank = INFINITY;
    int ppos = -1, nsel = 0;
    for (int r = 0; r < W; ++r) {
        float brank = -INFINITY;
        int bpos = NO_CANDIDATE;
        if (tid < W && s_state[tid] == SLOT_FINISHED) {
            float rk = mix(fmaf(p.bonus, (float)s_len[tid], s_score[tid]), JOINT ? s_psi[tid] : 0.f);
            if (LM) rk = fmaf(p.lmw, s_lm[tid], rk);
            const int pos = tid * V + p.etx;
            if (rk > -INFINITY && before(prank, ppos, rk, pos)) { brank = rk; bpos = pos; }
        }
        for (int j = 0; j < W; ++j) {
            if (s_state[j] != SLOT_LIVE) continue;
            for (int k = tid; k < V; k += BEAM_THREADS) {
                const float rk = cand_rank(j, k, cand_score(j, k));
                const int pos = j * V + k;
                if (!(rk > -INFINITY) || !before(prank, ppos, rk, pos) || !before(rk, pos, brank, bpos)) continue;
                brank = rk; bpos = pos;
            }
        }
        first_in_workgroup(s_first, r, brank, bpos);
        if (bpos == NO_CANDIDATE) break;                                // (uniform) no candidate is left
        if (tid == 0) { sel_rank[r] = brank; sel_pos[r] = bpos; }
        prank = brank; ppos = bpos; nsel = r + 1;
    }
    __syncthreads();
    // ---- 3. the new beam's records, in the order taken; a slot that took nothing is empty
    if (tid < W) {
        int par = -1, k = p.etx, len = 0, fin = 0;
        float sc = -INFINITY, rk = -INFINITY;
        if (tid < nsel) {
            const int pos = sel_pos[tid];
            par = pos / V; k = pos % V; rk = sel_rank[tid];
            if (s_state[par] == SLOT_FINISHED) { sc = s_score[par]; len = s_len[par]; fin = 1; }
            else { sc = cand_score(par, k); len = s_len[par] + (k != p.etx); fin = k == p.etx; }
        }
        p.score_out[base + tid] = sc; p.rank_out[base + tid] = rk; p.len_out[base + tid] = len; p.fin_out[base + tid] = fin;
        if (JOINT) {
            float psi = -INFINITY;
            if (par >= 0) psi = s_state[par] == SLOT_FINISHED ? s_psi[par] : p.psi_cand[(base + par) * p.psi_ld + k];
            p.psi_out[base + tid] = psi;
        }
        if (JOINT || LM) { p.par_out[base + tid] = par; p.last_out[base + tid] = k; }
        if (LM) {
            float lm = -INFINITY;
            if (par >= 0) lm = s_state[par] == SLOT_FINISHED ? s_lm[par] : cand_lm(par, k);
            p.lm_out[base + tid] = lm;
            s_src[tid] = (par >= 0 && s_state[par] == SLOT_LIVE && k != p.etx) ? par : -1;     // the slots that step the LM
        }
        s_par[tid] = par; s_k[tid] = k;
    }
    __syncthreads();
    // ---- 4. tokens (without STX and ETX): the parent's row, plus k
    child_rows(p.tok_out + base * p.tok_ld, p.tok_in + base * p.tok_ld, p.tok_ld, nsel, p.capacity, s_par, s_len, s_k,
               [&](int r, int par) { return s_state[par] == SLOT_LIVE && s_k[r] != p.etx; });
    // ---- 5. the next step's ancestor rows: the parent's history, then the parent's own row for position t (an empty slot: its own row)
    for (int idx = tid; idx < W * (p.t + 1); idx += BEAM_THREADS) {
        const int r = idx / (p.t + 1), x = idx % (p.t + 1), par = s_par[r];
        int row = (int)base + (par < 0 ? r : par);
        if (x < p.t && par >= 0) row = p.anc_in[(base + par) * p.anc_ld + x];
        p.anc_out[(base + r) * p.anc_ld + x] = row;
    }
    // ---- 6. the next LM step's cell inputs: a slot that took a label gets [wte[k] | h] and c of its PARENT, every other slot zeros
    if (LM && p.lm_state.xh) gather_state<true>(p.lm_state, base, W, s_src, s_k);
    // ---- 7. the next step's input rows
    if (!p.y) return;
    const int C4 = p.C / 4;
    for (int idx = tid; idx < W * C4; idx += BEAM_THREADS) {
        const int r = idx / C4, c = idx % C4;
        reinterpret_cast<f32x4 *>(p.y + (base + r) * p.C)[c] = reinterpret_cast<const f32x4 *>(p.wte + (long)s_k[r] * p.C)[c];
    }
}

// what the halo_decode_beam_select entry points check and pass on; the joint and LM entries add their own
int beam_select_args(BeamSelArgs &p, const float *logits, long ld, int N, int beam, int V, int t, int capacity, int etx, float length_bonus,
                     const float *scores_in, const int *lengths_in, const int *finished_in, const int *tokens_in, const int *ancestors_in,
                     float *scores_out, float *ranks_out, int *lengths_out, int *finished_out, int *tokens_out, int *ancestors_out,
                     long tokens_ld, long ancestors_ld, const float *wte, int vocab, int C, float *y_next) {
    HALO_CHECK_ARG(logits && scores_in && lengths_in && finished_in && tokens_in && ancestors_in);
    HALO_CHECK_ARG(scores_out && ranks_out && lengths_out && finished_out && tokens_out && ancestors_out);
    HALO_CHECK_ARG(N > 0 && beam >= 1 && beam <= BEAM_MAX && V > 0 && V <= 8192 && ld >= V && etx >= 0 && etx < V);
    HALO_CHECK_ARG(t >= 0 && t < capacity && tokens_ld >= capacity && ancestors_ld > t && (long)N * beam <= 0x7fffffffL / V);
    HALO_CHECK_ARG(scores_in != scores_out && lengths_in != lengths_out && finished_in != finished_out && tokens_in != tokens_out &&
                   ancestors_in != ancestors_out);
    HALO_CHECK_ARG(!y_next || (wte && vocab >= V && C > 0 && C % 4 == 0 && ((uintptr_t)wte | (uintptr_t)y_next) % 16 == 0));
    p.logits = logits; p.ld = ld; p.V = V; p.W = beam; p.t = t; p.capacity = capacity; p.etx = etx; p.bonus = length_bonus;
    p.score_in = scores_in; p.len_in = lengths_in; p.fin_in = finished_in; p.tok_in = tokens_in; p.anc_in = ancestors_in;
    p.score_out = scores_out; p.rank_out = ranks_out; p.len_out = lengths_out; p.fin_out = finished_out; p.tok_out = tokens_out;
    p.anc_out = ancestors_out; p.tok_ld = tokens_ld; p.anc_ld = ancestors_ld; p.wte = wte; p.C = C; p.y = y_next;
    p.cached = (long)beam * V <= BEAM_LDS_FLOATS;
    return HALO_OK;
}

size_t beam_select_lds(const BeamSelArgs &p) { return p.cached ? (size_t)p.W * p.V * sizeof(float) : 0; }

void beam_select_no_lm(BeamSelArgs &p) {
    p.lg = p.lg_bias = p.lm_in = nullptr; p.lm_out = nullptr; p.ldlg = 0; p.lmw = 0.f; p.lm_eos = -1;
    p.lm_state = {nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0};
}

}  // namespace

extern "C" {

int halo_decode_beam_select(const float *logits, long ld, int N, int beam, int V, int t, int capacity, int etx, float length_bonus,
                            const float *scores_in, const int *lengths_in, const int *finished_in, const int *tokens_in,
                            const int *ancestors_in, float *scores_out, float *ranks_out, int *lengths_out, int *finished_out,
                            int *tokens_out, int *ancestors_out, long tokens_ld, long ancestors_ld, const float *wte, int vocab, int C,
                            float *y_next, halo_stream_t stream) {
    BeamSelArgs p;
    const int status = beam_select_args(p, logits, ld, N, beam, V, t, capacity, etx, length_bonus, scores_in, lengths_in, finished_in,
                                        tokens_in, ancestors_in, scores_out, ranks_out, lengths_out, finished_out, tokens_out,
                                        ancestors_out, tokens_ld, ancestors_ld, wte, vocab, C, y_next);
    if (status != HALO_OK) return status;
    p.c = 0.f; p.omc = 1.f; p.psi_cand = nullptr; p.psi_ld = 0; p.psi_in = nullptr; p.psi_out = nullptr; p.par_out = p.last_out = nullptr;
    beam_select_no_lm(p);
    hipLaunchKernelGGL((dec_beam_select_kernel<false, false>), dim3((unsigned)N), dim3(BEAM_THREADS), beam_select_lds(p), (hipStream_t)stream, p);
    return halo_launch_status();
}

int halo_decode_beam_select_joint(const float *logits, long ld, int N, int beam, int V, int t, int capacity, int etx, float length_bonus,
                                  float ctc_weight, const float *psi_cand, long psi_ld, const float *psi_in, float *psi_out,
                                  const float *scores_in, const int *lengths_in, const int *finished_in, const int *tokens_in,
                                  const int *ancestors_in, float *scores_out, float *ranks_out, int *lengths_out, int *finished_out,
                                  int *tokens_out, int *ancestors_out, int *parents_out, int *last_out, long tokens_ld, long ancestors_ld,
                                  const float *wte, int vocab, int C, float *y_next, halo_stream_t stream) {
    BeamSelArgs p;
    const int status = beam_select_args(p, logits, ld, N, beam, V, t, capacity, etx, length_bonus, scores_in, lengths_in, finished_in,
                                        tokens_in, ancestors_in, scores_out, ranks_out, lengths_out, finished_out, tokens_out,
                                        ancestors_out, tokens_ld, ancestors_ld, wte, vocab, C, y_next);
    if (status != HALO_OK) return status;
    HALO_CHECK_ARG(psi_cand && psi_in && psi_out && parents_out && last_out && psi_in != psi_out && psi_ld >= V);
    HALO_CHECK_ARG(ctc_weight >= 0.f && ctc_weight <= 1.f);
    p.c = ctc_weight; p.omc = 1.0f - ctc_weight; p.psi_cand = psi_cand; p.psi_ld = psi_ld; p.psi_in = psi_in; p.psi_out = psi_out;
    p.par_out = parents_out; p.last_out = last_out;
    beam_select_no_lm(p);
    hipLaunchKernelGGL((dec_beam_select_kernel<true, false>), dim3((unsigned)N), dim3(BEAM_THREADS), beam_select_lds(p), (hipStream_t)stream, p);
    return halo_launch_status();
}

int halo_decode_beam_select_lm(const float *logits, long ld, int N, int beam, int V, int t, int capacity, int etx, float length_bonus,
                               float ctc_weight, const float *psi_cand, long psi_ld, const float *psi_in, float *psi_out, const float *lg,
                               long ldlg, const float *lg_bias, const float *lm_in, float *lm_out, float lm_weight, int lm_eos,
                               const float *scores_in, const int *lengths_in, const int *finished_in, const int *tokens_in,
                               const int *ancestors_in, float *scores_out, float *ranks_out, int *lengths_out, int *finished_out,
                               int *tokens_out, int *ancestors_out, int *parents_out, int *last_out, long tokens_ld, long ancestors_ld,
                               const float *wte, int vocab, int C, float *y_next, const float *lm_wte, int lm_hidden, int lm_layers,
                               const float *h_in, const float *c_in, float *lm_xh, float *c_out, halo_stream_t stream) {
    BeamSelArgs p;
    const int status = beam_select_args(p, logits, ld, N, beam, V, t, capacity, etx, length_bonus, scores_in, lengths_in, finished_in,
                                        tokens_in, ancestors_in, scores_out, ranks_out, lengths_out, finished_out, tokens_out,
                                        ancestors_out, tokens_ld, ancestors_ld, wte, vocab, C, y_next);
    if (status != HALO_OK) return status;
    HALO_CHECK_ARG(lg && lm_in && lm_out && lm_in != lm_out && parents_out && last_out && ldlg >= V && lm_eos >= -1 && lm_eos < V);
    HALO_CHECK_ARG(lm_weight == lm_weight && fabsf(lm_weight) < INFINITY);
    if (psi_cand) {
        HALO_CHECK_ARG(psi_in && psi_out && psi_in != psi_out && psi_ld >= V && ctc_weight >= 0.f && ctc_weight <= 1.f);
    } else {
        HALO_CHECK_ARG(!psi_in && !psi_out);
    }
    if (lm_xh) {                                                       // (NULL: the last step, nothing steps the LM again)
        HALO_CHECK_ARG(lm_wte && h_in && c_in && c_out && lm_hidden > 0 && lm_hidden % 4 == 0 && lm_layers > 0 && h_in != lm_xh && c_in != c_out);
        HALO_CHECK_ARG(((uintptr_t)lm_wte | (uintptr_t)h_in | (uintptr_t)c_in | (uintptr_t)lm_xh | (uintptr_t)c_out) % 16 == 0);
    }
    p.c = psi_cand ? ctc_weight : 0.f; p.omc = 1.0f - p.c; p.psi_cand = psi_cand; p.psi_ld = psi_ld; p.psi_in = psi_in; p.psi_out = psi_out;
    p.par_out = parents_out; p.last_out = last_out;
    p.lg = lg; p.lg_bias = lg_bias; p.ldlg = ldlg; p.lm_in = lm_in; p.lm_out = lm_out; p.lmw = lm_weight; p.lm_eos = lm_eos;
    p.lm_state = {lm_wte, h_in, c_in, lm_xh, c_out, lm_hidden, lm_layers};
    p.cached = 2L * beam * V <= BEAM_LM_LDS_FLOATS;                    // both tables or neither: the same bits either way
    const size_t lds = p.cached ? (size_t)2 * beam * V * sizeof(float) : 0;
    if (psi_cand) hipLaunchKernelGGL((dec_beam_select_kernel<true, true>), dim3((unsigned)N), dim3(BEAM_THREADS), lds, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((dec_beam_select_kernel<false, true>), dim3((unsigned)N), dim3(BEAM_THREADS), lds, (hipStream_t)stream, p);
    return halo_launch_status();
}

}  // extern "C"
