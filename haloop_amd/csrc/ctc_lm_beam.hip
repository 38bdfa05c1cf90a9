// CTC prefix beam search with shallow fusion of an LSTM language model (haloop_amd/fusion.py CTCFusionDecoder): one frame
// of every row per launch, one workgroup per row.  The search is csrc/ctc_prefix_beam.hip's on the pieces of beam_common.h; a member
// carries besides its CTC masses pb / pnb the LM's log-probability lm of its prefix, and slot n W + j holds the LM's logits g and LSTM
// state after that prefix.  Per frame t < L
//   1. wave w: the log-sum-exp over V of g[slot j] + g_bias for members j = w, w + 4, ..., so lp_j[k] = (g_j[k] + bias[k]) - lse_j
//   2. totals, stay candidates and the merge (CTC mass only: the stay keeps its own lm)
//   3. the W best: an extension of j by k ranks at fma(a, lm_j + lp_j[k], e[t, k] + (pb_j if k == last_j else total_j)) + b (len_j + 1),
//      a stay at fma(a, lm_j, logaddexp(pb', pnb')) + b len_j; candidates whose CTC mass is -inf are never taken.  A thread owns the
//      extensions by its classes and keeps its first across the rounds.
//   4. the new beam's records, tokens, parent and last (0: a stay) into the other copy
//   5. the gather of the LSTM state for the cell launches
// A row with t >= L passes its beam through (parent = own index, last = 0) and loads no emission.  The launches that follow (one
// halo_rnnt_lstm_cell per layer, halo_decode_linear, halo_rnnt_beam_keep) are csrc/rnnt_beam.hip's, unchanged.
// LDS: the frame's V emissions and, when (W + 1) V <= LDS_FLOATS, the row's W V LM logits (56 KiB of dynamic LDS at most; otherwise the
// logits are recomputed from L2), besides W-sized records (< 2 KiB static): under the 64 KiB a launch gets without the opt-in.
#include "halo_common.h"
#include "halo_internal.h"
#include "beam_common.h"

namespace {

using namespace beam;

constexpr int LDS_FLOATS = 14336;          // 56 KiB of dynamic LDS: the frame's emissions (V <= 8192) and, when they fit too, W V logits

struct CtcLmBeamArgs {
    const float *e;            // [T][N][V] log-probabilities, strides st (frame) and sn (row), unit class stride
    long st, sn;
    int T, V, W, cap, t;
    const int *il;             // [N] frames of each row (clamped to [0, T] here)
    float a, b;                // lm_weight, insertion_bonus
    const float *g, *g_bias;   // [N * W][ldg] LM logits of every slot without their bias; the bias [V] (may be NULL)
    long ldg;
    const float *rec_in;       // [N][W][4] pb | pnb | lm | ranking value
    const int *meta_in;        // [N][W][4] length (-1: no member) | last token | hash of the prefix | hash without its last token
    const int *tok_in;         // [N][W][tok_ld]
    float *rec_out;
    int *meta_out, *tok_out;
    long tok_ld;
    int *parent, *last;        // [N][W] of the new beam
    StateGather state;         // this frame's state -> the cells' inputs
    int cached;                // the row's W V logits are kept in LDS, else recomputed from L2
};

__global__ __launch_bounds__(BEAM_THREADS) void ctc_lm_beam_step_kernel(const CtcLmBeamArgs p) {
    // the beam read: masses, LM score, length, last token, hashes; the frame: lse, totals, the stay candidates' masses and rank, the
    // insertion bonus of an extension, the shortlist (bit j of word s), the member whose extension merged into s (-1), whether an
    // extension of j was merged away; the new beam: rank, position, and the gather's source slot and token
    __shared__ float s_pb[BEAM_MAX], s_pnb[BEAM_MAX], s_lm[BEAM_MAX], s_sc[BEAM_MAX], s_lse[BEAM_MAX], s_tot[BEAM_MAX], s_spb[BEAM_MAX],
        s_spnb[BEAM_MAX], s_bl[BEAM_MAX], sel_sc[BEAM_MAX];
    __shared__ int s_len[BEAM_MAX], s_ltok[BEAM_MAX], s_short[BEAM_MAX], s_mj[BEAM_MAX], s_nm[BEAM_MAX], sel_pos[BEAM_MAX], s_src[BEAM_MAX],
        s_k[BEAM_MAX];
    __shared__ unsigned s_hash[BEAM_MAX], s_hprev[BEAM_MAX];
    __shared__ FirstScratch s_first;
    extern __shared__ float dyn[];                                     // e[V] | cached: z[j][v] = g_j[v] + bias[v]
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, W = p.W, V = p.V, cap = p.cap;
    const long base = (long)n * W;
    const int L = min(max(p.il[n], 0), p.T);
    const bool active = p.t < L;                                       // (uniform over the workgroup)
    float *s_e = dyn, *zs = dyn + V;
    if (tid < BEAM_MAX) {
        float pb = -INFINITY, pnb = -INFINITY, lm = -INFINITY, sc = -INFINITY;
        int len = -1, ltok = 0;
        unsigned hash = 0u, hprev = 0u;
        if (tid < W) {
            if (p.t == 0) {                                            // the empty prefix: every alignment of no frames ends "in blank"
                if (tid == 0) { pb = 0.f; lm = 0.f; sc = 0.f; len = 0; hash = HASH_EMPTY; }
            } else {
                const float *rf = p.rec_in + (base + tid) * 4;
                const int *ri = p.meta_in + (base + tid) * 4;
                pb = rf[0]; pnb = rf[1]; lm = rf[2]; sc = rf[3];
                len = ri[0]; ltok = ri[1]; hash = (unsigned)ri[2]; hprev = (unsigned)ri[3];
                if (len > cap) len = -1;                               // (never under the host's loop)
            }
        }
        s_pb[tid] = pb; s_pnb[tid] = pnb; s_lm[tid] = lm; s_sc[tid] = sc; s_len[tid] = len; s_ltok[tid] = ltok;
        s_hash[tid] = hash; s_hprev[tid] = hprev; s_short[tid] = 0; s_mj[tid] = -1; s_nm[tid] = 0;
    }
    if (active) {                                                      // frame t < L of this row alone
        const float *row = p.e + (long)p.t * p.st + (long)n * p.sn;
        for (int k = tid; k < V; k += BEAM_THREADS) s_e[k] = row[k];
    }
    __syncthreads();
    int nb = 0;                                                        // members stand first, in the order taken
    while (nb < W && s_len[nb] >= 0) ++nb;
    int nsel = nb;

    // the LM logit of member j at class v: the same operations whether it is read back from LDS or recomputed, so the same bits
    auto logit = [&](int j, int v) { return p.g[(base + j) * p.ldg + v] + (p.g_bias ? p.g_bias[v] : 0.f); };
    auto z = [&](int j, int v) { return p.cached ? zs[j * V + v] : logit(j, v); };
    // the extension of j by k: its CTC mass, the LM score of its prefix, its rank
    auto extension = [&](int j, int k, float &ctc, float &lm) {
        ctc = s_e[k] + (k == s_ltok[j] ? s_pb[j] : s_tot[j]);
        lm = s_lm[j] + (z(j, k) - s_lse[j]);
        return __fmaf_rn(p.a, lm, ctc) + s_bl[j];
    };

    if (active) {
        // ---- 1. wave w: log-sum-exp of members w, w + 4, ...
        for (int j = wave; j < nb; j += BEAM_WAVES) {
            const float lse = wave_lse(j, V, p.cached ? zs + j * V : nullptr, logit);
            if (lane == 0) s_lse[j] = lse;
        }
        // ---- 2. totals and stay candidates; the shortlist of (s, j) with y_s possibly y_j + [last_s]
        if (tid < nb) {
            const float pb = s_pb[tid], pnb = s_pnb[tid], tot = logaddexpf_(pb, pnb);
            s_tot[tid] = tot;
            s_spb[tid] = tot + s_e[0];
            s_spnb[tid] = s_len[tid] > 0 ? pnb + s_e[s_ltok[tid]] : -INFINITY;
            s_bl[tid] = p.b * (float)(s_len[tid] + 1);
        }
        shortlist_pair(nb, s_len, s_hash, s_hprev, s_short);
        __syncthreads();
        // the merge: wave w compares the tokens of the shortlisted pairs of s = w, w + 4, ...
        for (int s = wave; s < nb; s += BEAM_WAVES) {
            const int j = merged_member(s, s_short[s], s_len, [&](int m) { return p.tok_in + (base + m) * p.tok_ld; });
            if (j >= 0 && lane == 0) {
                const int k = s_ltok[s];
                s_mj[s] = j; s_nm[j] = 1;
                s_spnb[s] = logaddexpf_(s_spnb[s], s_e[k] + (k == s_ltok[j] ? s_pb[j] : s_tot[j]));
            }
        }
        __syncthreads();
        // ---- 3. the W best candidates, one per round.  A thread owns the stay candidate tid and the extensions by its classes k = 1 + tid,
        //         1 + tid + 256, ... of every member, and keeps the first of its candidates in the order behind the last one taken; only
        //         the thread that owned the one just taken looks for its next (positions are unique).
        float stay_sc = -INFINITY;
        bool stay_ok = false;
        if (tid < nb) {
            const float ctc = logaddexpf_(s_spb[tid], s_spnb[tid]);
            stay_ok = ctc > -INFINITY;
            stay_sc = __fmaf_rn(p.a, s_lm[tid], ctc) + p.b * (float)s_len[tid];
        }
        auto first_behind = [&](float psc, int ppos, float &bsc, int &bpos) {
            bsc = -INFINITY; bpos = NO_CANDIDATE;
            if (stay_ok && before(psc, ppos, stay_sc, tid)) { bsc = stay_sc; bpos = tid; }
            for (int j = 0; j < nb; ++j) {
                if (s_len[j] >= cap) continue;                          // no room: no extension
                const bool merged = s_nm[j] != 0;
                for (int k = 1 + tid; k < V; k += BEAM_THREADS) {
                    float ctc, lm;
                    const float sc = extension(j, k, ctc, lm);
                    const int pos = W + j * V + k;
                    if (!(ctc > -INFINITY) || !before(psc, ppos, sc, pos) || !before(sc, pos, bsc, bpos)) continue;
                    if (merged) {
                        bool gone = false;
                        for (int s = 0; s < nb; ++s) gone = gone || (s_mj[s] == j && s_ltok[s] == k);
                        if (gone) continue;
                    }
                    bsc = sc; bpos = pos;
                }
            }
        };
        float lsc;
        int lpos;
        nsel = 0;
        first_behind(INFINITY, -1, lsc, lpos);
        for (int r = 0; r < W; ++r) {
            float bsc = lsc;
            int bpos = lpos;
            first_in_workgroup(s_first, r, bsc, bpos);
            if (bpos == NO_CANDIDATE) break;                            // (uniform) no candidate is left
            if (tid == 0) { sel_sc[r] = bsc; sel_pos[r] = bpos; }
            nsel = r + 1;
            if (lpos == bpos && r + 1 < W) first_behind(bsc, bpos, lsc, lpos);
        }
        __syncthreads();
    }
    // ---- 4. the new beam's records, in the order taken, into the other copy; a row past its frames keeps its own
    if (tid < W) {
        float pb = -INFINITY, pnb = -INFINITY, lm = -INFINITY, sc = -INFINITY;
        int len = -1, ltok = 0, par = -1, k = 0;
        unsigned hash = 0u, hprev = 0u;
        if (tid < nsel) {
            const int pos = active ? sel_pos[tid] : tid;
            par = pos < W ? pos : (pos - W) / V;
            k = pos < W ? 0 : (pos - W) % V;
            if (k == 0) {
                pb = active ? s_spb[par] : s_pb[par]; pnb = active ? s_spnb[par] : s_pnb[par]; lm = s_lm[par];
                len = s_len[par]; ltok = s_ltok[par]; hash = s_hash[par]; hprev = s_hprev[par];
                sc = active ? sel_sc[tid] : s_sc[par];
            } else {
                float ctc;
                extension(par, k, ctc, lm);
                pnb = ctc; len = s_len[par] + 1; ltok = k; hprev = s_hash[par]; hash = hash_append(s_hash[par], k);
                sc = sel_sc[tid];
            }
        }
        float *rf = p.rec_out + (base + tid) * 4;
        int *ri = p.meta_out + (base + tid) * 4;
        rf[0] = pb; rf[1] = pnb; rf[2] = lm; rf[3] = sc;
        ri[0] = len; ri[1] = ltok; ri[2] = (int)hash; ri[3] = (int)hprev;
        p.parent[base + tid] = par; p.last[base + tid] = k;
        s_src[tid] = par < 0 ? tid : par; s_k[tid] = k;                 // the gather's source: a slot without a member takes its own
    }
    __syncthreads();
    // lp < cap where a label is taken: only such members are extended
    child_rows(p.tok_out + base * p.tok_ld, p.tok_in + base * p.tok_ld, p.tok_ld, nsel, cap, s_src, s_len, s_k,
               [&](int r, int) { return s_k[r] != 0; });
    // ---- 5. the gather: every new slot's cell inputs and c from its parent's
    gather_state(p.state, base, W, s_src, s_k);
}

}  // namespace

extern "C" {

int halo_ctc_lm_beam_step(const float *emissions, long stride_t, long stride_n, int T, int N, int V, const int *emission_lengths, int frame,
                          int beam, int capacity, float lm_weight, float insertion_bonus, const float *g, long ldg, const float *g_bias,
                          const float *rec_in, const int *meta_in, const int *tokens_in, float *rec_out, int *meta_out, int *tokens_out,
                          long tokens_ld, int *parent, int *last, const float *wte, int hidden, int layers, const float *h_in,
                          const float *c_in, float *xh, float *c_out, halo_stream_t stream) {
    HALO_CHECK_ARG(emissions && emission_lengths && g && rec_in && meta_in && tokens_in && rec_out && meta_out && tokens_out);
    HALO_CHECK_ARG(parent && last && wte && h_in && c_in && xh && c_out);
    HALO_CHECK_ARG(N > 0 && T > 0 && V >= 2 && V <= 8192 && beam >= 1 && beam <= BEAM_MAX && frame >= 0 && frame < T);
    HALO_CHECK_ARG(capacity >= 1 && tokens_ld >= capacity && ldg >= V && hidden > 0 && hidden % 4 == 0 && layers > 0);
    HALO_CHECK_ARG(lm_weight == lm_weight && insertion_bonus == insertion_bonus && fabsf(lm_weight) < INFINITY && fabsf(insertion_bonus) < INFINITY);
    HALO_CHECK_ARG(((uintptr_t)wte | (uintptr_t)h_in | (uintptr_t)c_in | (uintptr_t)xh | (uintptr_t)c_out) % 16 == 0);
    HALO_CHECK_ARG(rec_in != rec_out && meta_in != meta_out && tokens_in != tokens_out && h_in != xh && c_in != c_out);
    CtcLmBeamArgs p;
    p.e = emissions; p.st = stride_t; p.sn = stride_n; p.T = T; p.V = V; p.W = beam; p.cap = capacity; p.t = frame; p.il = emission_lengths;
    p.a = lm_weight; p.b = insertion_bonus; p.g = g; p.g_bias = g_bias; p.ldg = ldg; p.rec_in = rec_in; p.meta_in = meta_in;
    p.tok_in = tokens_in; p.rec_out = rec_out; p.meta_out = meta_out; p.tok_out = tokens_out; p.tok_ld = tokens_ld; p.parent = parent;
    p.last = last; p.state = {wte, h_in, c_in, xh, c_out, hidden, layers};
    p.cached = ((long)beam + 1) * V <= LDS_FLOATS;
    const size_t lds = (size_t)(p.cached ? beam + 1 : 1) * V * sizeof(float);
    hipLaunchKernelGGL(ctc_lm_beam_step_kernel, dim3((unsigned)N), dim3(BEAM_THREADS), lds, (hipStream_t)stream, p);
    return halo_launch_status();
}

}  // extern "C"
