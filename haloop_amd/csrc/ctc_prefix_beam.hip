// CTC prefix beam search with exact merging (haloop_amd/ctc.py ctc_prefix_beam_search; [Hannun14], Graves' prefix search; DESIGN.md
// 3.3p): the whole decode of a batch in one launch, one workgroup per utterance, the frame loop inside.  A beam member is a prefix y with
// the log-mass of its alignments that end in blank (pb) and in its last label (pnb).  Per frame t < L
//   1. every member's stay candidate (pb' = total + e[t, 0], pnb' = pnb + e[t, last]) and total = logaddexp(pb, pnb)
//   2. the merge (beam_common.h): the mass of the extension of j that spells stay candidate s joins pnb'_s and the extension is no
//      candidate.  Two members never extend to the same prefix, so there is no other merge.
//   3. the W best of the stay candidates (position j) and the extensions (position W + j V + k, score e[t, k] + (pb_j if k == last_j else
//      total_j), only from members shorter than the capacity), one per round.  A thread owns the extensions by its classes and keeps its
//      first across the rounds; only the owner of the candidate just taken looks for its next.  A candidate's score is two operands away
//      from the frame's emissions.  Candidates at -inf are never taken.
//   4. the new beam's records and token rows, in the order taken, into the other copy of the beam (double-buffered by frame parity).
// LDS: the records (W-sized, < 2 KiB static); the frame's V emissions, double-buffered so that frame t + 1 is requested from global memory
// before frame t's rounds and lands in LDS behind them (E_LDS_FLOATS = 8192 floats = 32 KiB of dynamic LDS: V <= 4096; above that the
// rounds read the emissions from L2 by the same operations, the same bits); the token rows of both copies of the beam as 16-bit tokens
// (TOK_LDS_TOKENS = 12288 = 24 KiB: 2 W capacity <= 12288 and V <= 65536; otherwise they live in the caller's workspace as 32-bit
// tokens, written and read by this workgroup alone).  58 KiB at most: under the 64 KiB a launch gets without the opt-in.
// Frames at or past L, and another row's frames, are never loaded.
//
// The carried search (halo_ctc_prefix_beam_advance, haloop_amd/ctc.py PrefixBeamStream) is the same kernel template with
// CARRIED set: the frame loop is entered from a beam in global memory and left into it, so a stream's frames may arrive over any number
// of launches.  A row's state is a BeamRecords header and its token rows: one copy of 16-bit tokens where the launch works on them in LDS
// (loaded and stored once per launch), else both copies of 32-bit tokens, worked on in place, with the header naming the current copy.
// The frame parity of the double buffers is local to a launch; the state is stored from whichever copy the launch ended on.
//
// Contextual biasing (halo_ctc_prefix_beam_biased, halo_ctc_prefix_beam_advance_biased, haloop_amd/biasing.py ContextGraph; DESIGN.md
// 3.3ac) is the same frame body with BIASED set: a member carries the state c of a phrase automaton and the boost z it holds, a
// candidate ranks by its CTC mass + its boost, and pb / pnb stay CTC masses.  The extension of j by k looks up col = columns[k],
// c' = next[c_j width + col], z' = z_j + gain[c_j width + col]; every index read from memory is clamped into its table first.  LDS: the
// members' c and z, twice (256 bytes static, in the BIASED instantiations alone), nothing dynamic: the budget above stands.  A thread
// holds the columns of its first PF classes in registers for the whole launch (they do not change with the frame) and every member's
// z + gain[c width + 0], the boost of an extension by a token in no phrase, per frame; the columns of further classes and the gains of
// tokens in a phrase come from L2, as do the W next states of the candidates taken.  No table is cached in LDS, so the launcher has no
// further dispatch: BIASED times the four above.  The unbiased instantiations compile to what they were.
#include <type_traits>

#include "halo_common.h"
#include "beam_common.h"

namespace {

using namespace beam;

constexpr int E_LDS_FLOATS = 8192;         // two frames of emissions in LDS: V <= 4096
constexpr int TOK_LDS_TOKENS = 12288;      // both copies of the beam's token rows in LDS as 16-bit tokens: 2 W capacity <= 12288
constexpr int PF = 4;                      // emissions of the next frame a thread holds in registers across a frame (V <= 1024: all of them)
constexpr int V_MAX = 1 << 26;             // positions W + j V + k stay below 2^31
constexpr int STREAM_BEGIN_BIT = 2;        // bit 1 of the per-stream flags (include/halo.h: bit 0 active, bit 1 begin, bit 2 final)

// the head of a row's carried state: the W records, the member count and (token rows in the state) the copy that is current
struct BeamRecords {
    float pb[BEAM_MAX], pnb[BEAM_MAX], sc[BEAM_MAX];
    int len[BEAM_MAX], last[BEAM_MAX];
    unsigned hash[BEAM_MAX], hprev[BEAM_MAX];
    int nb, copy, pad[14];
};
static_assert(sizeof(BeamRecords) == 512, "the token rows behind the records stay 16-byte aligned");

struct CtcPrefixBeamArgs {
    const float *e;                        // [T][N][V] log-probabilities, strides st (frame) and sn (row), unit class stride
    long st, sn;
    int T, V, W, cap;
    const int64_t *il;                     // [N] frames of each row (NULL: T), clamped to [0, T] here
    int *ws;                               // token rows [N][2][W][cap] when they do not fit LDS
    int64_t *tokens, *lengths, *counts;    // [N][W][cap], [N][W], [N]
    float *scores;                         // [N][W]
    // the carried search only
    const int *nf;                         // [N] frames of each row in this launch (NULL: T), clamped to [0, T]
    const int *flags;                      // [N] per-stream flags (NULL: no row begins)
    unsigned char *state;                  // [N][state_bytes]
    size_t state_bytes;
    // the biased search only (include/halo.h: the device form of a phrase automaton)
    const int *columns, *next;             // [V] the column of every token (0: in no phrase); [states][width] the transitions
    const float *gain;                     // [states][width] what a transition adds to the boost
    int states, width;
    float *boosts;                         // [N][W] out: the boost in every score (0 where absent)
    int64_t *cstates;                      // [N][W] out: the automaton state of every hypothesis (-1 where absent)
};

// behind the BeamRecords of a biased row's carried state
struct BiasRecords {
    int c[BEAM_MAX];
    float z[BEAM_MAX];
};
static_assert(sizeof(BiasRecords) == 128, "the token rows behind the records stay 16-byte aligned");

template <bool STAGED, bool TOK_LDS, bool CARRIED, bool BIASED>
__global__ __launch_bounds__(BEAM_THREADS) void ctc_prefix_beam_kernel(const CtcPrefixBeamArgs p) {
    using tok_t = typename std::conditional<TOK_LDS, unsigned short, int>::type;
    // the beam, twice (frame parity): masses, score, length, last token (0: the empty prefix), hash of the prefix and of the prefix without
    // its last token
    __shared__ float s_pb[2][BEAM_MAX], s_pnb[2][BEAM_MAX], s_sc[2][BEAM_MAX];
    __shared__ int s_len[2][BEAM_MAX], s_last[2][BEAM_MAX], s_nb[2];
    __shared__ unsigned s_hash[2][BEAM_MAX], s_hprev[2][BEAM_MAX];
    // the frame: totals, the stay candidates' masses, the shortlist (bit j of word s), the member whose extension merged into s (-1: none)
    __shared__ float s_tot[BEAM_MAX], s_spb[BEAM_MAX], s_spnb[BEAM_MAX], sel_sc[BEAM_MAX];
    __shared__ int s_short[BEAM_MAX], s_mj[BEAM_MAX], sel_pos[BEAM_MAX];
    __shared__ FirstScratch s_first;
    // BIASED: every member's automaton state and boost, twice (frame parity); used by, and allocated in, those instantiations alone
    __shared__ int s_c[2][BEAM_MAX];
    __shared__ float s_z[2][BEAM_MAX];
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, W = p.W, V = p.V, cap = p.cap;
    int L;
    bool begin = true;                                                 // from the empty prefix (the whole-utterance search: always)
    if constexpr (CARRIED) {
        L = max(0, min(p.nf ? p.nf[n] : p.T, p.T));
        begin = p.flags && (p.flags[n] & STREAM_BEGIN_BIT);
        if (L == 0 && !begin) return;                                  // (uniform) the row does not take part: nothing of it is written
    } else {
        L = max(0, min(p.il ? (int)p.il[n] : p.T, p.T));
    }
    BeamRecords *st = nullptr;
    BiasRecords *stb = nullptr;                                        // BIASED: behind the records
    unsigned char *st_rows = nullptr;                                  // the state's token rows, behind its header
    unsigned short *st_tok = nullptr;                                  // TOK_LDS: the state's one copy of the token rows [W][cap]
    if constexpr (CARRIED) {
        st = reinterpret_cast<BeamRecords *>(p.state + (size_t)n * p.state_bytes);
        stb = reinterpret_cast<BiasRecords *>(st + 1);
        st_rows = reinterpret_cast<unsigned char *>(st + 1) + (BIASED ? sizeof(BiasRecords) : 0);
        st_tok = reinterpret_cast<unsigned short *>(st_rows);
    }
    // a column or a state read from memory, clamped into its table (a graph's tables hold nothing else; a state that no launch wrote may)
    auto column_of = [&](int k) { return max(0, min(p.columns[k], p.width - 1)); };
    auto state_in = [&](int c) { return max(0, min(c, p.states - 1)); };
    const float *rows = p.e + (long)n * p.sn;
    float *s_e = reinterpret_cast<float *>(dyn);                       // STAGED: [2][V]
    tok_t *tok;                                                        // [2][W][cap]
    if constexpr (TOK_LDS) tok = reinterpret_cast<tok_t *>(dyn + (STAGED ? 2 * (size_t)V * sizeof(float) : 0));
    else if constexpr (CARRIED) tok = reinterpret_cast<tok_t *>(st_rows);
    else tok = reinterpret_cast<tok_t *>(p.ws) + (size_t)n * 2 * W * cap;
    auto tok_row = [&](int copy, int j) { return tok + ((size_t)copy * W + j) * cap; };

    int cur = 0;
    if (begin) {
        if (tid < BEAM_MAX) {                                          // the empty prefix: every alignment of no frames ends "in blank"
            s_pb[0][tid] = tid == 0 ? 0.f : -INFINITY; s_pnb[0][tid] = -INFINITY; s_sc[0][tid] = tid == 0 ? 0.f : -INFINITY;
            s_len[0][tid] = 0; s_last[0][tid] = 0; s_hash[0][tid] = HASH_EMPTY; s_hprev[0][tid] = 0u;
            s_short[tid] = 0;
            if (tid == 0) s_nb[0] = 1;
            if constexpr (BIASED) { s_c[0][tid] = 0; s_z[0][tid] = 0.f; }
        }
    } else if constexpr (CARRIED) {                                    // the beam the last launch left
        if constexpr (!TOK_LDS) cur = st->copy & 1;                    // (the token rows stay where they are)
        if (tid < BEAM_MAX) {
            s_pb[cur][tid] = st->pb[tid]; s_pnb[cur][tid] = st->pnb[tid]; s_sc[cur][tid] = st->sc[tid];
            // counts, lengths and tokens index memory: a state that no launch wrote (a row that never began) stays inside its own rows
            s_len[cur][tid] = max(0, min(st->len[tid], cap)); s_last[cur][tid] = max(0, min(st->last[tid], V - 1));
            s_hash[cur][tid] = st->hash[tid]; s_hprev[cur][tid] = st->hprev[tid];
            s_short[tid] = 0;
            if (tid == 0) s_nb[cur] = max(0, min(st->nb, W));
            if constexpr (BIASED) { s_c[cur][tid] = state_in(stb->c[tid]); s_z[cur][tid] = stb->z[tid]; }
        }
        if constexpr (TOK_LDS) {
            const int nb0 = min(st->nb, W);
            for (int r = wave; r < nb0; r += BEAM_WAVES) {
                const int lr = min(st->len[r], cap);
                for (int x = lane; x < lr; x += 64) tok_row(0, r)[x] = st_tok[(size_t)r * cap + x];
            }
        }
    }
    if constexpr (STAGED)
        if (L > 0)
            for (int k = tid; k < V; k += BEAM_THREADS) s_e[k] = rows[k];
    // BIASED: the columns of this thread's first PF classes, for every frame (the address clamped like the emissions' below)
    int colv[PF];
    if constexpr (BIASED) {
#pragma unroll
        for (int i = 0; i < PF; ++i) colv[i] = column_of(min(1 + tid + i * BEAM_THREADS, V - 1));
    }
    __syncthreads();

    for (int t = 0; t < L; ++t) {
        const float *row = rows + (long)t * p.st;
        const int eb = (t & 1) * V;
        auto em = [&](int k) {
            if constexpr (STAGED) return s_e[eb + k];
            else return row[k];
        };
        // the next frame's emissions are requested here, before this frame's rounds; the addresses are clamped into the row's own frames
        // and classes so that every load is issued unconditionally (what a clamp duplicates is dropped where it would be stored)
        float nx[PF];
        if constexpr (STAGED) {
            const float *next = rows + (long)min(t + 1, L - 1) * p.st;
#pragma unroll
            for (int i = 0; i < PF; ++i) nx[i] = next[min(tid + i * BEAM_THREADS, V - 1)];
        }
        const int nb = s_nb[cur];
        // ---- 1. totals and stay candidates; the shortlist of (s, j) with y_s possibly y_j + [last_s]
        if (tid < BEAM_MAX) {
            s_mj[tid] = -1;
            if (tid < nb) {
                const float pb = s_pb[cur][tid], pnb = s_pnb[cur][tid], tot = logaddexpf_(pb, pnb);
                s_tot[tid] = tot;
                s_spb[tid] = tot + em(0);
                s_spnb[tid] = s_len[cur][tid] > 0 ? pnb + em(s_last[cur][tid]) : -INFINITY;
            }
        }
        shortlist_pair(nb, s_len[cur], s_hash[cur], s_hprev[cur], s_short);
        __syncthreads();
        // ---- 2. the merge: wave w compares the tokens of the shortlisted pairs of s = w, w + 4, ...
        for (int s = wave; s < nb; s += BEAM_WAVES) {
            const int j = merged_member(s, s_short[s], s_len[cur], [&](int m) { return tok_row(cur, m); });
            if (j >= 0 && lane == 0) {
                const int k = s_last[cur][s];
                s_mj[s] = j;
                s_spnb[s] = logaddexpf_(s_spnb[s], em(k) + (k == s_last[cur][j] ? s_pb[cur][j] : s_tot[j]));
            }
        }
        __syncthreads();
        // ---- 3. the W best candidates, one per round.  A thread owns the stay candidate tid and the extensions by its classes k = 1 + tid,
        //         1 + tid + 256, ... of every member, whose scalars it holds in registers, and keeps the first of its candidates in the order
        //         behind the last one taken; only the thread that owned the one just taken looks for its next (positions are unique).
        //         BIASED: a candidate ranks by its CTC mass + its boost, and is a candidate by its mass (-inf: never taken).
        const float stay_mass = tid < nb ? logaddexpf_(s_spb[tid], s_spnb[tid]) : -INFINITY;
        float stay_sc = stay_mass;
        if constexpr (BIASED) stay_sc = tid < nb ? stay_mass + s_z[cur][tid] : -INFINITY;
        float totv[BEAM_MAX], pbv[BEAM_MAX];
        int lastv[BEAM_MAX];
#pragma unroll
        for (int j = 0; j < BEAM_MAX; ++j) {
            const bool open = j < nb && s_len[cur][j] < cap;            // else no extension: every score of j is -inf
            totv[j] = open ? s_tot[j] : -INFINITY; pbv[j] = open ? s_pb[cur][j] : -INFINITY; lastv[j] = open ? s_last[cur][j] : -1;
        }
        // BIASED: every member's boost, the first entry of its row of the tables and its boost after a token in no phrase (column 0)
        float zv[BEAM_MAX], zdef[BEAM_MAX];
        int rowv[BEAM_MAX];
        if constexpr (BIASED) {
#pragma unroll
            for (int j = 0; j < BEAM_MAX; ++j) {
                const bool live = j < nb;
                zv[j] = live ? s_z[cur][j] : 0.f; rowv[j] = live ? s_c[cur][j] * p.width : 0;
                zdef[j] = zv[j] + p.gain[rowv[j]];
            }
        }
        // the extensions merged away, one per stay candidate at most: (member, class), class -1 for none; bit k % 64 of merged_k says
        // that some extension by a class congruent to k was (a filter in front of the exact comparison)
        int gone_j[BEAM_MAX], gone_k[BEAM_MAX];
        unsigned long long merged_k = 0;
#pragma unroll
        for (int s = 0; s < BEAM_MAX; ++s) {
            gone_j[s] = s_mj[s];                                        // (-1 in slots without a member too)
            gone_k[s] = gone_j[s] >= 0 ? s_last[cur][s] : -1;
            if (gone_j[s] >= 0) merged_k |= 1ull << (gone_k[s] & 63);
        }
        auto first_behind = [&](float psc, int ppos, float &bsc, int &bpos) {
            bsc = -INFINITY; bpos = NO_CANDIDATE;
            if (stay_mass > -INFINITY && before(psc, ppos, stay_sc, tid)) { bsc = stay_sc; bpos = tid; }
            int i = 0;
#pragma nounroll                                                        // (BIASED: unrolled, the members' gain loads of two classes cost 500 VGPRs)
            for (int k = 1 + tid; k < V; k += BEAM_THREADS, ++i) {
                const float ek = em(k);
                int col = 0;
                if constexpr (BIASED) {
                    if (i < PF) {
#pragma unroll
                        for (int q = 0; q < PF; ++q) col = i == q ? colv[q] : col;
                    } else {
                        col = column_of(k);
                    }
                }
                unsigned gone = 0;                                      // bit j: the extension of j by k was merged away
                if ((merged_k >> (k & 63)) & 1) {
#pragma unroll
                    for (int s = 0; s < BEAM_MAX; ++s) gone |= gone_k[s] == k ? 1u << (gone_j[s] & (BEAM_MAX - 1)) : 0u;
                }
#pragma unroll
                for (int j = 0; j < BEAM_MAX; ++j) {
                    const float mass = ek + (k == lastv[j] ? pbv[j] : totv[j]);
                    float sc = mass;
                    if constexpr (BIASED) {
                        if (!(mass > -INFINITY)) continue;              // (nothing is looked up for a candidate that is none)
                        sc = mass + (col ? zv[j] + p.gain[rowv[j] + col] : zdef[j]);
                    }
                    const int pos = W + j * V + k;
                    if (((gone >> j) & 1) || !(mass > -INFINITY) || !before(psc, ppos, sc, pos) || !before(sc, pos, bsc, bpos)) continue;
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
            if (bpos == NO_CANDIDATE) break;                            // (uniform) no candidate is left
            if (tid == 0) { sel_sc[r] = bsc; sel_pos[r] = bpos; }
            nsel = r + 1;
            if (lpos == bpos && r + 1 < W) first_behind(bsc, bpos, lsc, lpos);
        }
        __syncthreads();
        // ---- 4. the new beam, in the order taken, into the other copy
        const int nxt = cur ^ 1;
        if (tid < BEAM_MAX) {
            s_short[tid] = 0;
            if (tid < nsel) {
                const int pos = sel_pos[tid];
                if (pos < W) {
                    s_pb[nxt][tid] = s_spb[pos]; s_pnb[nxt][tid] = s_spnb[pos];
                    s_len[nxt][tid] = s_len[cur][pos]; s_last[nxt][tid] = s_last[cur][pos];
                    s_hash[nxt][tid] = s_hash[cur][pos]; s_hprev[nxt][tid] = s_hprev[cur][pos];
                    if constexpr (BIASED) { s_c[nxt][tid] = s_c[cur][pos]; s_z[nxt][tid] = s_z[cur][pos]; }
                } else {
                    const int par = (pos - W) / V, k = (pos - W) % V;
                    if constexpr (BIASED) {                             // the mass and the boost again, by the operations that ranked it
                        const int at = s_c[cur][par] * p.width + column_of(k);
                        s_c[nxt][tid] = state_in(p.next[at]); s_z[nxt][tid] = s_z[cur][par] + p.gain[at];
                        s_pb[nxt][tid] = -INFINITY; s_pnb[nxt][tid] = em(k) + (k == s_last[cur][par] ? s_pb[cur][par] : s_tot[par]);
                    } else {
                        s_pb[nxt][tid] = -INFINITY; s_pnb[nxt][tid] = sel_sc[tid];
                    }
                    s_len[nxt][tid] = s_len[cur][par] + 1; s_last[nxt][tid] = k;
                    s_hprev[nxt][tid] = s_hash[cur][par]; s_hash[nxt][tid] = hash_append(s_hash[cur][par], k);
                }
                s_sc[nxt][tid] = sel_sc[tid];
            }
            if (tid == 0) s_nb[nxt] = nsel;
        }
        for (int r = wave; r < nsel; r += BEAM_WAVES) {                 // wave w copies the token rows of slots w, w + 4, ...
            const int pos = sel_pos[r], par = pos < W ? pos : (pos - W) / V, k = pos < W ? 0 : (pos - W) % V, lp = s_len[cur][par];
            for (int x = lane; x < lp + (k != 0); x += 64) child_token(tok_row(nxt, r), tok_row(cur, par), x, lp, k);
        }
        if constexpr (STAGED) {
            if (t + 1 < L) {
                float *ne = s_e + (eb ^ V);                             // the other frame's buffer (eb is 0 or V)
#pragma unroll
                for (int i = 0; i < PF; ++i) {
                    const int k = tid + i * BEAM_THREADS;
                    if (k < V) ne[k] = nx[i];
                }
                const float *next = row + p.st;
                for (int k = tid + PF * BEAM_THREADS; k < V; k += BEAM_THREADS) ne[k] = next[k];
            }
        }
        __syncthreads();
        cur = nxt;
    }

    // the beam after the last frame, in its order; a row of no frames keeps the empty prefix, score 0
    const int nb = s_nb[cur];
    const long base = (long)n * W;
    if (tid < W) {
        p.lengths[base + tid] = tid < nb ? s_len[cur][tid] : -1;
        p.scores[base + tid] = tid < nb ? s_sc[cur][tid] : -INFINITY;
        if constexpr (BIASED) {
            p.boosts[base + tid] = tid < nb ? s_z[cur][tid] : 0.f;
            p.cstates[base + tid] = tid < nb ? (int64_t)s_c[cur][tid] : -1;
        }
    }
    if (tid == 0) p.counts[n] = nb;
    for (int idx = tid; idx < W * cap; idx += BEAM_THREADS) {
        const int r = idx / cap, x = idx % cap;
        p.tokens[base * cap + idx] = (r < nb && x < s_len[cur][r]) ? (int64_t)tok_row(cur, r)[x] : -1;
    }
    if constexpr (CARRIED) {                                           // the state, from the copy this launch ended on
        if (tid < BEAM_MAX) {
            const bool live = tid < nb;
            st->pb[tid] = live ? s_pb[cur][tid] : -INFINITY; st->pnb[tid] = live ? s_pnb[cur][tid] : -INFINITY;
            st->sc[tid] = live ? s_sc[cur][tid] : -INFINITY;
            st->len[tid] = live ? s_len[cur][tid] : 0; st->last[tid] = live ? s_last[cur][tid] : 0;
            st->hash[tid] = live ? s_hash[cur][tid] : HASH_EMPTY; st->hprev[tid] = live ? s_hprev[cur][tid] : 0u;
            if (tid == 0) { st->nb = nb; st->copy = TOK_LDS ? 0 : cur; }
            if constexpr (BIASED) { stb->c[tid] = live ? s_c[cur][tid] : 0; stb->z[tid] = live ? s_z[cur][tid] : 0.f; }
        }
        if constexpr (TOK_LDS) {
            for (int r = wave; r < nb; r += BEAM_WAVES)
                for (int x = lane; x < s_len[cur][r]; x += 64) st_tok[(size_t)r * cap + x] = tok_row(cur, r)[x];
        }
    }
}

bool tokens_in_lds(int V, int beam, int capacity) { return V <= 65536 && 2 * (long)beam * capacity <= TOK_LDS_TOKENS; }

bool valid_shape(int N, int T, int V, int beam, int capacity) {
    return N > 0 && T > 0 && V >= 2 && V <= V_MAX && beam >= 1 && beam <= BEAM_MAX && capacity >= 1 && capacity <= T;
}

// the carried search: capacity is the longest hypothesis of the stream, whatever the frames of one launch
bool valid_stream_shape(int V, int beam, int capacity) {
    return V >= 2 && V <= V_MAX && beam >= 1 && beam <= BEAM_MAX && capacity >= 1 && capacity <= HALO_CTC_PREFIX_BEAM_MAX_CAPACITY;
}

template <bool CARRIED, bool BIASED>
void launch(const CtcPrefixBeamArgs &a, int N, bool staged, bool tok_lds, hipStream_t stream) {
    const size_t lds = (staged ? 2 * (size_t)a.V * sizeof(float) : 0) + (tok_lds ? 2 * (size_t)a.W * a.cap * sizeof(unsigned short) : 0);
    const dim3 grid((unsigned)N), block(BEAM_THREADS);
    if (staged && tok_lds) hipLaunchKernelGGL((ctc_prefix_beam_kernel<true, true, CARRIED, BIASED>), grid, block, lds, stream, a);
    else if (staged) hipLaunchKernelGGL((ctc_prefix_beam_kernel<true, false, CARRIED, BIASED>), grid, block, lds, stream, a);
    else if (tok_lds) hipLaunchKernelGGL((ctc_prefix_beam_kernel<false, true, CARRIED, BIASED>), grid, block, lds, stream, a);
    else hipLaunchKernelGGL((ctc_prefix_beam_kernel<false, false, CARRIED, BIASED>), grid, block, lds, stream, a);
}

// the device form of a phrase automaton (include/halo.h): at least the root and column 0, tables that a 32-bit index reaches
bool valid_context(const int *columns, const int *next, const float *gain, int states, int width) {
    return columns && next && gain && states >= 1 && states <= HALO_CONTEXT_MAX_STATES && width >= 1 && (long)states * width <= 0x7fffffffL;
}

void no_context(CtcPrefixBeamArgs &a) {
    a.columns = nullptr; a.next = nullptr; a.gain = nullptr; a.states = 0; a.width = 0; a.boosts = nullptr; a.cstates = nullptr;
}

void set_context(CtcPrefixBeamArgs &a, const int *columns, const int *next, const float *gain, int states, int width, float *boosts,
                 int64_t *cstates) {
    a.columns = columns; a.next = next; a.gain = gain; a.states = states; a.width = width; a.boosts = boosts; a.cstates = cstates;
}

}  // namespace

extern "C" {

size_t halo_ctc_prefix_beam_workspace_bytes(int N, int T, int V, int beam, int capacity) {
    if (!valid_shape(N, T, V, beam, capacity) || tokens_in_lds(V, beam, capacity)) return 0;
    return (size_t)N * 2 * beam * capacity * sizeof(int);
}

int halo_ctc_prefix_beam(const float *emissions, long stride_t, long stride_n, int T, int N, int V, const int64_t *emission_lengths,
                         int beam, int capacity, void *workspace, int64_t *tokens, int64_t *lengths, float *scores, int64_t *counts,
                         halo_stream_t stream) {
    HALO_CHECK_ARG(emissions && tokens && lengths && scores && counts);
    HALO_CHECK_ARG(valid_shape(N, T, V, beam, capacity));
    const bool staged = 2 * (long)V <= E_LDS_FLOATS, tok_lds = tokens_in_lds(V, beam, capacity);
    HALO_CHECK_ARG(tok_lds || workspace);
    CtcPrefixBeamArgs a;
    a.e = emissions; a.st = stride_t; a.sn = stride_n; a.T = T; a.V = V; a.W = beam; a.cap = capacity; a.il = emission_lengths;
    a.ws = (int *)workspace; a.tokens = tokens; a.lengths = lengths; a.counts = counts; a.scores = scores;
    a.nf = nullptr; a.flags = nullptr; a.state = nullptr; a.state_bytes = 0;
    no_context(a);
    launch<false, false>(a, N, staged, tok_lds, (hipStream_t)stream);
    return halo_launch_status();
}

int halo_ctc_prefix_beam_biased(const float *emissions, long stride_t, long stride_n, int T, int N, int V, const int64_t *emission_lengths,
                                int beam, int capacity, void *workspace, int64_t *tokens, int64_t *lengths, float *scores, int64_t *counts,
                                const int *ctx_columns, const int *ctx_next, const float *ctx_gain, int ctx_states, int ctx_width,
                                float *boosts, int64_t *states, halo_stream_t stream) {
    HALO_CHECK_ARG(emissions && tokens && lengths && scores && counts && boosts && states);
    HALO_CHECK_ARG(valid_shape(N, T, V, beam, capacity));
    HALO_CHECK_ARG(valid_context(ctx_columns, ctx_next, ctx_gain, ctx_states, ctx_width));
    const bool staged = 2 * (long)V <= E_LDS_FLOATS, tok_lds = tokens_in_lds(V, beam, capacity);
    HALO_CHECK_ARG(tok_lds || workspace);
    CtcPrefixBeamArgs a;
    a.e = emissions; a.st = stride_t; a.sn = stride_n; a.T = T; a.V = V; a.W = beam; a.cap = capacity; a.il = emission_lengths;
    a.ws = (int *)workspace; a.tokens = tokens; a.lengths = lengths; a.counts = counts; a.scores = scores;
    a.nf = nullptr; a.flags = nullptr; a.state = nullptr; a.state_bytes = 0;
    set_context(a, ctx_columns, ctx_next, ctx_gain, ctx_states, ctx_width, boosts, states);
    launch<false, true>(a, N, staged, tok_lds, (hipStream_t)stream);
    return halo_launch_status();
}

size_t halo_ctc_prefix_beam_state_bytes(int V, int beam, int capacity) {
    if (!valid_stream_shape(V, beam, capacity)) return 0;
    const size_t rows = tokens_in_lds(V, beam, capacity) ? (size_t)beam * capacity * sizeof(unsigned short)
                                                         : 2 * (size_t)beam * capacity * sizeof(int);
    return sizeof(BeamRecords) + (rows + 15) / 16 * 16;
}

int halo_ctc_prefix_beam_advance(const float *emissions, long stride_t, long stride_n, int T, int N, int V, const int *n_frames,
                                 const int *flags, int beam, int capacity, void *state, int64_t *tokens, int64_t *lengths, float *scores,
                                 int64_t *counts, halo_stream_t stream) {
    HALO_CHECK_ARG(emissions && state && tokens && lengths && scores && counts);
    HALO_CHECK_ARG(N > 0 && T > 0 && valid_stream_shape(V, beam, capacity));
    CtcPrefixBeamArgs a;
    a.e = emissions; a.st = stride_t; a.sn = stride_n; a.T = T; a.V = V; a.W = beam; a.cap = capacity; a.il = nullptr;
    a.ws = nullptr; a.tokens = tokens; a.lengths = lengths; a.counts = counts; a.scores = scores;
    a.nf = n_frames; a.flags = flags; a.state = (unsigned char *)state; a.state_bytes = halo_ctc_prefix_beam_state_bytes(V, beam, capacity);
    no_context(a);
    launch<true, false>(a, N, 2 * (long)V <= E_LDS_FLOATS, tokens_in_lds(V, beam, capacity), (hipStream_t)stream);
    return halo_launch_status();
}

size_t halo_ctc_prefix_beam_biased_state_bytes(int V, int beam, int capacity) {
    const size_t plain = halo_ctc_prefix_beam_state_bytes(V, beam, capacity);
    return plain ? plain + sizeof(BiasRecords) : 0;
}

int halo_ctc_prefix_beam_advance_biased(const float *emissions, long stride_t, long stride_n, int T, int N, int V, const int *n_frames,
                                        const int *flags, int beam, int capacity, void *state, int64_t *tokens, int64_t *lengths,
                                        float *scores, int64_t *counts, const int *ctx_columns, const int *ctx_next, const float *ctx_gain,
                                        int ctx_states, int ctx_width, float *boosts, int64_t *states, halo_stream_t stream) {
    HALO_CHECK_ARG(emissions && state && tokens && lengths && scores && counts && boosts && states);
    HALO_CHECK_ARG(N > 0 && T > 0 && valid_stream_shape(V, beam, capacity));
    HALO_CHECK_ARG(valid_context(ctx_columns, ctx_next, ctx_gain, ctx_states, ctx_width));
    CtcPrefixBeamArgs a;
    a.e = emissions; a.st = stride_t; a.sn = stride_n; a.T = T; a.V = V; a.W = beam; a.cap = capacity; a.il = nullptr;
    a.ws = nullptr; a.tokens = tokens; a.lengths = lengths; a.counts = counts; a.scores = scores;
    a.nf = n_frames; a.flags = flags; a.state = (unsigned char *)state;
    a.state_bytes = halo_ctc_prefix_beam_biased_state_bytes(V, beam, capacity);
    set_context(a, ctx_columns, ctx_next, ctx_gain, ctx_states, ctx_width, boosts, states);
    launch<true, true>(a, N, 2 * (long)V <= E_LDS_FLOATS, tokens_in_lds(V, beam, capacity), (hipStream_t)stream);
    return halo_launch_status();
}

}  // extern "C"
