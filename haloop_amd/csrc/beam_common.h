// What the device beam searches share (csrc/rnnt_beam.hip, rnnt_lm_beam.hip, ctc_prefix_beam.hip, ctc_lm_beam.hip and
// dec_beam_select_kernel of decode_beam.hip): one workgroup of BEAM_THREADS threads per row keeps a beam of at most BEAM_MAX members in LDS and takes the W best of
// its W V candidates in W rounds, one per round: the first in the total order (score descending, candidate position ascending) behind the
// last one taken.  No list of candidates is built; each search scans its own candidates and hands every thread's first to
// first_in_workgroup().  The order and the merge rule are the contract of every n-best list the library returns: they are stated here,
// once.  Every piece is forced inline and keeps its float expressions whole and its sums in one order (the lane's stride, then the wave's
// butterfly), so a search computes the same bits whether a value is read back from LDS or recomputed, and no float goes through an atomic.
#pragma once
#include "halo_common.h"

namespace beam {

constexpr int BEAM_MAX = 16, BEAM_THREADS = 256, BEAM_WAVES = BEAM_THREADS / 64;     // (haloop_amd/ops.py BEAM_MAX)
constexpr int NO_CANDIDATE = 0x7fffffff;   // the position behind every candidate's: what a thread (a round) with nothing left holds

__device__ __forceinline__ float logaddexpf_(float a, float b) {
    const float m = fmaxf(a, b);
    return m == -INFINITY ? m : m + log1pf(expf(-fabsf(a - b)));
}

// (sc, pos) stands before (osc, opos) in the order (score descending, position ascending)
__device__ __forceinline__ bool before(float sc, int pos, float osc, int opos) { return sc > osc || (sc == osc && pos < opos); }

// ---- the round's reduction.  Every thread brings the first of its own candidates, (-inf, NO_CANDIDATE) for none, and leaves with the
// workgroup's first: a wave butterfly, one word pair per wave in LDS, one barrier, the pick among the waves.  The scratch is
// double-buffered by the round's parity, so one barrier per round is enough: a wave that runs ahead writes the other copy.  Called by the
// whole workgroup (it holds the barrier); NO_CANDIDATE comes back in every thread alike.
struct FirstScratch {
    float sc[2][BEAM_WAVES];
    int pos[2][BEAM_WAVES];
};

__device__ __forceinline__ void first_in_workgroup(FirstScratch &s, int round, float &bsc, int &bpos) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = round & 1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float osc = __shfl_xor(bsc, o, 64);
        const int opos = __shfl_xor(bpos, o, 64);
        if (before(osc, opos, bsc, bpos)) { bsc = osc; bpos = opos; }
    }
    if (lane == 0) { s.sc[b][wave] = bsc; s.pos[b][wave] = bpos; }
    __syncthreads();
    bsc = s.sc[b][0]; bpos = s.pos[b][0];
#pragma unroll
    for (int w = 1; w < BEAM_WAVES; ++w)
        if (before(s.sc[b][w], s.pos[b][w], bsc, bpos)) { bsc = s.sc[b][w]; bpos = s.pos[b][w]; }
}

// ---- a member's log-sum-exp over V, by one wave: logit(j, v) is the member's logit; `cache` (NULL: none) is the member's row of V
// floats in LDS, filled here (read back by this lane below, by the others after the caller's barrier).  The second pass reads what the
// caller's z(j, v) will read: the cache, or the same operations again.
template <class Logit>
__device__ __forceinline__ float wave_lse(int j, int V, float *cache, Logit logit) {
    const int lane = threadIdx.x & 63;
    float m = -INFINITY;
    for (int v = lane; v < V; v += 64) {
        const float x = logit(j, v);
        if (cache) cache[v] = x;
        m = fmaxf(m, x);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    float s = 0.f;
    if (cache) for (int v = lane; v < V; v += 64) s += expf(cache[v] - m);
    else for (int v = lane; v < V; v += 64) s += expf(logit(j, v) - m);
    return m + logf(wave_sum(s));
}

// ---- the CTC merge.  The extension of member j by k spells the prefix of stay candidate s exactly when y_s = y_j + [k].  A member
// carries a 32-bit hash of its prefix and of the prefix without its last token; thread (s, j) of the first BEAM_MAX^2 shortlists the
// pair (bit j of word s, one integer atomicOr: a bit set, whatever the order), and a wave compares the tokens, which alone decides.
constexpr unsigned HASH_EMPTY = 0x811C9DC5u;                           // of the empty prefix
__device__ __forceinline__ unsigned hash_append(unsigned h, int k) { return h * 0x9E3779B1u + (unsigned)k; }

__device__ __forceinline__ void shortlist_pair(int nb, const int *len, const unsigned *hash, const unsigned *hprev, int *shortlist) {
    const int s = threadIdx.x / BEAM_MAX, j = threadIdx.x % BEAM_MAX;
    if (s < nb && j < nb && len[s] == len[j] + 1 && hprev[s] == hash[j]) atomicOr(&shortlist[s], 1 << j);
}

// the member of the shortlist `mask` of s whose len[j] tokens are the first of s's (-1: none), uniform over the calling wave; row(j) is
// member j's token row.  Beam members are distinct, so no second j spells y_s[:-1]: the first match ends the search.
template <class Row>
__device__ __forceinline__ int merged_member(int s, int mask, const int *len, Row row) {
    const int lane = threadIdx.x & 63;
    while (mask) {                                                      // (uniform over the wave)
        const int j = __ffs(mask) - 1, lj = len[j];
        mask &= mask - 1;
        const auto *ts = row(s), *tj = row(j);
        bool differ = false;
        for (int x = lane; x < lj; x += 64) differ = differ || ts[x] != tj[x];
        if (!__any(differ)) return j;
    }
    return -1;
}

// ---- a new member's token row: its parent's lp tokens, then k at lp when k is a label (not a blank, a stay or an end mark; then lp is
// below the capacity: only such members are extended).  child_token is element x of the rule; child_rows spreads the nsel rows of a beam
// in global memory over the workgroup: row r from row src[r], lengths len[parent], tokens k[r], label(r, parent) asked at x == lp only.
template <class Tok>
__device__ __forceinline__ void child_token(Tok *dst, const Tok *parent, int x, int lp, int k) {
    dst[x] = x < lp ? parent[x] : (Tok)k;
}

template <class Tok, class IsLabel>
__device__ __forceinline__ void child_rows(Tok *out, const Tok *in, long ld, int nsel, int capacity, const int *src, const int *len,
                                           const int *k, IsLabel label) {
    for (int idx = threadIdx.x; idx < nsel * capacity; idx += BEAM_THREADS) {
        const int r = idx / capacity, x = idx % capacity, par = src[r], lp = len[par];
        if (x < lp || (x == lp && label(r, par))) child_token(out + r * ld, in + par * ld, x, lp, k[r]);
    }
}

// ---- the gather of the LSTM state for the cell launches that follow a selection (halo_rnnt_lstm_cell): slot r of the row's W takes the
// cell inputs [wte[k[r]] | h of slot src[r]] and c of slot src[r], for every layer: 2 layers + 1 rows of H floats per slot, all of the
// row's copies spread over the threads, four loads in flight per thread before their stores.  `first` is the row's first slot.
// ZERO_ABSENT: a slot with src[r] < 0 (it steps nothing) has its rows zeroed instead, so that the cells read nothing unwritten.
struct StateGather {
    const float *wte;          // [V][H] the embedding
    const float *h_in, *c_in;  // [layers][slots][H] the state read
    float *xh, *c_out;         // [layers][slots][2 H] = x | h_prev of the cells; [layers][slots][H] the next state's c, before the cells
    int H, layers;
};

template <bool ZERO_ABSENT = false>
__device__ __forceinline__ void gather_state(const StateGather &g, long first, int W, const int *src, const int *k) {
    const int H4 = g.H / 4, per = 2 * g.layers + 1, total = W * per * H4;
    const long slots = (long)gridDim.x * W;
    constexpr int GU = 4;
    for (int i0 = threadIdx.x; i0 < total; i0 += GU * BEAM_THREADS) {
        f32x4 v[GU];
        f32x4 *dst[GU];
#pragma unroll
        for (int e = 0; e < GU; ++e) {
            const int idx = i0 + e * BEAM_THREADS;
            dst[e] = nullptr;
            if (idx >= total) continue;
            const int r = idx / (per * H4), q = idx / H4 % per, x = idx % H4, par = src[r];
            const bool zero = ZERO_ABSENT && par < 0;
            if (zero) v[e] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (q < g.layers) {                                         // h of layer q -> the h half of its [x | h] row
                if (!zero) v[e] = reinterpret_cast<const f32x4 *>(g.h_in + ((long)q * slots + first + par) * g.H)[x];
                dst[e] = reinterpret_cast<f32x4 *>(g.xh + ((long)q * slots + first + r) * 2 * g.H) + H4 + x;
            } else if (q < 2 * g.layers) {                              // c of layer q - layers
                if (!zero) v[e] = reinterpret_cast<const f32x4 *>(g.c_in + ((long)(q - g.layers) * slots + first + par) * g.H)[x];
                dst[e] = reinterpret_cast<f32x4 *>(g.c_out + ((long)(q - g.layers) * slots + first + r) * g.H) + x;
            } else {                                                    // the new token's embedding -> layer 0's x half
                if (!zero) v[e] = reinterpret_cast<const f32x4 *>(g.wte + (long)k[r] * g.H)[x];
                dst[e] = reinterpret_cast<f32x4 *>(g.xh + (first + r) * 2 * g.H) + x;
            }
        }
#pragma unroll
        for (int e = 0; e < GU; ++e)
            if (dst[e]) *dst[e] = v[e];
    }
}

}  // namespace beam
