// Forced alignment for gfx950: the max-plus twins of the CTC lattice (ctc.hip) and of the transducer lattice (lattice.hip), each with
// its back-pointers and a backtrace, one workgroup per utterance.  fp32 throughout, no atomics, finite launches: no
// workgroup reads what another workgroup writes.
//
// The recursion is a serial chain T (or T + U) long, so the emissions are taken off it: every thread keeps the emissions of its states
// for the next D frames in registers, requested one chunk of D frames ahead of their use (nothing of T x C is staged in LDS: T is
// bounded by the workspace alone).  A thread owns the states tid, tid + BLK, ..., PER of them; the previous frame's row lives in LDS
// (double buffered, one barrier per frame), or, when the lattice fits one wave, in a register of each lane with the s-1 / s-2
// neighbours taken by wave shuffles (no LDS and no barrier on the chain).
//
// Back-pointers are packed by wave ballots, so one lane of a wave stores the decisions of 64 states at once:
//   CTC         2 bits per (t, s): words[n][t][s / 64][2] uint64, bit s % 64 of word 0 / word 1 = bit 0 / bit 1 of the shift (0 stay,
//               1 from s-1, 2 from s-2)
//   transducer  1 bit per cell, indexed by anti-diagonal: words[n][t + u][u / 64] uint64, bit u % 64 set = the cell was entered by its
//               label arc from (t, u-1), clear = by the blank arc from (t-1, u)
// The backtrace is one thread's walk; the other threads stage the words of the next 64 frames (the walk moves down by at most two
// states, or one u, per frame, so three, or two, 64-state groups cover a chunk) from global memory into LDS in one parallel pass, which
// keeps the walk's own chain on LDS latency.  The CTC walk leaves its states in LDS and one thread per frame writes the outputs.
#include "halo_common.h"

namespace {

typedef unsigned long long u64;

constexpr int CHUNK = 64;        // frames (diagonals) of back-pointers staged per backtrace pass

struct CtcViterbiArgs {
    const float *lp;
    long stride_t, stride_n;
    int T, N, C;
    const int64_t *targets;
    long tg_stride;
    int S;
    const int64_t *il, *tl;
    u64 *words;                  // [N][T][G][2]
    int G;                       // ceil((2S+1) / 64)
    float *scores;               // [N]
    int64_t *alignments;         // [N][T]
    int *starts, *ends;          // [N][S]
};

template <int BLK, int PER, int D>
__global__ __launch_bounds__(BLK) void ctc_viterbi_kernel(const CtcViterbiArgs p) {
    extern __shared__ __attribute__((aligned(16))) float rows[];      // two rows of 2 + PER * BLK floats: [0], [1] stay -inf
    __shared__ u64 stage[CHUNK * 3 * 2];
    __shared__ int walk[2];                                           // the walker's state; whether the row is feasible
    __shared__ int path[CHUNK + 1];                                   // the states of a chunk's frames, latest first
    constexpr int R = PER * BLK + 2;
    constexpr bool ONE_WAVE = BLK == 64 && PER == 1;
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = p.T, S = p.S, G = p.G;
    const int64_t *tg = p.targets + (long)n * p.tg_stride;
    const int il = max(0, min(p.il ? (int)p.il[n] : T, T));
    const int tl = max(0, min((int)p.tl[n], S));
    const int states = 2 * tl + 1;
    const float *lp = p.lp + (long)n * p.stride_n;
    u64 *words = p.words + (size_t)n * T * G * 2;
    int64_t *ali = p.alignments + (long)n * T;
    int *starts = p.starts + (long)n * S, *ends = p.ends + (long)n * S;
    const float ninf = -INFINITY;

    for (int t = il + tid; t < T; t += BLK) ali[t] = -1;
    for (int u = tl + tid; u < S; u += BLK) starts[u] = ends[u] = -1;

    // this thread's states: the class whose emission each adds (-1: none -- past the target, or a label outside [0, C)) and whether the
    // skip arc s-2 -> s exists
    int cls[PER];
    unsigned skip = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int s = tid + k * BLK;
        cls[k] = -1;
        if (s < states) {
            const long lab = (s & 1) ? tg[s >> 1] : 0;
            if (lab >= 0 && lab < p.C) cls[k] = (int)lab;
            if ((s & 1) && s >= 3 && lab != tg[(s >> 1) - 1]) skip |= 1u << k;
        }
    }
    // every load is issued unconditionally, from an address inside the row's own frames (frame min(t, il - 1); class 0 for a state without
    // an emission), and a state without an emission drops the value where it is used: a load under a branch, or a select right behind
    // it, makes the compiler wait for each load where it is issued
    const int tmax = max(il - 1, 0);
    auto emission = [&](int t, int k) { return lp[(long)min(t, tmax) * p.stride_t + max(cls[k], 0)]; };

    float *prev = rows, *cur = rows + R;
    float vreg = ninf;                                                // ONE_WAVE: this lane's state
    if (tid < 2) prev[tid] = cur[tid] = ninf;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int s = tid + k * BLK;
        const float v = (s < 2 && il > 0 && cls[k] >= 0) ? emission(0, k) : ninf;
        if (ONE_WAVE) vreg = v; else prev[2 + s] = v;
    }
    float nxt[D][PER];
#pragma unroll
    for (int j = 0; j < D; ++j)
#pragma unroll
        for (int k = 0; k < PER; ++k) nxt[j][k] = emission(1 + j, k);
    if (!ONE_WAVE) __syncthreads();

    for (int t0 = 1; t0 < il; t0 += D) {
        float e[D][PER];
#pragma unroll
        for (int j = 0; j < D; ++j)
#pragma unroll
            for (int k = 0; k < PER; ++k) e[j][k] = nxt[j][k];
        // the next chunk's emissions are requested here, a whole chunk of frames before the chain needs them
#pragma unroll
        for (int j = 0; j < D; ++j)
#pragma unroll
            for (int k = 0; k < PER; ++k) nxt[j][k] = emission(t0 + D + j, k);
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const int t = t0 + j;
            if (t >= il) break;
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const int s = tid + k * BLK;
                float a, b, c;
                if (ONE_WAVE) {
                    a = vreg;
                    b = __shfl_up(vreg, 1, 64);
                    c = __shfl_up(vreg, 2, 64);
                    if (lane < 1) b = ninf;
                    if (lane < 2) c = ninf;
                } else {
                    a = prev[2 + s]; b = prev[1 + s]; c = prev[s];
                }
                // smallest shift among equal predecessors: stay, then s-1, then s-2
                float best = a;
                int shift = 0;
                if (b > best) { best = b; shift = 1; }
                if (((skip >> k) & 1) && c > best) { best = c; shift = 2; }
                const float v = cls[k] >= 0 ? best + e[j][k] : ninf;
                if (ONE_WAVE) vreg = v; else cur[2 + s] = v;
                const u64 lo = __ballot(shift & 1), hi = __ballot(shift >> 1);
                const int g = wave + k * (BLK / 64);
                if (lane == 0 && g < G) {
                    u64 *w = words + ((size_t)t * G + g) * 2;
                    w[0] = lo; w[1] = hi;
                }
            }
            if (!ONE_WAVE) {
                __syncthreads();
                float *tmp = prev; prev = cur; cur = tmp;
            }
        }
    }
    if (ONE_WAVE) prev[2 + tid] = vreg;
    __syncthreads();                                                  // the last row, and every back-pointer word, is visible to the block

    if (tid == 0) {
        float score;
        int s_end = 2 * tl;
        if (il == 0) score = tl == 0 ? 0.f : ninf;
        else {
            const float a = prev[2 + 2 * tl], b = tl > 0 ? prev[1 + 2 * tl] : ninf;
            score = a;
            if (b > a) { score = b; s_end = 2 * tl - 1; }             // equal: the final blank
        }
        p.scores[n] = score;
        walk[0] = s_end;
        walk[1] = score > ninf;
    }
    __syncthreads();
    if (!walk[1]) {                                                   // infeasible: nothing is aligned
        for (int t = tid; t < il; t += BLK) ali[t] = -1;
        for (int u = tid; u < tl; u += BLK) starts[u] = ends[u] = -1;
        return;
    }
    // The walk itself touches LDS only: thread 0 writes the chunk's states, then one thread per frame turns its state into the frame's
    // label and the token boundaries (the loads of targets and the stores run in parallel, off the walk's chain).
    int later = -1;                                                   // the state one frame after the chunk's first (uniform)
    for (int thi = il - 1; thi >= 0; thi -= CHUNK) {
        const int g0 = walk[0] >> 6;
        for (int idx = tid; idx < CHUNK * 3; idx += BLK) {
            const int j = idx / 3, r = idx % 3, t = thi - j, g = g0 - r;
            if (t >= 1 && g >= 0) {
                const u64 *w = words + ((size_t)t * G + g) * 2;
                stage[idx * 2] = w[0]; stage[idx * 2 + 1] = w[1];
            }
        }
        __syncthreads();
        if (tid == 0) {
            int s = walk[0];
            for (int j = 0; j < CHUNK; ++j) {
                const int t = thi - j;
                path[j] = s;
                if (t <= 0) break;
                const int at = (j * 3 + (g0 - (s >> 6))) * 2, bit = s & 63;
                s -= (int)((stage[at] >> bit) & 1) | ((int)((stage[at + 1] >> bit) & 1) << 1);
                path[j + 1] = s;                                      // the state at frame t - 1 (the next chunk's first, after the last step)
            }
            walk[0] = s;
        }
        __syncthreads();
        for (int j = tid; j < CHUNK; j += BLK) {
            const int t = thi - j;
            if (t < 0) break;
            const int st = path[j], u = st >> 1;
            ali[t] = (st & 1) ? tg[u] : 0;
            if (st & 1) {
                if (st != (j == 0 ? later : path[j - 1])) ends[u] = t;
                if (t == 0 || path[j + 1] != st) starts[u] = t;
            }
        }
        later = path[CHUNK - 1];
        __syncthreads();
    }
}

struct TransducerViterbiArgs {
    const float *joint;          // [N][T][U1][K]
    int N, T, U1, K;
    const int64_t *targets;      // [N][U1 - 1]
    const int *j_len, *t_len;
    u64 *words;                  // [N][T + U1 - 1][W]
    int W;                       // ceil(U1 / 64)
    float *scores;               // [N]
    int *frames;                 // [N][U1 - 1]
};

template <int BLK, int PER, int D>
__global__ __launch_bounds__(BLK) void transducer_viterbi_kernel(const TransducerViterbiArgs p) {
    extern __shared__ __attribute__((aligned(16))) float rows[];      // two diagonals of 1 + PER * BLK floats: [0] stays -inf
    __shared__ u64 stage[CHUNK * 2];
    __shared__ int walk[2];
    constexpr int R = PER * BLK + 1;
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = p.T, U1 = p.U1, K = p.K, W = p.W;
    const float *jn = p.joint + (size_t)n * T * U1 * K;
    const int64_t *tg = p.targets + (long)n * (U1 - 1);
    const int Tn = max(0, min(p.j_len[n], T)), Un = max(0, min(p.t_len[n], U1 - 1));
    u64 *words = p.words + (size_t)n * (T + U1 - 1) * W;
    int *frames = p.frames + (long)n * (U1 - 1);
    const float ninf = -INFINITY;

    for (int u = Un + tid; u < U1 - 1; u += BLK) frames[u] = -1;
    if (Tn == 0) {
        for (int u = tid; u < Un; u += BLK) frames[u] = -1;
        if (tid == 0) p.scores[n] = ninf;
        return;
    }
    // this thread's columns u: the class of the label arc into u from u-1 (-1: none: u = 0, u > Un, or a label outside [0, K))
    int cls[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int u = tid + k * BLK;
        cls[k] = -1;
        if (u >= 1 && u <= Un) {
            const long y = tg[u - 1];
            if (y >= 0 && y < K) cls[k] = (int)y;
        }
    }
    // the two arcs into cell (t, u) = (d - u, u) of diagonal d; cells outside the lengths are never read
    // Every load is issued unconditionally, from a cell inside the lengths (the indices are clamped), and an arc that does not exist drops
    // the value where it is used: a load under a branch, or a select right behind it, makes the compiler wait for each load where it is
    // issued.
    auto blank_in = [&](int d, int k) {
        const int u = tid + k * BLK, t = d - u;
        return jn[((size_t)min(max(t - 1, 0), Tn - 1) * U1 + min(u, Un)) * K];
    };
    auto label_in = [&](int d, int k) {
        const int u = tid + k * BLK, t = d - u;
        return jn[((size_t)min(max(t, 0), Tn - 1) * U1 + min(max(u - 1, 0), Un)) * K + max(cls[k], 0)];
    };

    float *prev = rows, *cur = rows + R;
    if (tid == 0) prev[0] = cur[0] = ninf;
#pragma unroll
    for (int k = 0; k < PER; ++k) prev[1 + tid + k * BLK] = (tid + k * BLK == 0) ? 0.f : ninf;      // diagonal 0: cell (0, 0)
    float nb[D][PER], ny[D][PER];
#pragma unroll
    for (int j = 0; j < D; ++j)
#pragma unroll
        for (int k = 0; k < PER; ++k) { nb[j][k] = blank_in(1 + j, k); ny[j][k] = label_in(1 + j, k); }
    __syncthreads();

    const int dlast = Tn - 1 + Un;
    for (int d0 = 1; d0 <= dlast; d0 += D) {
        float eb[D][PER], ey[D][PER];
#pragma unroll
        for (int j = 0; j < D; ++j)
#pragma unroll
            for (int k = 0; k < PER; ++k) { eb[j][k] = nb[j][k]; ey[j][k] = ny[j][k]; }
        // the next chunk of diagonals is requested here, before this chunk's maxima
#pragma unroll
        for (int j = 0; j < D; ++j)
#pragma unroll
            for (int k = 0; k < PER; ++k) { nb[j][k] = blank_in(d0 + D + j, k); ny[j][k] = label_in(d0 + D + j, k); }
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const int d = d0 + j;
            if (d > dlast) break;
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const int u = tid + k * BLK;
                const int t = d - u;
                const bool inside = t >= 0 && t < Tn;
                const float a = (inside && t >= 1 && u <= Un) ? prev[1 + u] + eb[j][k] : ninf;      // from (t-1, u) by blank
                const float b = (inside && cls[k] >= 0) ? prev[u] + ey[j][k] : ninf;                // from (t, u-1) by the label
                const int from_label = b > a;                         // equal: the blank predecessor
                cur[1 + u] = from_label ? b : a;
                const u64 bits = __ballot(from_label);
                const int g = wave + k * (BLK / 64);
                if (lane == 0 && g < W) words[(size_t)d * W + g] = bits;
            }
            __syncthreads();
            float *tmp = prev; prev = cur; cur = tmp;
        }
    }
    if (tid == 0) {
        const float score = prev[1 + Un] + jn[((size_t)(Tn - 1) * U1 + Un) * K];
        p.scores[n] = score;
        walk[0] = Un;
        walk[1] = score > ninf;
    }
    __syncthreads();
    if (!walk[1]) {
        for (int u = tid; u < Un; u += BLK) frames[u] = -1;
        return;
    }
    for (int dhi = dlast; dhi >= 1; dhi -= CHUNK) {
        const int g0 = walk[0] >> 6;
        for (int idx = tid; idx < CHUNK * 2; idx += BLK) {
            const int j = idx >> 1, d = dhi - j, g = g0 - (idx & 1);
            if (d >= 1 && g >= 0) stage[idx] = words[(size_t)d * W + g];
        }
        __syncthreads();
        if (tid == 0) {
            int u = walk[0];
            for (int j = 0; j < CHUNK; ++j) {
                const int d = dhi - j;
                if (d < 1) break;
                if ((stage[j * 2 + (g0 - (u >> 6))] >> (u & 63)) & 1) { frames[u - 1] = d - u; --u; }
            }
            walk[0] = u;
        }
        __syncthreads();
    }
}

// states (columns) per thread and frames (diagonals) of emissions in flight, by the lattice's width: one wave up to 64, then 256 threads
#define HALO_VITERBI_DISPATCH(KERNEL, width, grid, lds, stream, args)                                                       \
    do {                                                                                                                    \
        if ((width) <= 64) hipLaunchKernelGGL((KERNEL<64, 1, 8>), grid, dim3(64), lds(64), stream, args);                    \
        else if ((width) <= 256) hipLaunchKernelGGL((KERNEL<256, 1, 8>), grid, dim3(256), lds(256), stream, args);           \
        else if ((width) <= 512) hipLaunchKernelGGL((KERNEL<256, 2, 4>), grid, dim3(256), lds(512), stream, args);           \
        else if ((width) <= 1024) hipLaunchKernelGGL((KERNEL<256, 4, 2>), grid, dim3(256), lds(1024), stream, args);         \
        else if ((width) <= 2048) hipLaunchKernelGGL((KERNEL<256, 8, 2>), grid, dim3(256), lds(2048), stream, args);         \
        else if ((width) <= 4096) hipLaunchKernelGGL((KERNEL<256, 16, 1>), grid, dim3(256), lds(4096), stream, args);        \
        else hipLaunchKernelGGL((KERNEL<256, 30, 1>), grid, dim3(256), lds(7680), stream, args);                             \
    } while (0)

constexpr int MAX_WIDTH = 7679;  // states of a CTC lattice, columns of a transducer lattice: the lattice kernels' bound (30 x 256 = 7680)

}  // namespace

extern "C" {

size_t halo_ctc_viterbi_workspace_bytes(int T, int N, int S) {
    if (T <= 0 || N <= 0 || S < 0) return 0;
    return (size_t)N * T * ((2 * (size_t)S + 1 + 63) / 64) * 2 * sizeof(u64);
}

int halo_ctc_viterbi(const float *lp, long stride_t, long stride_n, int T, int N, int C, const int64_t *targets, long tg_stride, int S,
                     const int64_t *input_lengths, const int64_t *target_lengths, void *workspace, float *scores, int64_t *alignments,
                     int *starts, int *ends, halo_stream_t stream) {
    HALO_CHECK_ARG(lp && targets && target_lengths && workspace && scores && alignments && starts && ends);
    HALO_CHECK_ARG(T > 0 && N > 0 && C > 0 && S >= 1 && tg_stride >= S);
    if (2 * (long)S + 1 > MAX_WIDTH) return HALO_ENOTSUP;
    CtcViterbiArgs a;
    a.lp = lp; a.stride_t = stride_t; a.stride_n = stride_n; a.T = T; a.N = N; a.C = C; a.targets = targets; a.tg_stride = tg_stride;
    a.S = S; a.il = input_lengths; a.tl = target_lengths; a.words = (u64 *)workspace; a.G = (2 * S + 1 + 63) / 64;
    a.scores = scores; a.alignments = alignments; a.starts = starts; a.ends = ends;
#define CTC_ROWS(w) (2 * ((size_t)(w) + 2) * sizeof(float))
    HALO_VITERBI_DISPATCH(ctc_viterbi_kernel, 2 * S + 1, dim3(N), CTC_ROWS, (hipStream_t)stream, a);
#undef CTC_ROWS
    return halo_launch_status();
}

size_t halo_transducer_viterbi_workspace_bytes(int N, int T, int U1) {
    if (N <= 0 || T <= 0 || U1 <= 0) return 0;
    return (size_t)N * ((size_t)T + U1 - 1) * (((size_t)U1 + 63) / 64) * sizeof(u64);
}

int halo_transducer_viterbi(const float *joint, int N, int T, int U1, int K, const int64_t *targets, const int *joint_lengths,
                            const int *target_lengths, void *workspace, float *scores, int *frames, halo_stream_t stream) {
    HALO_CHECK_ARG(joint && targets && joint_lengths && target_lengths && workspace && scores && frames);
    HALO_CHECK_ARG(N > 0 && T > 0 && U1 >= 2 && K > 0);
    if (U1 > MAX_WIDTH) return HALO_ENOTSUP;
    TransducerViterbiArgs a;
    a.joint = joint; a.N = N; a.T = T; a.U1 = U1; a.K = K; a.targets = targets; a.j_len = joint_lengths; a.t_len = target_lengths;
    a.words = (u64 *)workspace; a.W = (U1 + 63) / 64; a.scores = scores; a.frames = frames;
#define DIAG_ROWS(w) (2 * ((size_t)(w) + 1) * sizeof(float))
    HALO_VITERBI_DISPATCH(transducer_viterbi_kernel, U1, dim3(N), DIAG_ROWS, (hipStream_t)stream, a);
#undef DIAG_ROWS
    return halo_launch_status();
}

}  // extern "C"
